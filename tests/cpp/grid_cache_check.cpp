// grid_cache_check.cpp - the rebuild policy of the sun and camera grids (csrc/grid_cache.h, product code) replayed on the host, under
// ASan + UBSan (tests/test_sanitizers.py): the request sequences of tests/test_gpu_sun_grid.py and tests/test_gpu_camera_grid.py
// (which see the builds through UhStats on a GPU) and the asymmetries between the two grids. A request is one ensure_*_grid call
// (csrc/grid_cache.hip) that got past its early exits: decide(), and built_for() when that said Build.
#include <cstdio>
#include <string>
#include <vector>

#include "grid_cache.h"

using namespace uh;

static int g_failures = 0;

static void expect(bool ok, const std::string& what) {
   if (!ok) {
      std::printf("FAIL: %s\n", what.c_str());
      g_failures++;
   }
}

static const char* name(GridDecision d) { return d == GridDecision::Use ? "use" : (d == GridDecision::Wait ? "wait" : "build"); }

// the sun grid's request: the first of all builds at once, no batch shortcut
static GridDecision sun_request(GridCache<3>& p, uint64_t geom, const float* dir) {
   const GridDecision d = p.decide(geom, dir, true);
   if (d == GridDecision::Build) p.built_for(geom, dir);
   return d;
}

// the camera grid's: even a first request waits, unless the call carries 8 frames or more
static GridDecision cam_request(GridCache<32>& p, uint64_t geom, const float* mats, uint32_t batch = 1) {
   const GridDecision d = p.decide(geom, mats, false, batch >= 8);
   if (d == GridDecision::Build) p.built_for(geom, mats);
   return d;
}

static void expect_seq(const std::vector<GridDecision>& got, const std::vector<GridDecision>& want, const std::string& what) {
   std::string g, w;
   for (GridDecision d : got) g += std::string(name(d)) + " ";
   for (GridDecision d : want) w += std::string(name(d)) + " ";
   expect(got == want, what + ": got " + g + "| expected " + w);
}

struct Mats {
   float m[32];
   explicit Mats(float seed) {
      for (int k = 0; k < 32; k++) m[k] = seed + 0.25f * (float)k;
   }
};

int main() {
   const GridDecision U = GridDecision::Use, W = GridDecision::Wait, B = GridDecision::Build;
   const float dirA[3] = {0.0f, 1.0f, 0.0f}, dirB[3] = {0.6f, 0.8f, 0.0f}, dirC[3] = {0.0f, 0.8f, 0.6f};

   {  // test_direction_changes_and_settling: A A B C B B B A A builds at requests 0, 5 and 8 and nowhere else
      GridCache<3> p;
      const float* seq[9] = {dirA, dirA, dirB, dirC, dirB, dirB, dirB, dirA, dirA};
      std::vector<GridDecision> got;
      for (const float* d : seq) got.push_back(sun_request(p, 1, d));
      expect_seq(got, {B, U, W, W, W, B, U, W, B}, "sun directions A A B C B B B A A");
   }
   {  // geometry that moves every frame never rebuilds: the version changes at requests 2-5 and is then still
      GridCache<3> p;
      const uint64_t geom[9] = {1, 1, 2, 3, 4, 5, 5, 5, 5};
      std::vector<GridDecision> got;
      for (uint64_t g : geom) got.push_back(sun_request(p, g, dirA));
      expect_seq(got, {B, U, W, W, W, W, B, U, U}, "sun grid under moving geometry");
   }
   {  // test_settling_moving_camera_and_geometry_changes
      GridCache<32> p;
      std::vector<GridDecision> got;
      for (int k = 0; k < 4; k++) got.push_back(cam_request(p, 1, Mats((float)k).m));  // four different cameras
      const Mats rest(10.0f), other(20.0f);
      got.push_back(cam_request(p, 1, rest.m));   // a fifth, seen for the first time
      got.push_back(cam_request(p, 1, rest.m));   // again: build
      got.push_back(cam_request(p, 1, rest.m));   // a hit
      got.push_back(cam_request(p, 1, other.m));  // a new camera: wait, then build
      got.push_back(cam_request(p, 1, other.m));
      got.push_back(cam_request(p, 2, other.m));  // a geometry bump: wait, then build
      got.push_back(cam_request(p, 2, other.m));
      got.push_back(cam_request(p, 2, other.m));
      expect_seq(got, {W, W, W, W, W, B, U, W, B, W, B, U}, "camera settling, moving camera, geometry bump");
   }
   {  // a first camera request that carries a batch of 8 frames builds at once, one of 7 does not; the sun grid has no such shortcut
      GridCache<32> p8, p7;
      const Mats m(1.0f);
      expect(cam_request(p8, 1, m.m, 8) == B, "camera: a first request with batch = 8 builds at once");
      expect(cam_request(p8, 1, m.m, 8) == U, "camera: and is a hit afterwards");
      expect(cam_request(p7, 1, m.m, 7) == W, "camera: a first request with batch = 7 waits");
      expect(cam_request(p7, 1, m.m, 7) == B, "camera: the second one builds");
   }
   {  // invalidate() (an option changed), then the same key: the sun grid builds at once, the camera grid waits once
      GridCache<3> s;
      expect(sun_request(s, 1, dirA) == B && sun_request(s, 1, dirA) == U, "sun: first build and hit");
      s.invalidate();
      expect(sun_request(s, 1, dirA) == B, "sun: builds at once after invalidate()");
      expect(sun_request(s, 1, dirA) == U, "sun: a hit after the rebuild");
      GridCache<32> c;
      const Mats m(3.0f);
      expect(cam_request(c, 1, m.m) == W && cam_request(c, 1, m.m) == B && cam_request(c, 1, m.m) == U, "camera: wait, build, hit");
      c.invalidate();
      expect(cam_request(c, 1, m.m) == W, "camera: waits once after invalidate()");
      expect(cam_request(c, 1, m.m) == B, "camera: then builds");
   }
   {  // a sun request with nothing attempted leaves the pending pair alone; a hit clears have_pending in both
      GridCache<3> s;
      (void)s.decide(1, dirA, true);
      expect(!s.have_pending && !s.attempted, "sun: a first request does not touch the pending pair");
      s.built_for(1, dirA);
      expect(sun_request(s, 1, dirB) == W && s.have_pending, "sun: another direction becomes the pending pair");
      expect(sun_request(s, 1, dirA) == U && !s.have_pending, "sun: a hit clears the pending pair");
      expect(sun_request(s, 1, dirB) == W, "sun: so the other direction has to settle anew");
      GridCache<32> c;
      const Mats m(4.0f), o(5.0f);
      (void)cam_request(c, 1, m.m);
      expect(c.have_pending, "camera: every request that is no hit is the pending pair");
      (void)cam_request(c, 1, m.m);
      expect(cam_request(c, 1, o.m) == W && cam_request(c, 1, m.m) == U && !c.have_pending && cam_request(c, 1, o.m) == W, "camera: a hit clears the pending pair");
   }
   {  // keys are compared as bytes: 0.0f and -0.0f are different keys
      GridCache<3> s;
      const float pos[3] = {0.0f, 1.0f, 0.0f}, neg[3] = {-0.0f, 1.0f, 0.0f};
      expect(sun_request(s, 1, pos) == B, "sun: first build");
      expect(!s.matches(1, neg) && s.matches(1, pos) && !s.matches(2, pos), "matches(): the key's bytes and the geometry version");
      expect(sun_request(s, 1, neg) == W && sun_request(s, 1, pos) == U && sun_request(s, 1, neg) == W && sun_request(s, 1, neg) == B, "sun: -0.0 is another direction than 0.0");
   }
   {  // a refused build - attempted, no valid grid - is a hit that yields nothing to use: it is not tried again on every frame
      GridCache<3> s;
      bool valid = true;
      if (s.decide(1, dirA, true) == B) {
         s.built_for(1, dirA);
         valid = false;  // the builder refused
      }
      int builds = 0;
      for (int k = 0; k < 5; k++) builds += sun_request(s, 1, dirA) != U;
      expect(s.attempted && !valid && builds == 0, "a refusal is kept: five more requests, no build");
   }
   if (g_failures) {
      std::printf("GRID CACHE CHECK FAILED: %d\n", g_failures);
      return 1;
   }
   std::printf("GRID CACHE CHECK OK\n");
   return 0;
}
