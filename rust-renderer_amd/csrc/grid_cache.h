// grid_cache.h - when a cached visibility grid (sun_grid.h: the per-direction sun grid, the per-camera grid) is reused, waited for
// or rebuilt. A grid belongs to one (geometry version, key) pair - the key is the sun direction (3 floats) or inverse_view and
// inverse_projection (32) - and a build costs as much as a thousand frames' worth of what the grid saves: a pair other than the
// grid's is built for only once it has been asked for twice in a row, and the tree is walked meanwhile, so a sun, a camera or an
// instance that moves every frame never builds. Host code without HIP (tests/cpp/grid_cache_check.cpp replays the sequences the
// GPU tests hold the library to); the grid itself is context_state.h CachedGrid.
#pragma once
#include <cstdint>
#include <cstring>

namespace uh {

enum class GridDecision {
   Use,    // the grid, or the refusal, of this very pair is what there is: no build
   Wait,   // another pair than the grid's, not yet settled: walk the tree
   Build,  // build for this pair now, then built_for()
};

template <int N>
struct GridCache {
   uint64_t geom = 0, geom_pending = 0;         // the geometry version the grid was built (or refused) for / of the last request that waited
   float key[N] = {}, key_pending[N] = {};      // compared as bytes: -0.0 and 0.0 are different keys
   bool attempted = false;                      // a build for (geom, key) was tried; it may have been refused
   bool have_pending = false;

   bool matches(uint64_t g, const float* k) const { return geom == g && std::memcmp(k, key, sizeof(key)) == 0; }

   // first_at_once: with no build attempted (a new context, after invalidate()) the first request builds, and leaves the pending pair
   // alone (the sun grid; the camera grid waits for its second request even then). enough_frames: this request alone repays the
   // build (the camera grid's call that carries a batch of frames).
   GridDecision decide(uint64_t g, const float* k, bool first_at_once, bool enough_frames = false) {
      if (attempted && matches(g, k)) {
         have_pending = false;
         return GridDecision::Use;
      }
      if (!attempted && first_at_once) return GridDecision::Build;
      const bool settled = have_pending && geom_pending == g && std::memcmp(k, key_pending, sizeof(key)) == 0;
      std::memcpy(key_pending, k, sizeof(key));
      geom_pending = g;
      have_pending = true;
      return settled || enough_frames ? GridDecision::Build : GridDecision::Wait;
   }
   // a build for (g, k) was tried, whatever came of it
   void built_for(uint64_t g, const float* k) {
      attempted = true;
      have_pending = false;
      geom = g;
      std::memcpy(key, k, sizeof(key));
   }
   // what the grid was built with has changed (an option): the next request is a first one
   void invalidate() { attempted = false; }
};

}  // namespace uh
