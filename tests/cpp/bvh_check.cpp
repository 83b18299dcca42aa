// bvh_check.cpp — host-side invariants of the BVH4 builder (csrc/bvh_build.cpp), built with
// -fsanitize=address,undefined by tests/test_bvh_builder.py. Triangle soups come from a seeded LCG,
// including degenerate cases (zero-area, duplicated, coincident centroids, huge coordinates).
//   every input triangle is the child of exactly one node (a leaf is one triangle); child refs are in range and
//   form a tree (each interior node referenced once); the slots of a node hold its triangles first, then its nodes,
//   then empty slots; the device node's implicit addressing (tri_base + slot, child_base + slot - n_tri) reproduces
//   the explicit refs; every full-precision child box contains its subtree's triangles; every quantised box contains
//   the full-precision box; empty slots are inverted boxes; level_start describes the breadth-first levels.
// Every tree is also held to check_tree (csrc/bvh_invariants.h: the statement of the same invariants on the device's arrays alone,
// which uh_check_acceleration runs on trees written by the GPU), with packets and corners baked from tri_order as the context bakes
// them: the host builder is its reference and must pass with no violation. A mutation section then breaks a tree in ten ways, one
// per kind of fault check_tree exists to find, and expects each to be reported in its class ("MUTATIONS k/k caught").
// The node test's arithmetic (csrc/node_slab.h, the very text node_compute of traversal.h compiles) against the triangle test's
// (tri_compute of traversal.h, restated here with fmaf in the same order), for rays that start up to 1e6 away from the geometry:
//   for every (ray, triangle) pair the triangle test accepts, every slot on the way from the root to the triangle's leaf passes
//   the node test - with idir as the host computes it (correctly rounded) and with every component one ulp up and one ulp down
//   (the hardware reciprocal is good to one ulp).
// `bvh_check count` prints the number of culled pairs instead of failing on them: with -DUH_SLAB_MARGIN=... that measures the
// smallest margin that culls nothing (DESIGN.md "Arithmetic contract").
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "bvh.h"
#include "bvh_invariants.h"
#include "node_slab.h"

using namespace uh;

static uint32_t g_state = 1;
static float rnd() {
   g_state = g_state * 747796405u + 1u;
   uint32_t w = ((g_state >> ((g_state >> 28) + 4u)) ^ g_state) * 277803737u;
   w = (w >> 22) ^ w;
   return (float)w / 4294967296.0f;
}

static double rnd64() { return ((double)(uint32_t)(rnd() * 4294967296.0f) + 0.5) / 4294967296.0; }  // (0, 1)

static bool g_count_only = false;
static int g_mutations_caught = 0, g_mutations_tried = 0;
static unsigned long long g_culled = 0, g_accepted = 0;

struct F3 {
   float x, y, z;
};
static F3 operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static float dot_fma(F3 a, F3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
static F3 cross_fma(F3 a, F3 b) { return {std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)), std::fmaf(a.x, b.y, -(a.y * b.x))}; }

// tri_compute of traversal.h on a packet baked as scene_build.hip bakes it (v0, e1 = v1 - v0, e2 = v2 - v0 in float): true when a
// ray that has found nothing yet (best.t = tmax) accepts the triangle; *t_out = its parameter
static bool tri_accepts(const float* c, F3 o, F3 d, float tmin, float tmax, float* t_out) {
   const F3 v0 = {c[0], c[1], c[2]}, e1 = {c[3] - c[0], c[4] - c[1], c[5] - c[2]}, e2 = {c[6] - c[0], c[7] - c[1], c[8] - c[2]};
   const F3 p = cross_fma(d, e2);
   const float det = dot_fma(e1, p);
   if (det == 0.0f) return false;
   const float inv = 1.0f / det;
   const F3 tv = o - v0;
   const float u = dot_fma(tv, p) * inv;
   if (!(u >= 0.0f && u <= 1.0f)) return false;
   const F3 q = cross_fma(tv, e1);
   const float v = dot_fma(d, q) * inv;
   if (!(v >= 0.0f && u + v <= 1.0f)) return false;
   const float t = dot_fma(e2, q) * inv;
   if (!(t > tmin) || !(t < tmax)) return false;
   *t_out = t;
   return true;
}

static float safe_rcp_dir(float x) { return 1.0f / (std::fabs(x) < 1e-30f ? std::copysign(1e-30f, x) : x); }  // traversal.h, with the host's division

// node_compute of traversal.h for one slot: the planes by the text the kernel compiles (node_slab.h); tcap = the t of the hit
// that must not be lost (whatever the walk has found by then is no nearer, or the triangle does not matter)
static bool slot_passes(const Node4C& q, int k, F3 o, F3 idir, float tmin, float tcap) {
   const float ov[3] = {o.x, o.y, o.z}, iv[3] = {idir.x, idir.y, idir.z};
   float tnear = tmin, tfar = tcap, step[3], d[3];
   for (int a = 0; a < 3; a++) {
      const uint32_t bits = ((q.meta >> (8 * a)) & 0xffu) << 23;
      std::memcpy(&step[a], &bits, 4);
      d[a] = q.origin[a] - ov[a];
   }
   const float growth = slab_node_growth(d[0], step[0], d[1], step[1], d[2], step[2]);
   for (int a = 0; a < 3; a++) {
      float sa, bn, bf;
      slab_axis(d[a], step[a], iv[a], growth, sa, bn, bf);
      const bool neg = iv[a] < 0.0f;
      const uint32_t qn = ((neg ? q.qhi[a] : q.qlo[a]) >> (8 * k)) & 0xffu, qf = ((neg ? q.qlo[a] : q.qhi[a]) >> (8 * k)) & 0xffu;
      tnear = std::fmax(tnear, slab_t(qn, sa, bn));
      tfar = std::fmin(tfar, slab_t(qf, sa, bf));
   }
   return tnear <= tfar;
}

// rays from `distance` away towards points of the triangles (a third anywhere on one, a third within 2e-7 * distance of one of
// its edges on the inside, a third exactly at a vertex), from directions within acos(0.3) of the triangle's normal; direction =
// target - origin, unnormalised (t about 1) or of unit length (t about distance). Every ray is held against `near` triangles: the
// one it aims at and those after it in packet order (its neighbours in the tree), or all of them.
static int far_ray_check(const std::vector<float>& corners, const BuildOutput& out, const char* name, int rays, uint32_t near) {
   const uint32_t n = (uint32_t)(corners.size() / 9);
   if (n == 0 || out.cnodes.empty()) return 0;
   std::vector<uint32_t> up_node(out.cnodes.size(), kEmptyRef), up_slot(out.cnodes.size(), 0), leaf_node(n, kEmptyRef), leaf_slot(n, 0);
   for (uint32_t ni = 0; ni < out.nodes.size(); ni++)
      for (uint32_t k = 0; k < 4; k++) {
         const uint32_t c = out.nodes[ni].child[k];
         if (c == kEmptyRef) continue;
         if (c & kLeafBit) {
            if ((c & ~kLeafBit) < n) leaf_node[c & ~kLeafBit] = ni, leaf_slot[c & ~kLeafBit] = k;
         } else if (c < out.cnodes.size()) {
            up_node[c] = ni, up_slot[c] = k;
         }
      }
   unsigned long long accepted = 0, culled = 0;
   int errors = 0;
   const double distances[5] = {1e2, 3e3, 1e4, 1e5, 1e6};
   for (int di = 0; di < 5; di++)
      for (int unit = 0; unit < (distances[di] <= 3e3 ? 2 : 1); unit++)
         for (int r = 0; r < rays; r++) {
            const double D = distances[di];
            const uint32_t p = std::min(n - 1, (uint32_t)(rnd64() * n));
            const float* c = &corners[9 * (size_t)out.tri_order[p]];
            double w[3] = {rnd64(), rnd64(), rnd64()};
            if (r % 3 == 2) {
               const int v = (int)(rnd64() * 3) % 3;
               w[0] = v == 0, w[1] = v == 1, w[2] = v == 2;
            } else {
               if (w[0] + w[1] > 1.0) w[0] = 1.0 - w[0], w[1] = 1.0 - w[1];
               w[2] = 1.0 - w[0] - w[1];
               if (r % 3 == 1) {
                  // towards an edge: the weight of the opposite vertex = distance from the edge / height over it <= 2e-7 D / height
                  const int v = (int)(rnd64() * 3) % 3, i1 = (v + 1) % 3, i2 = (v + 2) % 3;
                  double e[3], f[3];
                  for (int a = 0; a < 3; a++) e[a] = (double)c[3 * i2 + a] - c[3 * i1 + a], f[a] = (double)c[3 * v + a] - c[3 * i1 + a];
                  const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], fe = f[0] * e[0] + f[1] * e[1] + f[2] * e[2];
                  const double h2 = f[0] * f[0] + f[1] * f[1] + f[2] * f[2] - (ee > 0 ? fe * fe / ee : 0.0);
                  const double wv = h2 > 0 ? std::fmin(1.0, rnd64() * 2e-7 * D / std::sqrt(h2)) : 0.0, s = rnd64();
                  w[v] = wv, w[i1] = (1.0 - wv) * s, w[i2] = (1.0 - wv) * (1.0 - s);
               }
            }
            double tg[3], nrm[3];
            for (int a = 0; a < 3; a++) tg[a] = (double)(float)(w[0] * c[a] + w[1] * c[3 + a] + w[2] * c[6 + a]);
            {
               const double e1[3] = {(double)c[3] - c[0], (double)c[4] - c[1], (double)c[5] - c[2]}, e2[3] = {(double)c[6] - c[0], (double)c[7] - c[1], (double)c[8] - c[2]};
               nrm[0] = e1[1] * e2[2] - e1[2] * e2[1], nrm[1] = e1[2] * e2[0] - e1[0] * e2[2], nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
               const double l = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
               if (l > 0) nrm[0] /= l, nrm[1] /= l, nrm[2] /= l; else nrm[0] = 0, nrm[1] = 0, nrm[2] = 1;
            }
            // a unit vector with cos to the normal uniform in [0.3, 1]
            double tx[3] = {std::fabs(nrm[0]) < 0.9 ? 1.0 : 0.0, std::fabs(nrm[0]) < 0.9 ? 0.0 : 1.0, 0.0}, bx[3];
            const double tn = tx[0] * nrm[0] + tx[1] * nrm[1] + tx[2] * nrm[2];
            for (int a = 0; a < 3; a++) tx[a] -= tn * nrm[a];
            const double tl = std::sqrt(tx[0] * tx[0] + tx[1] * tx[1] + tx[2] * tx[2]);
            for (int a = 0; a < 3; a++) tx[a] /= tl;
            bx[0] = nrm[1] * tx[2] - nrm[2] * tx[1], bx[1] = nrm[2] * tx[0] - nrm[0] * tx[2], bx[2] = nrm[0] * tx[1] - nrm[1] * tx[0];
            const double cz = 0.3 + 0.7 * rnd64(), sz = std::sqrt(1.0 - cz * cz), phi = 6.283185307179586 * rnd64();
            float of[3], df[3];
            double len = 0;
            for (int a = 0; a < 3; a++) {
               of[a] = (float)(tg[a] + D * (cz * nrm[a] + sz * (std::cos(phi) * tx[a] + std::sin(phi) * bx[a])));
               len += (tg[a] - (double)of[a]) * (tg[a] - (double)of[a]);
            }
            for (int a = 0; a < 3; a++) df[a] = (float)((tg[a] - (double)of[a]) / (unit ? std::sqrt(len) : 1.0));
            const F3 o = {of[0], of[1], of[2]}, d = {df[0], df[1], df[2]};
            const float tmin = 0.001f, tmax = 10000.0f;
            const uint32_t first = near >= n ? 0 : p, last = near >= n ? n : std::min(n, p + near);
            for (uint32_t j = first; j < last; j++) {
               float t;
               if (!tri_accepts(&corners[9 * (size_t)out.tri_order[j]], o, d, tmin, tmax, &t)) continue;
               accepted++;
               for (int ulp = -1; ulp <= 1; ulp++) {
                  F3 idir = {safe_rcp_dir(d.x), safe_rcp_dir(d.y), safe_rcp_dir(d.z)};
                  if (ulp) {
                     const float to = ulp > 0 ? INFINITY : -INFINITY;
                     idir = {std::nextafterf(idir.x, to), std::nextafterf(idir.y, to), std::nextafterf(idir.z, to)};
                  }
                  bool lost = false;
                  for (uint32_t node = leaf_node[j], slot = leaf_slot[j]; node != kEmptyRef && !lost; slot = up_slot[node], node = up_node[node])
                     lost = !slot_passes(out.cnodes[node], (int)slot, o, idir, tmin, t);
                  if (lost) {
                     culled++;
                     if (!g_count_only && errors++ < 5)
                        std::printf("FAIL[%s]: the node test culls a triangle the triangle test accepts (packet %u, distance %g, idir %+d ulp, t %g)\n", name, j, D, ulp, (double)t);
                  }
               }
            }
         }
   g_accepted += accepted, g_culled += culled;
   std::printf("%s: far rays: %llu accepted (ray, triangle) pairs, %llu culled on the way to the leaf (3 reciprocals each)\n", name, accepted, culled);
   if (accepted < (unsigned long long)rays) {
      std::printf("FAIL[%s]: the far rays hit too little for the check to mean anything\n", name);
      errors++;
   }
   return g_count_only ? 0 : errors;
}

// a host-built tree as the context uploads it (scene_build.hip uh_build_acceleration): packets and world corners in leaf order
struct DeviceForm {
   std::vector<Node4C> nodes;
   std::vector<TriPacket> packets;
   std::vector<float> corners;
   std::vector<uint32_t> mesh, level_start, keys;  // keys: the scene's, ascending
   DeviceForm(const std::vector<float>& soup, const std::vector<uint32_t>& soup_keys, const BuildOutput& out) : nodes(out.cnodes), level_start(out.level_start), keys(soup_keys) {
      const size_t n = out.tri_order.size();
      packets.resize(n);
      corners.resize(9 * n);
      mesh.resize(n);
      for (size_t i = 0; i < n; i++) {
         const uint32_t src = out.tri_order[i];
         if (src >= soup_keys.size()) continue;  // (reported by check())
         const float* c = &soup[9 * (size_t)src];
         std::memcpy(&corners[9 * i], c, 9 * sizeof(float));
         TriPacket& q = packets[i];
         q.v0[0] = c[0], q.v0[1] = c[1], q.v0[2] = c[2];
         q.e1x = c[3] - c[0], q.e1yz[0] = c[4] - c[1], q.e1yz[1] = c[5] - c[2];
         q.e2[0] = c[6] - c[0], q.e2[1] = c[7] - c[1], q.e2z = c[8] - c[2];
         q.key = soup_keys[src];
         q.pad[0] = q.pad[1] = 0;
         mesh[i] = q.key >> kPrimBits;
      }
      std::sort(keys.begin(), keys.end());
   }
   TreeView view() const {
      TreeView v;
      v.nodes = nodes.data(), v.num_nodes = (uint32_t)nodes.size();
      v.packets = packets.data(), v.num_tris = (uint32_t)packets.size();
      v.corners = corners.data();
      v.shade_mesh = mesh.data(), v.shade_stride = sizeof(uint32_t);
      v.level_start = level_start.data(), v.level_entries = (uint32_t)level_start.size();
      v.keys = keys.data(), v.num_keys = (uint32_t)keys.size();
      return v;
   }
};

// check_tree must find each of these in its class, and nothing in the tree they were made from
static int mutation_check(const std::vector<float>& soup, const char* name, int* caught, int* tried) {
   std::vector<uint32_t> keys(soup.size() / 9);
   for (uint32_t i = 0; i < keys.size(); i++) keys[i] = i;
   BuildInput in{soup.data(), keys.data(), (uint32_t)keys.size()};
   BuildOutput out;
   build_bvh4(in, out, 2);
   const DeviceForm good(soup, keys, out);
   int errors = 0;
   if (check_tree(good.view()).total()) {
      std::printf("FAIL[%s]: the tree the mutations start from has violations: %s\n", name, check_tree(good.view()).text().c_str());
      return 1;
   }
   std::vector<uint32_t> level_of(good.nodes.size(), 0);
   for (uint32_t l = 0; l + 1 < good.level_start.size(); l++)
      for (uint32_t i = good.level_start[l]; i < good.level_start[l + 1]; i++) level_of[i] = l;
   auto n_tri = [](const Node4C& q) { return (q.meta >> kMetaTriShift) & 7u; };
   auto n_child = [](const Node4C& q) { return (q.meta >> kMetaChildShift) & 7u; };
   // the last node (deep in the tree) that `want` accepts
   auto find = [&](auto want) {
      for (uint32_t i = (uint32_t)good.nodes.size(); i-- > 0;)
         if (want(good.nodes[i])) return (int64_t)i;
      return (int64_t)-1;
   };
   auto set_byte = [](uint32_t& w, uint32_t k, uint32_t b) { w = (w & ~(0xffu << (8 * k))) | (b << (8 * k)); };
   struct Mutation {
      const char* what;
      int cls;
      std::function<bool(DeviceForm&)> apply;  // false: the tree has no place for it
   };
   const int64_t with_tri = find([&](const Node4C& q) { return n_tri(q) >= 1; }), with_node = find([&](const Node4C& q) { return n_child(q) > n_tri(q); }),
                 with_empty = find([&](const Node4C& q) { return n_child(q) < 4; });
   const std::vector<Mutation> mutations = {
      {"a plane of a triangle slot moved inwards past the padded box", kTcContainment, [&](DeviceForm& t) {
          if (with_tri < 0) return false;
          set_byte(t.nodes[with_tri].qlo[0], 0, t.nodes[with_tri].qhi[0] & 0xffu);  // the lower x plane onto the upper one
          return true;
       }},
      {"a plane of a node slot moved inwards past the padded box", kTcContainment, [&](DeviceForm& t) {
          if (with_node < 0) return false;
          Node4C& q = t.nodes[with_node];
          const uint32_t k = n_tri(q);
          set_byte(q.qhi[1], k, (q.qlo[1] >> (8 * k)) & 0xffu);  // the upper y plane onto the lower one
          return true;
       }},
      {"meta's n_child lowered by one", kTcRefs, [&](DeviceForm& t) {
          if (with_node < 0) return false;
          t.nodes[with_node].meta -= 1u << kMetaChildShift;  // its last node child is no longer referenced
          return true;
       }},
      {"child_base's n_tri bits differ from meta's", kTcCounts, [&](DeviceForm& t) {
          t.nodes[0].child_base ^= 1u << kChildBaseBits;
          return true;
       }},
      {"tri_base shifted by one", kTcRefs, [&](DeviceForm& t) {
          if (with_tri < 0) return false;
          t.nodes[with_tri].tri_base += 1;
          return true;
       }},
      {"a child_base points into its own level", kTcLevels, [&](DeviceForm& t) {
          if (with_node < 0) return false;
          Node4C& q = t.nodes[with_node];
          q.child_base = (q.child_base & ~kChildBaseMask) | t.level_start[level_of[with_node]];
          return true;
       }},
      {"an empty slot given a real box", kTcEmpty, [&](DeviceForm& t) {
          if (with_empty < 0) return false;
          Node4C& q = t.nodes[with_empty];
          set_byte(q.qlo[2], n_child(q), 0u);
          set_byte(q.qhi[2], n_child(q), 255u);
          return true;
       }},
      {"an exponent byte set to 0", kTcCounts, [&](DeviceForm& t) {
          t.nodes[t.nodes.size() / 2].meta &= ~0xff00u;
          return true;
       }},
      {"a packet's e1 changed by an ulp", kTcPackets, [&](DeviceForm& t) {
          float& e = t.packets[t.packets.size() / 3].e1x;
          e = std::nextafterf(e, INFINITY);
          return true;
       }},
      {"one key duplicated over another", kTcKeys, [&](DeviceForm& t) {
          if (t.packets.size() < 2) return false;
          t.packets[1].key = t.packets[0].key;
          return true;
       }},
   };
   for (const Mutation& m : mutations) {
      DeviceForm t = good;
      ++*tried;
      const bool applied = m.apply(t);
      const TreeReport rep = applied ? check_tree(t.view()) : TreeReport();
      if (applied && rep.violations[m.cls]) {
         ++*caught;
      } else {
         std::printf("FAIL[%s]: %s: %s\n", name, m.what, applied ? ("not reported as " + std::string(tree_class_name(m.cls)) + "; check_tree says: " + rep.text()).c_str() : "the tree has no place for it");
         errors++;
      }
   }
   // (every mutation worked on a copy: the tree they share is as it was)
   if (check_tree(good.view()).total()) {
      std::printf("FAIL[%s]: the restored tree has violations\n", name);
      errors++;
   }
   return errors;
}

static int check(const std::vector<float>& corners, int threads, const char* name, bool geometry = true, int far_rays = 0, uint32_t near = 16, bool too_deep = false) {
   const uint32_t n = (uint32_t)(corners.size() / 9);
   std::vector<uint32_t> keys(n);
   for (uint32_t i = 0; i < n; i++) keys[i] = i;
   BuildInput in{corners.data(), keys.data(), n};
   BuildOutput out;
   build_bvh4(in, out, threads);
   int errors = 0;
   {
      // the same tree through the statement that device-built trees are held to: no violation, and it skips the geometry exactly
      // where this check is told to. too_deep: the one tree here that the context would not install - its depth is the one finding
      const DeviceForm dev(corners, keys, out);
      const TreeReport rep = check_tree(dev.view());
      std::printf("%s: check_tree: %u levels, SAH figure %.3f, %s%s\n", name, rep.levels, rep.sah, rep.text().c_str(), rep.geometry ? "" : " (non-finite corners: containment skipped)");
      if (rep.total() != (too_deep ? 1u : 0u) || rep.violations[kTcLevels] != (too_deep ? 1u : 0u) || rep.geometry != geometry) {
         std::printf("FAIL[%s]: check_tree on the host builder's tree\n", name);
         errors++;
      }
   }
   auto fail = [&](const char* what, uint32_t a, uint32_t b) {
      if (errors++ < 5) std::printf("FAIL[%s]: %s (%u, %u)\n", name, what, a, b);
   };
   if (out.nodes.empty() || out.nodes.size() != out.cnodes.size()) fail("node arrays", (uint32_t)out.nodes.size(), (uint32_t)out.cnodes.size());
   if (out.level_start.size() < 2 || out.level_start.front() != 0 || out.level_start.back() != out.nodes.size()) fail("level_start", (uint32_t)out.level_start.size(), 0);
   if (out.max_depth + 2 != out.level_start.size()) fail("max_depth vs levels", out.max_depth, (uint32_t)out.level_start.size());
   if (out.tri_order.size() != n) fail("tri_order size", (uint32_t)out.tri_order.size(), n);
   std::vector<uint32_t> seen(n, 0), node_refs(out.nodes.size(), 0);
   std::vector<uint32_t> packet_use(n, 0);
   for (uint32_t i = 0; i < out.tri_order.size(); i++) {
      if (out.tri_order[i] >= n) fail("tri_order entry out of range", i, out.tri_order[i]);
      else seen[out.tri_order[i]]++;
   }
   for (uint32_t i = 0; i < n; i++)
      if (seen[i] != 1) fail("triangle not exactly once in tri_order", i, seen[i]);
   // recursive subtree bounds
   struct Frame {
      uint32_t node;
   };
   std::vector<Frame> st{{0}};
   while (!st.empty()) {
      uint32_t ni = st.back().node;
      st.pop_back();
      const NodeW& nd = out.nodes[ni];
      const Node4C& q = out.cnodes[ni];
      float scale[3];
      for (int a = 0; a < 3; a++) scale[a] = std::ldexp(1.0f, (int)((q.meta >> (8 * a)) & 0xff) - 127);
      const uint32_t n_tri = (q.meta >> kMetaTriShift) & 7, n_child = (q.meta >> kMetaChildShift) & 7;
      if (n_tri > n_child || n_child > 4) fail("child counts", n_tri, n_child);
      if ((q.child_base >> kChildBaseBits) != n_tri) fail("n_tri is not in the top bits of child_base (what the traversal reads)", ni, q.child_base >> kChildBaseBits);
      for (int a = 0; a < 3; a++)
         if (((q.meta >> (8 * a)) & 0xff) < 1 || ((q.meta >> (8 * a)) & 0xff) > 254) fail("step exponent byte out of range", ni, (uint32_t)a);
      for (int k = 0; k < 4; k++) {
         uint32_t c = nd.child[k];
         const uint32_t implicit = (uint32_t)k < n_tri ? (kLeafBit | (q.tri_base + (uint32_t)k)) : ((uint32_t)k < n_child ? (q.child_base & kChildBaseMask) + ((uint32_t)k - n_tri) : kEmptyRef);
         if (implicit != c) fail("implicit child address differs from the explicit ref", ni, (uint32_t)k);
         if (c == kEmptyRef) {
            for (int a = 0; a < 3; a++)
               if (((q.qlo[a] >> (8 * k)) & 0xff) != 0xff || ((q.qhi[a] >> (8 * k)) & 0xff) != 0) fail("empty slot is not an inverted box", ni, (uint32_t)k);
            continue;
         }
         const float lo[3] = {nd.lo[0][k], nd.lo[1][k], nd.lo[2][k]}, hi[3] = {nd.hi[0][k], nd.hi[1][k], nd.hi[2][k]};
         for (int a = 0; a < 3; a++) {
            float qlo = q.origin[a] + scale[a] * (float)((q.qlo[a] >> (8 * k)) & 0xff);
            float qhi = q.origin[a] + scale[a] * (float)((q.qhi[a] >> (8 * k)) & 0xff);
            // the kernel evaluates origin + scale*q in t-space; in world space allow one ulp of the sum
            float slack = 4e-7f * std::fmax(std::fabs(lo[a]), std::fabs(hi[a])) + 1e-30f;
            if (geometry && (!(qlo <= lo[a] + slack) || !(qhi >= hi[a] - slack))) fail("quantised box does not contain the full box", ni, (uint32_t)(k * 3 + a));
         }
         if (c & kLeafBit) {
            const uint32_t p = c & ~kLeafBit;
            if (p >= n) {
               fail("packet index out of range", ni, p);
               continue;
            }
            {
               packet_use[p]++;
               const float* t = &corners[9 * (size_t)out.tri_order[p]];
               for (int v = 0; v < 3; v++)
                  for (int a = 0; a < 3; a++)
                     if (geometry && (!(t[3 * v + a] >= lo[a]) || !(t[3 * v + a] <= hi[a]))) fail("triangle outside its leaf box", ni, p);
            }
         } else {
            if (c >= out.nodes.size()) {
               fail("child index out of range", ni, c);
               continue;
            }
            node_refs[c]++;
            // child's own children must lie inside this slot's box (boxes are padded outwards at every level)
            const NodeW& ch = out.nodes[c];
            for (int j = 0; j < 4; j++)
               if (ch.child[j] != kEmptyRef) {
                  const float clo[3] = {ch.lo[0][j], ch.lo[1][j], ch.lo[2][j]}, chi[3] = {ch.hi[0][j], ch.hi[1][j], ch.hi[2][j]};
                  for (int a = 0; a < 3; a++) {
                     float pad = 2e-4f + 2e-5f * std::fmax(std::fabs(clo[a]), std::fabs(chi[a]));
                     if (geometry && (!(clo[a] >= lo[a] - pad) || !(chi[a] <= hi[a] + pad))) fail("grandchild box escapes its parent slot", ni, c);
                  }
               }
            st.push_back({c});
         }
      }
   }
   for (uint32_t p = 0; p < n; p++)
      if (packet_use[p] != 1) fail("packet not referenced by exactly one leaf", p, packet_use[p]);
   for (size_t i = 1; i < node_refs.size(); i++)
      if (node_refs[i] != 1) fail("interior node not referenced exactly once", (uint32_t)i, node_refs[i]);
   if (far_rays && !errors) errors += far_ray_check(corners, out, name, far_rays, near);
   std::printf("%s: %u tris -> %zu nodes, depth %u, %s\n", name, n, out.nodes.size(), out.max_depth, errors ? "FAILED" : "ok");
   return errors;
}

int main(int argc, char** argv) {
   g_count_only = argc > 1 && !std::strcmp(argv[1], "count");
   int errors = 0;
   for (uint32_t seed : {1u, 4u}) {
      for (int threads : {1, 4}) {
         std::vector<float> soup;
         g_state = 12345 + seed;
         for (int i = 0; i < 200000; i++) {
            float c[3] = {rnd() * 40 - 20, rnd() * 15, rnd() * 16 - 8};
            for (int v = 0; v < 3; v++)
               for (int a = 0; a < 3; a++) soup.push_back(c[a] + (rnd() - 0.5f) * 0.4f);
         }
         errors += check(soup, threads, "random soup", true, 6000);
      }
   }
   {
      std::vector<float> empty;
      errors += check(empty, 1, "empty");
      std::vector<float> one = {0, 0, 0, 1, 0, 0, 0, 1, 0};
      errors += check(one, 1, "single triangle", true, 40000);
      {
         // 32 x 32 quads on the unit square in the plane z = 0: small triangles in a coordinate plane, where the builders' box
         // padding is an absolute 1e-4
         std::vector<float> grid;
         for (int i = 0; i < 32; i++)
            for (int j = 0; j < 32; j++) {
               const float x0 = (float)i / 32, x1 = (float)(i + 1) / 32, y0 = (float)j / 32, y1 = (float)(j + 1) / 32;
               const float t[18] = {x0, y0, 0, x1, y0, 0, x1, y1, 0, x0, y0, 0, x1, y1, 0, x0, y1, 0};
               grid.insert(grid.end(), t, t + 18);
            }
         errors += check(grid, 2, "32 x 32 grid in z = 0", true, 2000, 0xffffffffu);
         errors += mutation_check(grid, "32 x 32 grid in z = 0", &g_mutations_caught, &g_mutations_tried);
      }
      {
         std::vector<float> soup;
         g_state = 20250;
         for (int i = 0; i < 5000; i++) {
            float c[3] = {rnd() * 40 - 20, rnd() * 15, rnd() * 16 - 8};
            for (int v = 0; v < 3; v++)
               for (int a = 0; a < 3; a++) soup.push_back(c[a] + (rnd() - 0.5f) * 0.4f);
         }
         errors += mutation_check(soup, "5000-triangle soup", &g_mutations_caught, &g_mutations_tried);
      }
      std::vector<float> dup;
      for (int i = 0; i < 1000; i++) dup.insert(dup.end(), one.begin(), one.end());
      errors += check(dup, 4, "1000 identical triangles");
      std::vector<float> degenerate;
      g_state = 7;
      for (int i = 0; i < 5000; i++) {
         float p[3] = {rnd(), rnd(), rnd()};
         for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) degenerate.push_back(p[a]);  // zero-area (point) triangles
      }
      errors += check(degenerate, 2, "point triangles");
      std::vector<float> huge;
      for (int i = 0; i < 3000; i++)
         for (int k = 0; k < 9; k++) huge.push_back((rnd() - 0.5f) * 2e6f);
      errors += check(huge, 2, "huge coordinates");
      std::vector<float> planar;
      for (int i = 0; i < 20000; i++) {
         float x = rnd() * 10, z = rnd() * 10;
         float t[9] = {x, 0, z, x + 0.1f, 0, z, x, 0, z + 0.1f};
         planar.insert(planar.end(), t, t + 9);
      }
      errors += check(planar, 4, "coplanar sheet", true, 12000);
      // non-finite vertices must not break the structure (every packet in exactly one leaf, no crash): such
      // triangles are never hit (NaN fails every comparison in the slab and triangle tests)
      std::vector<float> poisoned = planar;
      for (size_t i = 0; i < poisoned.size(); i += 997) poisoned[i] = (i & 1) ? NAN : ((i & 2) ? INFINITY : -INFINITY);
      errors += check(poisoned, 4, "NaN / inf vertices", false);
   }
   {
      // clusters on a geometric series (each a factor 0.5 closer to the origin than the one before): SAH peels them off one
      // by one and the tree becomes a chain. The traversal stack holds kTraversalStackEntries entries = kMaxTreeLevels
      // levels; the context rebuilds such a scene balanced (csrc/scene_build.hip), which must fit for any triangle count.
      std::vector<float> chain;
      g_state = 99;
      for (int k = 0; k < 120; k++) {
         const float s = std::ldexp(1.0f, -k);
         for (int i = 0; i < 3; i++) {
            float c[3] = {s * (1.0f + 0.1f * rnd()), s * 0.1f * rnd(), s * 0.1f * rnd()};
            for (int v = 0; v < 3; v++)
               for (int a = 0; a < 3; a++) chain.push_back(c[a] + s * 0.01f * rnd());
         }
      }
      errors += check(chain, 2, "geometric-series clusters (SAH)", true, 0, 16, true);
      std::vector<uint32_t> keys(chain.size() / 9);
      BuildInput in{chain.data(), keys.data(), (uint32_t)keys.size()};
      BuildOutput sah, bal;
      build_bvh4(in, sah, 1);
      build_bvh4(in, bal, 1, true);
      std::printf("geometric-series clusters: SAH tree %zu levels, balanced tree %zu levels (the stack holds %u)\n", sah.level_start.size() - 1, bal.level_start.size() - 1, kMaxTreeLevels);
      if (bal.level_start.size() - 1 > kMaxTreeLevels) {
         std::printf("FAIL: balanced tree deeper than the traversal stack\n");
         errors++;
      }
      {
         for (uint32_t i = 0; i < keys.size(); i++) keys[i] = i;
         const TreeReport rep = check_tree(DeviceForm(chain, keys, bal).view());
         std::printf("geometric-series clusters (balanced): check_tree: %u levels, SAH figure %.3f, %s\n", rep.levels, rep.sah, rep.text().c_str());
         errors += rep.total() ? 1 : 0;
      }
      if (sah.level_start.size() - 1 <= 12) {
         std::printf("FAIL: the chain scene no longer produces a deep SAH tree (test lost its point)\n");
         errors++;
      }
   }
   {
      // the same series with >= 65536 triangles and several threads: the serial top of the threaded build must honour
      // `balanced` too (it used to split by SAH whatever the flag said, and a deep clustered scene stayed too deep)
      std::vector<float> chain;
      g_state = 4242;
      for (int k = 0; k < 100; k++) {
         const float s = std::ldexp(1.0f, -k);
         for (int i = 0; i < 700; i++) {
            float c[3] = {s * (1.0f + 0.1f * rnd()), s * 0.1f * rnd(), s * 0.1f * rnd()};
            for (int v = 0; v < 3; v++)
               for (int a = 0; a < 3; a++) chain.push_back(c[a] + s * 0.01f * rnd());
         }
      }
      std::vector<uint32_t> keys(chain.size() / 9);
      BuildInput in{chain.data(), keys.data(), (uint32_t)keys.size()};
      BuildOutput sah, bal;
      build_bvh4(in, sah, 4);
      build_bvh4(in, bal, 4, true);
      std::printf("%zu clustered triangles, 4 threads: SAH tree %zu levels, balanced tree %zu levels (the stack holds %u)\n", keys.size(), sah.level_start.size() - 1,
                  bal.level_start.size() - 1, kMaxTreeLevels);
      if (keys.size() < 65536 || bal.level_start.size() - 1 > kMaxTreeLevels) {
         std::printf("FAIL: threaded balanced tree deeper than the traversal stack\n");
         errors++;
      }
   }
   {
      // build_sah_top (the host half of the device builder): a binary tree over boxes - count - 1 nodes, node 0 the root, every
      // box in exactly one leaf, every other node referenced exactly once, a node's area that of its leaves' union
      for (uint32_t count : {2u, 3u, 17u, 1000u, 5000u}) {
         std::vector<float> boxes;
         g_state = 4242 + count;
         for (uint32_t i = 0; i < count; i++) {
            float c[3] = {rnd() * 30 - 15, rnd() * 10, rnd() * 12 - 6}, e[3] = {rnd(), rnd() * 0.5f, rnd()};
            for (int a = 0; a < 3; a++) boxes.push_back(c[a] - e[a]);
            for (int a = 0; a < 3; a++) boxes.push_back(c[a] + e[a]);
         }
         if (count == 17) boxes.assign(boxes.size(), 0.25f);  // identical degenerate boxes: the split must still terminate
         std::vector<TopNode> top;
         build_sah_top(boxes.data(), count, top);
         int bad = top.size() != count - 1;
         std::vector<int> leaf_use(count, 0), node_use(top.size(), 0);
         for (size_t k = 0; k < top.size() && !bad; k++)
            for (uint32_t r : {top[k].left, top[k].right}) {
               if (r & kLeafBit) {
                  if ((r & ~kLeafBit) >= count) bad = 1; else leaf_use[r & ~kLeafBit]++;
               } else {
                  if (r >= top.size() || r == 0) bad = 1; else node_use[r]++;
               }
            }
         for (uint32_t i = 0; i < count; i++) bad |= leaf_use[i] != 1;
         for (size_t k = 1; k < top.size(); k++) bad |= node_use[k] != 1;
         if (!bad) {
            // area of the root = area of the union of all boxes
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (uint32_t i = 0; i < count; i++)
               for (int a = 0; a < 3; a++) lo[a] = std::fmin(lo[a], boxes[6 * i + a]), hi[a] = std::fmax(hi[a], boxes[6 * i + 3 + a]);
            const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
            bad |= top[0].half_area != dx * dy + dy * dz + dz * dx;
         }
         std::printf("SAH top over %u boxes: %zu nodes, %s\n", count, top.size(), bad ? "FAILED" : "ok");
         errors += bad;
      }
   }
   std::printf("far rays in all: %llu accepted (ray, triangle) pairs, %llu culled by the node test, margin %g\n", g_accepted, g_culled, (double)kSlabMargin);
   std::printf("MUTATIONS %d/%d caught\n", g_mutations_caught, g_mutations_tried);
   std::printf(errors ? "BVH CHECK FAILED (%d)\n" : "BVH CHECK OK\n", errors);
   return errors ? 1 : 0;
}
