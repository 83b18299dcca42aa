// bvh_invariants.h - what the traversal relies on in a tree AS THE DEVICE HOLDS IT (bvh.h: Node4C array, packet array, world corners,
// BFS levels), checked on the host in double. Host only, no HIP: the context's diagnostics call (uh_check_acceleration, scene_build.hip)
// runs it on the arrays it reads back, tests/cpp/bvh_check.cpp runs it on the host builder's output - its reference: those trees pass
// with no violation - and on mutated copies of them.
//
// It needs no full-precision node (NodeW): a slot's tight box is the union of the world corners of its subtree, and what its planes
// must contain is that box grown by the builders' padding (bvh_build.cpp padded(), refit.hip child_boxes: 1e-4 + 1e-5 * max|coord|
// per axis), less the rounding of `lo - pad` to float.
//   levels       level_start begins at 0, ends at the node count, no level is empty, at most kMaxTreeLevels of them (the traversal
//                stack drops subtrees beyond), every node child in a strictly later level than its parent (the refit's passes go
//                level by level)
//   counts       n_tri <= n_child <= 4, the top bits of child_base = meta's n_tri, every step-exponent byte in [1, 254]
//   refs         every node but the root referenced exactly once and the root never; every packet referenced by exactly one slot,
//                every reference in range
//   keys         the packets' keys are the scene's keys, each exactly once; the shade packet's mesh is key >> 22
//   packets      the packet is the bake of its world corners bit for bit: v0 = c0, e1 = c1 - c0, e2 = c2 - c0 in float
//   empty        an empty slot is the inverted box 255 / 0 on every axis
//   containment  qlo <= qhi, and origin + step * qlo / qhi contain the padded tight box of the slot's subtree (skipped for trees with
//                non-finite corners)
// and one figure that is reported only: the sum over used slots of the dequantised box's area over the root's (the union of the
// root's slots) - the SAH cost of the tree with both constants 1.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh.h"

namespace uh {

// the arrays of a tree; strides in bytes (the device arrays are 16 * kNodeStride16 / 16 * kTriStride16 apart, the host builder's
// sizeof(Node4C) / sizeof(TriPacket))
struct TreeView {
   const void* nodes = nullptr;
   size_t node_stride = sizeof(Node4C);
   uint32_t num_nodes = 0;
   const void* packets = nullptr;
   size_t packet_stride = sizeof(TriPacket);
   uint32_t num_tris = 0;
   const float* corners = nullptr;          // world corners, 9 floats per packet
   const void* shade_mesh = nullptr;        // packet i's mesh word at shade_mesh + i * shade_stride
   size_t shade_stride = sizeof(ShadePacket);
   const uint32_t* level_start = nullptr;   // level_count + 1 entries
   uint32_t level_entries = 0;
   const uint32_t* keys = nullptr;          // the scene's keys, ascending, num_keys of them
   uint32_t num_keys = 0;
};

enum TreeClass : int { kTcLevels, kTcCounts, kTcRefs, kTcKeys, kTcPackets, kTcEmpty, kTcContainment, kTreeClasses };
inline const char* tree_class_name(int k) {
   static const char* const names[kTreeClasses] = {"levels", "counts", "refs", "keys", "packets", "empty slots", "containment"};
   return names[k];
}

struct TreeReport {
   uint64_t violations[kTreeClasses] = {0, 0, 0, 0, 0, 0, 0};
   std::string first[kTreeClasses];  // the first offender of each class
   uint32_t levels = 0;
   bool geometry = true;             // false: non-finite corners, containment not checked
   double sah = 0.0;
   uint64_t total() const {
      uint64_t t = 0;
      for (uint64_t v : violations) t += v;
      return t;
   }
   std::string text() const {
      std::string s;
      for (int k = 0; k < kTreeClasses; k++)
         if (violations[k]) s += std::string(s.empty() ? "" : "; ") + tree_class_name(k) + ": " + std::to_string(violations[k]) + " (first: " + first[k] + ")";
      return s.empty() ? "no violation" : s;
   }
};

inline TreeReport check_tree(const TreeView& v) {
   TreeReport r;
   auto bad = [&](int cls, const char* what, uint64_t a, uint64_t b) {
      if (!r.violations[cls]++) {
         char buf[200];
         std::snprintf(buf, sizeof(buf), "%s (%llu, %llu)", what, (unsigned long long)a, (unsigned long long)b);
         r.first[cls] = buf;
      }
   };
   const uint32_t nn = v.num_nodes, nt = v.num_tris;
   auto node = [&](uint32_t i) {
      Node4C q;
      std::memcpy(&q, (const char*)v.nodes + v.node_stride * (size_t)i, sizeof(q));
      return q;
   };
   auto packet = [&](uint32_t i) {
      TriPacket p;
      std::memcpy(&p, (const char*)v.packets + v.packet_stride * (size_t)i, sizeof(p));
      return p;
   };

   // ---- levels ----
   r.levels = v.level_entries ? v.level_entries - 1 : 0;
   std::vector<uint32_t> level_of(nn, 0);
   bool levels_ok = v.level_entries >= 2 && v.level_start[0] == 0 && v.level_start[v.level_entries - 1] == nn;
   for (uint32_t l = 0; levels_ok && l + 1 < v.level_entries; l++) levels_ok = v.level_start[l] < v.level_start[l + 1];
   if (!levels_ok) {
      bad(kTcLevels, "level_start does not begin at 0, end at the node count and grow strictly: entries, nodes", v.level_entries, nn);
   } else {
      for (uint32_t l = 0; l + 1 < v.level_entries; l++)
         for (uint32_t i = v.level_start[l]; i < v.level_start[l + 1]; i++) level_of[i] = l;
   }
   if (nn == 0) bad(kTcLevels, "no root node", 0, 0);
   if (r.levels > kMaxTreeLevels) bad(kTcLevels, "more levels than the traversal stack holds: levels, kMaxTreeLevels", r.levels, kMaxTreeLevels);

   // ---- geometry: finite? ----
   for (size_t i = 0; i < 9 * (size_t)nt && r.geometry; i++) r.geometry = std::isfinite(v.corners[i]);

   // ---- counts, refs, empty slots; the nodes in descending order, so that a child's tight box exists before its parent asks for it
   // (a child at or before its parent is a violation of `levels` or `refs`, and its box is then left out) ----
   std::vector<uint32_t> node_refs(nn, 0), packet_refs(nt, 0);
   std::vector<double> tight(6 * (size_t)nn);  // lo xyz, hi xyz of the node's subtree
   double area_sum = 0.0, root_area = 0.0;
   for (uint32_t ni = nn; ni-- > 0;) {
      const Node4C q = node(ni);
      uint32_t n_tri = (q.meta >> kMetaTriShift) & 7u, n_child = (q.meta >> kMetaChildShift) & 7u;
      if (n_tri > n_child || n_child > 4) bad(kTcCounts, "not n_tri <= n_child <= 4 in node, meta", ni, q.meta);
      if ((q.child_base >> kChildBaseBits) != n_tri) bad(kTcCounts, "the top bits of child_base are not meta's n_tri in node, child_base", ni, q.child_base);
      double step[3];
      for (int a = 0; a < 3; a++) {
         const uint32_t e = (q.meta >> (8 * a)) & 0xffu;
         if (e < 1 || e > 254) bad(kTcCounts, "step exponent byte outside [1, 254] in node, axis", ni, (uint64_t)a);
         step[a] = std::ldexp(1.0, (int)e - 127);
      }
      n_child = std::min(n_child, 4u);
      n_tri = std::min(n_tri, n_child);
      double* tb = &tight[6 * (size_t)ni];
      for (int a = 0; a < 3; a++) tb[a] = INFINITY, tb[3 + a] = -INFINITY;
      double ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};  // union of the dequantised slots
      for (uint32_t k = 0; k < 4; k++) {
         uint32_t ql[3], qh[3];
         for (int a = 0; a < 3; a++) ql[a] = (q.qlo[a] >> (8 * k)) & 0xffu, qh[a] = (q.qhi[a] >> (8 * k)) & 0xffu;
         if (k >= n_child) {
            for (int a = 0; a < 3; a++)
               if (ql[a] != 0xffu || qh[a] != 0u) {
                  bad(kTcEmpty, "empty slot is not the inverted box 255 / 0: node, slot", ni, k);
                  break;
               }
            continue;
         }
         double slo[3] = {INFINITY, INFINITY, INFINITY}, shi[3] = {-INFINITY, -INFINITY, -INFINITY};
         bool have = false;
         if (k < n_tri) {
            const uint64_t p = (uint64_t)q.tri_base + k;
            if (p >= nt) {
               bad(kTcRefs, "packet index out of range: node, packet", ni, p);
            } else {
               packet_refs[p]++;
               have = true;
               const float* c = v.corners + 9 * (size_t)p;
               for (int w = 0; w < 3; w++)
                  for (int a = 0; a < 3; a++) slo[a] = std::fmin(slo[a], (double)c[3 * w + a]), shi[a] = std::fmax(shi[a], (double)c[3 * w + a]);
            }
         } else {
            const uint64_t ch = (uint64_t)(q.child_base & kChildBaseMask) + (k - n_tri);
            if (ch >= nn) {
               bad(kTcRefs, "child index out of range: node, child", ni, ch);
            } else {
               node_refs[ch]++;
               if (levels_ok && level_of[ch] <= level_of[ni]) bad(kTcLevels, "child not in a later level than its parent: node, child", ni, ch);
               if (ch > ni) {
                  have = true;
                  for (int a = 0; a < 3; a++) slo[a] = tight[6 * (size_t)ch + a], shi[a] = tight[6 * (size_t)ch + 3 + a];
               }
            }
         }
         double dlo[3], dhi[3];
         for (int a = 0; a < 3; a++) {
            dlo[a] = (double)q.origin[a] + step[a] * ql[a];
            dhi[a] = (double)q.origin[a] + step[a] * qh[a];
            ulo[a] = std::fmin(ulo[a], dlo[a]);
            uhi[a] = std::fmax(uhi[a], dhi[a]);
         }
         const double ex = std::fmax(0.0, dhi[0] - dlo[0]), ey = std::fmax(0.0, dhi[1] - dlo[1]), ez = std::fmax(0.0, dhi[2] - dlo[2]);
         area_sum += ex * ey + ey * ez + ez * ex;
         if (!have) continue;
         for (int a = 0; a < 3; a++) tb[a] = std::fmin(tb[a], slo[a]), tb[3 + a] = std::fmax(tb[3 + a], shi[a]);
         if (!r.geometry) continue;
         for (int a = 0; a < 3; a++) {
            if (!(slo[a] <= shi[a])) continue;  // a subtree without a triangle (only in a broken tree: counted above)
            const double pad = 1e-4 + 1e-5 * std::fmax(std::fabs(slo[a]), std::fabs(shi[a]));
            const double need_lo = slo[a] - pad, need_hi = shi[a] + pad;
            // the builders round lo - pad and hi + pad to float (and compute the pad in float): bvh_check.cpp's slack
            const double slack = 4e-7 * std::fmax(std::fabs(need_lo), std::fabs(need_hi)) + 1e-30;
            if (ql[a] > qh[a]) bad(kTcContainment, "qlo > qhi in a used slot: node, slot * 3 + axis", ni, 3 * k + (uint64_t)a);
            else if (!(dlo[a] <= need_lo + slack) || !(dhi[a] >= need_hi - slack))
               bad(kTcContainment, "planes do not contain the padded box of the subtree: node, slot * 3 + axis", ni, 3 * k + (uint64_t)a);
         }
      }
      if (ni == 0) {
         const double ex = std::fmax(0.0, uhi[0] - ulo[0]), ey = std::fmax(0.0, uhi[1] - ulo[1]), ez = std::fmax(0.0, uhi[2] - ulo[2]);
         root_area = ex * ey + ey * ez + ez * ex;
      }
   }
   r.sah = root_area > 0.0 && std::isfinite(area_sum) ? area_sum / root_area : 0.0;
   if (nn && node_refs[0] != 0) bad(kTcRefs, "the root is referenced: node, times", 0, node_refs[0]);
   for (uint32_t i = 1; i < nn; i++)
      if (node_refs[i] != 1) bad(kTcRefs, "node not referenced exactly once: node, times", i, node_refs[i]);
   for (uint32_t p = 0; p < nt; p++)
      if (packet_refs[p] != 1) bad(kTcRefs, "packet not referenced by exactly one slot: packet, times", p, packet_refs[p]);

   // ---- keys and packets ----
   std::vector<uint32_t> have_keys(nt);
   for (uint32_t p = 0; p < nt; p++) {
      const TriPacket t = packet(p);
      have_keys[p] = t.key;
      uint32_t mesh;
      std::memcpy(&mesh, (const char*)v.shade_mesh + v.shade_stride * (size_t)p, 4);
      if (mesh != (t.key >> kPrimBits)) bad(kTcKeys, "the shade packet's mesh is not key >> 22: packet, mesh", p, mesh);
      const float* c = v.corners + 9 * (size_t)p;
      const float want[9] = {c[0], c[1], c[2], c[3] - c[0], c[4] - c[1], c[5] - c[2], c[6] - c[0], c[7] - c[1], c[8] - c[2]};
      const float got[9] = {t.v0[0], t.v0[1], t.v0[2], t.e1x, t.e1yz[0], t.e1yz[1], t.e2[0], t.e2[1], t.e2z};
      for (int k = 0; k < 9; k++)
         if (std::memcmp(&want[k], &got[k], 4) != 0 && !(std::isnan(want[k]) && std::isnan(got[k]))) {  // (a NaN's payload is the machine's)
            bad(kTcPackets, "packet is not the bake of its world corners: packet, float", p, (uint64_t)k);
            break;
         }
   }
   std::sort(have_keys.begin(), have_keys.end());
   {
      // both lists ascending: a key of one that the other lacks (a duplicate is one too many), counted once each
      size_t i = 0, j = 0;
      while (i < have_keys.size() || j < v.num_keys) {
         if (j == v.num_keys || (i < have_keys.size() && have_keys[i] < v.keys[j])) bad(kTcKeys, "a packet's key is not the scene's, or is there twice: key, position", have_keys[i], i), i++;
         else if (i == have_keys.size() || v.keys[j] < have_keys[i]) bad(kTcKeys, "a key of the scene is in no packet: key, position", v.keys[j], j), j++;
         else i++, j++;
      }
   }
   return r;
}

}  // namespace uh
