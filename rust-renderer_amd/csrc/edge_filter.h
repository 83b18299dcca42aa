// edge_filter.h — the edge-stopping tile filter of k_rtao_resolve<true>, k_rtgi_filter, k_glossy_filter and k_fog_resolve<true>: a block is a kFilterTileW x kFilterTileH tile
// of G-buffer pixels, one lane per pixel, tiles numbered along x first. The tile and its halo (the blur radius r <= kMaxR on every side)
// of (P, Nn, kPlanes value planes) are staged in LDS once per block; a tap counts when it is the centre or dot(nt, nn) >= normal_cos and
// |dot(Pt - P, nn)| <= plane. Staging and taps run dy outer, dx inner: the order of the callers' sums, which their tests hold bit for bit.
#pragma once
#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"

namespace uh {

constexpr int kFilterTileW = 32, kFilterTileH = kBlock / kFilterTileW;
static inline dim3 filter_grid(const HybridDev& hd) {
   return dim3(((hd.W + kFilterTileW - 1) / kFilterTileW) * ((hd.H + kFilterTileH - 1) / kFilterTileH));
}

// a lane's pixel (it may lie outside the frame) and its record in the tile staged for radius r
struct FilterLane {
   int x0, y0, px, py, centre;  // x0, y0: the tile's first pixel
};
__device__ __forceinline__ FilterLane filter_lane(const HybridDev& hd, int r) {
   const int tx = (int)threadIdx.x % kFilterTileW, ty = (int)threadIdx.x / kFilterTileW;
   const int tiles_x = ((int)hd.W + kFilterTileW - 1) / kFilterTileW;
   const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * kFilterTileW, y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * kFilterTileH;
   return {x0, y0, x0 + tx, y0 + ty, (ty + r) * (kFilterTileW + 2 * r) + (tx + r)};
}

template <int kMaxR, int kPlanes>
struct FilterTile {
   static constexpr int kRecords = (kFilterTileW + 2 * kMaxR) * (kFilterTileH + 2 * kMaxR);
   using Rec = float[6 + kPlanes][kRecords];  // planes of the staged records: P, Nn, then the values
   using Valid = uint8_t[kRecords];           // the record can be a tap: inside the frame, a pixel that cast
   // Two __shared__ arrays of the kernel, not one object: in one the compiler forms a plane's byte offset from the validity byte's
   // index (3 i + i), a vector instruction more per tap, and both filters measured 0.5 to 1 % slower.
   Rec& rec;
   Valid& valid;

   // every lane of the block: stages the tile for radius r and waits for it; value(g, i) stores pixel g's values in rec[6...][i]
   template <typename Value>
   __device__ __forceinline__ FilterLane stage(const HybridDev& hd, int r, Value&& value) {
      const FilterLane me = filter_lane(hd, r);
      const int W = (int)hd.W, H = (int)hd.H, hw = kFilterTileW + 2 * r, hh = kFilterTileH + 2 * r;  // rows of hw records
      for (int i = (int)threadIdx.x; i < hw * hh; i += kBlock) {
         const int gx = me.x0 - r + i % hw, gy = me.y0 - r + i / hw;
         bool ok = false;
         if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            const float4 P4 = hd.pos[g];
            V3 nn;
            ok = P4.w != 0.0f && rtao_normal(hd.nrm[g], nn);
            if (ok) {
               rec[0][i] = P4.x, rec[1][i] = P4.y, rec[2][i] = P4.z;
               rec[3][i] = nn.x, rec[4][i] = nn.y, rec[5][i] = nn.z;
               value(g, i);
            }
         }
         valid[i] = ok ? 1 : 0;
      }
      __syncthreads();
      return me;
   }

   // tap(i) for every record i that counts around a valid centre, (dx, dy) in [-r, r)^2 or - kClosed - [-r, r]^2; returns their number
   template <bool kClosed, typename Tap>
   __device__ __forceinline__ uint32_t taps(int centre, int r, float normal_cos, float plane, Tap&& tap) const {
      const int hw = kFilterTileW + 2 * r, end = kClosed ? r + 1 : r;
      const V3 P = v3(rec[0][centre], rec[1][centre], rec[2][centre]), nn = v3(rec[3][centre], rec[4][centre], rec[5][centre]);
      uint32_t n = 0;
      for (int dy = -r; dy < end; dy++) {
         for (int dx = -r; dx < end; dx++) {
            const int i = centre + dy * hw + dx;
            bool counts = dx == 0 && dy == 0;
            if (!counts && valid[i]) {
               const V3 Pt = v3(rec[0][i], rec[1][i], rec[2][i]), nt = v3(rec[3][i], rec[4][i], rec[5][i]);
               counts = dot3(nt, nn) >= normal_cos && fabsf(dot3(Pt - P, nn)) <= plane;
            }
            if (counts) {
               tap(i);
               n++;
            }
         }
      }
      return n;
   }

   // The same two for a filter with a validity rule of its own and a radius per lane (k_glossy_filter). stage: casts(g) says whether
   // pixel g (in the frame) can be a tap - the caller's rule, which implies a position w != 0 and a finite Nn wherever the P and Nn planes
   // are read (taps); a filter that reads its value planes alone (taps_depth) may admit any pixel.
   template <typename Casts, typename Value>
   __device__ __forceinline__ FilterLane stage(const HybridDev& hd, int r, Casts&& casts, Value&& value) {
      const FilterLane me = filter_lane(hd, r);
      const int W = (int)hd.W, H = (int)hd.H, hw = kFilterTileW + 2 * r, hh = kFilterTileH + 2 * r;
      for (int i = (int)threadIdx.x; i < hw * hh; i += kBlock) {
         const int gx = me.x0 - r + i % hw, gy = me.y0 - r + i / hw;
         bool ok = false;
         if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            ok = casts(g);
            if (ok) {
               const float4 P4 = hd.pos[g];
               V3 nn;
               rtao_normal(hd.nrm[g], nn);
               rec[0][i] = P4.x, rec[1][i] = P4.y, rec[2][i] = P4.z;
               rec[3][i] = nn.x, rec[4][i] = nn.y, rec[5][i] = nn.z;
               value(g, i);
            }
         }
         valid[i] = ok ? 1 : 0;
      }
      __syncthreads();
      return me;
   }
   // taps: the tile was staged for radius r, the lane's own radius is re <= r: (dx, dy) in [-re, re]^2; a tap other than the centre
   // also needs accept(i, max(|dx|, |dy|))
   template <typename Accept, typename Tap>
   __device__ __forceinline__ uint32_t taps(int centre, int r, int re, float normal_cos, float plane, Accept&& accept, Tap&& tap) const {
      const int hw = kFilterTileW + 2 * r;
      const V3 P = v3(rec[0][centre], rec[1][centre], rec[2][centre]), nn = v3(rec[3][centre], rec[4][centre], rec[5][centre]);
      uint32_t n = 0;
      for (int dy = -re; dy <= re; dy++) {
         for (int dx = -re; dx <= re; dx++) {
            const int i = centre + dy * hw + dx;
            bool counts = dx == 0 && dy == 0;
            if (!counts && valid[i] && accept(i, max(abs(dx), abs(dy)))) {
               const V3 Pt = v3(rec[0][i], rec[1][i], rec[2][i]), nt = v3(rec[3][i], rec[4][i], rec[5][i]);
               counts = dot3(nt, nn) >= normal_cos && fabsf(dot3(Pt - P, nn)) <= plane;
            }
            if (counts) {
               tap(i);
               n++;
            }
         }
      }
      return n;
   }
   // taps of a filter whose edge stop is a depth alone (k_fog_resolve: its records are staged by the stage above with a rule that admits
   // sky pixels, whose P and Nn planes are then not read): (dx, dy) in [-r, r]^2; a tap other than the centre needs a valid record and
   // |depth[i] - depth[centre]| <= rel * depth[centre], `depth` being one of the value planes
   template <typename Tap>
   __device__ __forceinline__ uint32_t taps_depth(int centre, int r, const float* depth, float rel, Tap&& tap) const {
      const int hw = kFilterTileW + 2 * r;
      const float D = depth[centre], bound = rel * D;
      uint32_t n = 0;
      for (int dy = -r; dy <= r; dy++) {
         for (int dx = -r; dx <= r; dx++) {
            const int i = centre + dy * hw + dx;
            if ((dx == 0 && dy == 0) || (valid[i] && fabsf(depth[i] - D) <= bound)) {
               tap(i);
               n++;
            }
         }
      }
      return n;
   }
};

}  // namespace uh
