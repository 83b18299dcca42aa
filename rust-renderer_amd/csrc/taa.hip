// taa.hip - temporal anti-aliasing of the hybrid frame (UH_HYBRID_TAA; utopian_hip.h): one kernel between the sky pass and present that
// blends deferred_output into a reprojected, clamped history. An extension: the reference's anti-aliasing is present's FXAA.
// Arithmetic: DESIGN.md section 2, "Temporal anti-aliasing: the arithmetic contract of UH_HYBRID_TAA"; tests/taa_reference.py restates it.
// Layout: the denoiser's - a block is 4 rows of 64 pixels, one row per wave, so that for a fixed offset of the 3 x 3 box a wave's 64 lanes
// read 64 consecutive texels, one coalesced 1 KB request. The nine reads of neighbouring pixels overlap and are served by the caches (no
// LDS tile: DESIGN.md section 4, "Temporal anti-aliasing").
#include <hip/hip_runtime.h>

#include "denoise_device.h"
#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"

namespace uh {

constexpr uint32_t kTaaRow = 64, kTaaRows = kBlock / kTaaRow;

// kMotion (UH_TAA_MOTION): a geometry pixel reprojects the motion texel's xyz - where its surface point was at the previous motion pass -
// instead of its position; a texel with w == 0 has no correspondence and starts a new history.
// A pixel whose colour fails temporal_sample_ok passes through with N = 0: the boxes of its neighbours leave it out, and a later call's
// history taps skip a texel whose N is 0 as they skip one outside the frame.
template <bool kMotion>
__global__ __launch_bounds__(kBlock) void k_hybrid_taa(FrameParams fp, TaaDev t) {
   const uint32_t x = blockIdx.x * kTaaRow + threadIdx.x, y = blockIdx.y * kTaaRows + threadIdx.y;
   const uint32_t W = fp.W, H = fp.H;
   bool blended = false, started = false;
   if (x < W && y < H) {
      const size_t i = (size_t)y * W + x;
      const float4 c = t.deferred[i];
      const bool live = temporal_sample_ok(c.x, c.y, c.z);
      // the neighbourhood box: mean and deviation per channel over the 3 x 3 pixels in the frame
      V3 lo = v3(0.0f, 0.0f, 0.0f), hi = lo;
      if (t.clamp && live) {
         V3 s1 = v3(0.0f, 0.0f, 0.0f), s2 = s1;
         float k = 0.0f;
         for (int dy = -1; dy <= 1; dy++) {
            for (int dx = -1; dx <= 1; dx++) {
               const int qx = (int)x + dx, qy = (int)y + dy;
               if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
               const float4 q = t.deferred[(size_t)qy * W + qx];
               if (!temporal_sample_ok(q.x, q.y, q.z)) continue;
               s1.x = s1.x + q.x, s1.y = s1.y + q.y, s1.z = s1.z + q.z;
               s2.x = s2.x + q.x * q.x, s2.y = s2.y + q.y * q.y, s2.z = s2.z + q.z * q.z;
               k = k + 1.0f;
            }
         }
         const V3 m1 = v3(s1.x / k, s1.y / k, s1.z / k), m2 = v3(s2.x / k, s2.y / k, s2.z / k);
         const V3 sg = v3(sqrtf(fmaxf(m2.x - m1.x * m1.x, 0.0f)), sqrtf(fmaxf(m2.y - m1.y * m1.y, 0.0f)), sqrtf(fmaxf(m2.z - m1.z * m1.z, 0.0f)));
         lo = v3(m1.x - t.clamp_gamma * sg.x, m1.y - t.clamp_gamma * sg.y, m1.z - t.clamp_gamma * sg.z);
         hi = v3(m1.x + t.clamp_gamma * sg.x, m1.y + t.clamp_gamma * sg.y, m1.z + t.clamp_gamma * sg.z);
      }
      float r = c.x, g = c.y, b = c.z, N = 1.0f;
      if (!live) N = 0.0f;
      if (t.prev_col && live) {
         // where the history is: a geometry pixel's point, every other pixel's primary-ray direction as a point at infinity
         const float4 P4 = t.pos[i];
         bool corresponds = true;
         float4 h;
         if (P4.w != 0.0f) {
            V3 q = xyz(P4);
            if (kMotion) {
               const float4 mv = t.motion[i];
               q = xyz(mv);
               corresponds = mv.w != 0.0f;
            }
            h = mat4_mul(fp.prev_pv, q.x, q.y, q.z, 1.0f);
         } else {
            V3 o, d;
            primary_ray(fp, x, y, 0.5f, 0.5f, o, d);
            h = mat4_mul(fp.prev_pv, d.x, d.y, d.z, 0.0f);
         }
         if (corresponds) {
            const float u = (h.x / h.w) * 0.5f + 0.5f, v = 1.0f - ((h.y / h.w) * 0.5f + 0.5f);
            const float fx = u * (float)W - 0.5f, fy = v * (float)H - 0.5f;
            if (h.w > 0.0f && isfinite(fx) && isfinite(fy)) {
               const float ix = floorf(fx), iy = floorf(fy);
               const float ax = rintf((fx - ix) * 256.0f) / 256.0f, ay = rintf((fy - iy) * 256.0f) / 256.0f;
               float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
               for (int tap = 0; tap < 4; tap++) {
                  const int dx = tap & 1, dy = tap >> 1;
                  const float w = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
                  if (w == 0.0f) continue;
                  const float tx = ix + (float)dx, ty = iy + (float)dy;
                  if (!(tx >= 0.0f && tx <= (float)(W - 1) && ty >= 0.0f && ty <= (float)(H - 1))) continue;
                  const size_t j = (size_t)(uint32_t)ty * W + (uint32_t)tx;
                  const float4 qc = t.prev_col[j];
                  const float qn = t.prev_n[j];
                  if (qn == 0.0f) continue;
                  sw = sw + w;
                  sr = sr + w * qc.x, sg = sg + w * qc.y, sb = sb + w * qc.z, sn = sn + w * qn;
               }
               if (sw > 0.0f) {
                  blended = true;
                  float hr = sr / sw, hg = sg / sw, hb = sb / sw;
                  N = fminf(sn / sw + 1.0f, t.max_history);
                  const float a = fmaxf(1.0f / N, t.alpha_min);
                  if (t.clamp) hr = fminf(fmaxf(hr, lo.x), hi.x), hg = fminf(fmaxf(hg, lo.y), hi.y), hb = fminf(fmaxf(hb, lo.z), hi.z);
                  r = hr + (c.x - hr) * a, g = hg + (c.y - hg) * a, b = hb + (c.z - hb) * a;
               }
            }
         }
      }
      started = !blended;
      t.col[i] = make_float4(r, g, b, c.w);
      t.n[i] = N;
   }
   // the two counters: one atomic per wave and counter, into the pair of the wave's number modulo the slots - a line of its own per pair,
   // so that the frame's waves do not queue on one address ("Motion vectors", measured what that costs)
   const unsigned long long bb = __ballot(blended), bs = __ballot(started);
   if (threadIdx.x == 0) {
      const uint32_t wave = (blockIdx.y * gridDim.x + blockIdx.x) * kTaaRows + threadIdx.y;
      uint32_t* pair = t.counters + (size_t)(wave % kTaaCounterSlots) * kTaaCounterStride;
      if (bb) atomicAdd(&pair[0], (uint32_t)__popcll(bb));
      if (bs) atomicAdd(&pair[1], (uint32_t)__popcll(bs));
   }
}

void launch_hybrid_taa(const LaunchCfg& c, const FrameParams& fp, const TaaDev& t) {
   const dim3 grid((fp.W + kTaaRow - 1) / kTaaRow, (fp.H + kTaaRows - 1) / kTaaRows), block(kTaaRow, kTaaRows);
   if (t.motion)
      k_hybrid_taa<true><<<grid, block, 0, c.stream>>>(fp, t);
   else
      k_hybrid_taa<false><<<grid, block, 0, c.stream>>>(fp, t);
}

}  // namespace uh
