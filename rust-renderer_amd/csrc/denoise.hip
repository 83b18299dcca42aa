// denoise.hip - the kernels of uh_denoise (include/utopian_hip.h "the denoiser"): input + temporal accumulation, the short-history
// variance estimate, the a-trous levels and the output. Arithmetic: DESIGN.md section 2, "Denoiser: the arithmetic contract of
// uh_denoise"; tests/denoise_reference.py restates it.
// Layout: a block is 4 rows of 64 pixels, one row per wave, so that for a fixed tap offset a wave's 64 lanes read 64 consecutive texels
// - every tap load of a float4 image is one coalesced 1 KB request. The taps of neighbouring pixels overlap and are served by the caches
// (the plain form; no LDS tile).
#include <hip/hip_runtime.h>

#include "denoise_device.h"
#include "kernel_common.h"

namespace uh {

constexpr uint32_t kDnRow = 64, kDnRows = 4;

static inline dim3 dn_grid(const DenoiseDev& d) { return dim3((d.W + kDnRow - 1) / kDnRow, (d.H + kDnRows - 1) / kDnRows); }
static inline dim3 dn_block() { return dim3(kDnRow, kDnRows); }

// d of stage 0: max(albedo / 255, 0.01) per channel on geometry with UH_DENOISE_DEMODULATE, else 1
__device__ __forceinline__ V3 dn_demodulator(const DenoiseDev& d, size_t i) {
   if (!d.demodulate) return v3(1.0f, 1.0f, 1.0f);
   const uchar4 a = d.g_alb[i];
   return v3(fmaxf(d.unorm_lut[a.x], 0.01f), fmaxf(d.unorm_lut[a.y], 0.01f), fmaxf(d.unorm_lut[a.z], 0.01f));
}

// ---- stages 0 and 1: the input, the reprojected history, the temporal colour and moments ----
// kMotion (UH_DENOISE_MOTION): the point that is reprojected and held against the history's plane is the motion texel's xyz - where the
// pixel's surface point was at the previous motion pass - instead of p; a texel with w == 0 has no correspondence and keeps no history.
// Without it the instantiation is the stage as it always was.
// A geometry pixel whose stage-0 colour fails temporal_sample_ok is written as if it were not geometry, cur.pos with w = 0 included: the
// later stages, the output's remodulation and the next call's history taps all skip it through that w. It still counts as geometry.
template <bool kMotion>
__global__ __launch_bounds__(256) void k_denoise_temporal(DenoiseDev d) {
   const uint32_t x = blockIdx.x * kDnRow + threadIdx.x, y = blockIdx.y * kDnRows + threadIdx.y;
   bool geo = false, kept = false;
   if (x < d.W && y < d.H) {
      const size_t i = (size_t)y * d.W + x;
      const float4 a = d.acc[i];
      float r = a.x / d.n, g = a.y / d.n, b = a.z / d.n;
      const float4 P4 = d.g_pos[i];
      geo = P4.w != 0.0f;
      const bool live = geo && temporal_sample_ok(r, g, b);
      d.cur.pos[i] = live ? P4 : make_float4(P4.x, P4.y, P4.z, 0.0f);
      if (!live) {
         const float4 c = make_float4(r, g, b, 0.0f);
         d.input[i] = c;
         d.cv[0][i] = c;
         d.temporal[i] = c;
         d.history[i] = 0.0f;
      } else {
         const V3 dm = dn_demodulator(d, i);
         if (d.demodulate) r = r / dm.x, g = g / dm.y, b = b / dm.z;
         d.input[i] = make_float4(r, g, b, 0.0f);
         const float l = dn_luminance(r, g, b), l2 = l * l;
         const V3 p = xyz(P4), n = xyz(d.g_nrm[i]);
         const float mesh = d.g_pbr[i].w;
         float cr = r, cg = g, cb = b, m1 = l, m2 = l2, N = 1.0f;
         V3 pp = p;
         bool corresponds = true;
         if (kMotion) {
            const float4 mv = d.motion[i];
            pp = xyz(mv);
            corresponds = mv.w != 0.0f;
         }
         if (d.temporal_on && corresponds) {
            const float4 h = mat4_mul(d.prev_pv, pp.x, pp.y, pp.z, 1.0f);
            const float u = (h.x / h.w) * 0.5f + 0.5f, v = 1.0f - ((h.y / h.w) * 0.5f + 0.5f);
            const float fx = u * (float)d.W - 0.5f, fy = v * (float)d.H - 0.5f;
            if (h.w > 0.0f && isfinite(fx) && isfinite(fy)) {
               const float ix = floorf(fx), iy = floorf(fy);
               const float ax = rintf((fx - ix) * 256.0f) / 256.0f, ay = rintf((fy - iy) * 256.0f) / 256.0f;
               const float tol = d.reproject_plane * fabsf(dn_view_z(d.view, p));
               float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, s1 = 0.0f, s2 = 0.0f;
               for (int t = 0; t < 4; t++) {
                  const int dx = t & 1, dy = t >> 1;
                  const float w = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
                  if (w == 0.0f) continue;
                  const float tx = ix + (float)dx, ty = iy + (float)dy;
                  if (!(tx >= 0.0f && tx <= (float)(d.W - 1) && ty >= 0.0f && ty <= (float)(d.H - 1))) continue;
                  const size_t j = (size_t)(uint32_t)ty * d.W + (uint32_t)tx;
                  const float4 q = d.prev.pos[j];
                  if (q.w == 0.0f) continue;
                  const float4 qn = d.prev.nrm[j];
                  if (!(qn.w == mesh)) continue;
                  if (!(dot3(n, xyz(qn)) >= d.reproject_normal_cos)) continue;
                  if (!(fabsf(dot3(xyz(q) - pp, n)) <= tol)) continue;
                  const float4 qc = d.prev.col[j];
                  const float2 qm = d.prev.mom[j];
                  sw = sw + w;
                  sr = sr + w * qc.x, sg = sg + w * qc.y, sb = sb + w * qc.z, sn = sn + w * qc.w;
                  s1 = s1 + w * qm.x, s2 = s2 + w * qm.y;
               }
               if (sw > 0.0f) {
                  kept = true;
                  N = fminf(sn / sw + 1.0f, d.max_history);
                  const float al = fmaxf(1.0f / N, d.alpha_min);
                  const float pr = sr / sw, pg = sg / sw, pb = sb / sw, p1 = s1 / sw, p2 = s2 / sw;
                  cr = pr + (r - pr) * al, cg = pg + (g - pg) * al, cb = pb + (b - pb) * al;
                  m1 = p1 + (l - p1) * al, m2 = p2 + (l2 - p2) * al;
               }
            }
         }
         const float var = fmaxf(m2 - m1 * m1, 0.0f);
         d.cur.nrm[i] = make_float4(n.x, n.y, n.z, mesh);
         d.cur.col[i] = make_float4(cr, cg, cb, N);
         d.cur.mom[i] = make_float2(m1, m2);
         d.cv[0][i] = make_float4(cr, cg, cb, var);
         d.temporal[i] = make_float4(cr * dm.x, cg * dm.y, cb * dm.z, 0.0f);
         d.history[i] = N;
      }
   }
   // the two counters: one atomic per wave and counter
   const unsigned long long bg = __ballot(geo), bk = __ballot(kept);
   if (threadIdx.x == 0) {
      if (bg) atomicAdd(&d.counters[0], (uint32_t)__popcll(bg));
      if (bk) atomicAdd(&d.counters[1], (uint32_t)__popcll(bk));
   }
}

// ---- stage 2: where the history is shorter than 4 frames, the variance from the 7 x 7 neighbourhood's moments ----
__global__ __launch_bounds__(256) void k_denoise_variance(DenoiseDev d) {
   const uint32_t x = blockIdx.x * kDnRow + threadIdx.x, y = blockIdx.y * kDnRows + threadIdx.y;
   if (x >= d.W || y >= d.H) return;
   const size_t i = (size_t)y * d.W + x;
   const float4 P4 = d.cur.pos[i];
   if (P4.w == 0.0f) {
      d.variance[i] = 0.0f;
      return;
   }
   const float N = d.cur.col[i].w;
   float var = d.cv[0][i].w;
   if (N < 4.0f) {
      const V3 p = xyz(P4), n = xyz(d.cur.nrm[i]);
      const float den = d.sigma_plane * fabsf(dn_view_z(d.view, p)) + 1e-6f;
      float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
      for (int dy = -3; dy <= 3; dy++) {
         for (int dx = -3; dx <= 3; dx++) {
            float4 Q4;
            const int qx = (int)x + dx, qy = (int)y + dy;
            if (!dn_geometry(d.cur.pos, d.W, d.H, qx, qy, Q4)) continue;
            const size_t j = (size_t)qy * d.W + qx;
            const float w = dn_normal_weight(n, xyz(d.cur.nrm[j])) * expf(-dn_plane_term(p, n, xyz(Q4), den));
            const float2 m = d.cur.mom[j];
            sw = sw + w;
            s1 = s1 + w * m.x, s2 = s2 + w * m.y;
         }
      }
      if (sw > 0.0f) {
         const float m1 = s1 / sw, m2 = s2 / sw;
         var = fmaxf(m2 - m1 * m1, 0.0f) * (4.0f / N);
      }
      d.cv[0][i].w = var;
   }
   d.variance[i] = var;
}

// ---- stage 3: one a-trous level, 5 x 5 taps at p + step * (dx, dy) ----
__global__ __launch_bounds__(256) void k_denoise_atrous(DenoiseDev d, const float4* __restrict__ in, float4* __restrict__ out, int step) {
   const uint32_t x = blockIdx.x * kDnRow + threadIdx.x, y = blockIdx.y * kDnRows + threadIdx.y;
   if (x >= d.W || y >= d.H) return;
   const size_t i = (size_t)y * d.W + x;
   const float4 P4 = d.cur.pos[i];
   const float4 cp = in[i];
   if (P4.w == 0.0f) {
      out[i] = cp;
      return;
   }
   const V3 p = xyz(P4), n = xyz(d.cur.nrm[i]);
   const float lp = dn_luminance(cp.x, cp.y, cp.z);
   const float plane_den = d.sigma_plane * fabsf(dn_view_z(d.view, p)) + 1e-6f;
   // g: the 3 x 3 Gaussian of the level's variance over the adjacent geometry pixels, renormalised
   float sg = 0.0f, sk = 0.0f;
   for (int dy = -1; dy <= 1; dy++) {
      for (int dx = -1; dx <= 1; dx++) {
         float4 Q4;
         const int qx = (int)x + dx, qy = (int)y + dy;
         if (!dn_geometry(d.cur.pos, d.W, d.H, qx, qy, Q4)) continue;
         const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
         sg = sg + k * in[(size_t)qy * d.W + qx].w;
         sk = sk + k;
      }
   }
   const float lum_den = d.sigma_luminance * sqrtf(sg / sk) + 1e-6f;
   // the centre tap: w = 9/64
   float sw = 0.140625f, sr = 0.140625f * cp.x, sgr = 0.140625f * cp.y, sb = 0.140625f * cp.z, sv = (0.140625f * 0.140625f) * cp.w;
   for (int dy = -2; dy <= 2; dy++) {
      for (int dx = -2; dx <= 2; dx++) {
         if (dx == 0 && dy == 0) continue;
         float4 Q4;
         const int qx = (int)x + step * dx, qy = (int)y + step * dy;
         if (!dn_geometry(d.cur.pos, d.W, d.H, qx, qy, Q4)) continue;
         const size_t j = (size_t)qy * d.W + qx;
         const float4 cq = in[j];
         const float k = dn_kernel(dx) * dn_kernel(dy);
         const float wn = dn_normal_weight(n, xyz(d.cur.nrm[j]));
         const float ep = dn_plane_term(p, n, xyz(Q4), plane_den);
         const float el = fabsf(lp - dn_luminance(cq.x, cq.y, cq.z)) / lum_den;
         const float w = (k * wn) * expf(-(ep + el));
         sw = sw + w;
         sr = sr + w * cq.x, sgr = sgr + w * cq.y, sb = sb + w * cq.z;
         sv = sv + (w * w) * cq.w;
      }
   }
   out[i] = make_float4(sr / sw, sgr / sw, sb / sw, sv / (sw * sw));
}

// ---- stage 4: remodulate; the 8-bit image through the path tracer's resolve (denominator 1) ----
__global__ __launch_bounds__(256) void k_denoise_output(DenoiseDev d, const float4* __restrict__ in) {
   const uint32_t x = blockIdx.x * kDnRow + threadIdx.x, y = blockIdx.y * kDnRows + threadIdx.y;
   if (x >= d.W || y >= d.H) return;
   const size_t i = (size_t)y * d.W + x;
   float4 c = in[i];
   if (d.cur.pos[i].w != 0.0f) {
      const V3 dm = dn_demodulator(d, i);
      c.x = c.x * dm.x, c.y = c.y * dm.y, c.z = c.z * dm.z;
   }
   c.w = 0.0f;
   d.color[i] = c;
   d.output[i] = resolve_color(c, 1u, 1u);
}

void launch_denoise_temporal(const LaunchCfg& c, const DenoiseDev& d) {
   if (d.motion)
      k_denoise_temporal<true><<<dn_grid(d), dn_block(), 0, c.stream>>>(d);
   else
      k_denoise_temporal<false><<<dn_grid(d), dn_block(), 0, c.stream>>>(d);
}
void launch_denoise_variance(const LaunchCfg& c, const DenoiseDev& d) { k_denoise_variance<<<dn_grid(d), dn_block(), 0, c.stream>>>(d); }
void launch_denoise_atrous(const LaunchCfg& c, const DenoiseDev& d, uint32_t level) {
   k_denoise_atrous<<<dn_grid(d), dn_block(), 0, c.stream>>>(d, d.cv[level & 1], d.cv[(level & 1) ^ 1], 1 << level);
}
void launch_denoise_output(const LaunchCfg& c, const DenoiseDev& d, uint32_t from) { k_denoise_output<<<dn_grid(d), dn_block(), 0, c.stream>>>(d, d.cv[from]); }

}  // namespace uh
