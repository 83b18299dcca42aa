// node_quant.h - the quantisation of a BVH4 node's child boxes (bvh.h Node4C), as host + device functions shared by the host
// builder (bvh_build.cpp) and the on-device refit (refit.hip, which the device builders end in), so that both write the same nodes
// bit for bit.
//
// Every node has a FRAME of its own, chosen from its children: origin = their lowest planes (rounded down), and per axis a
// power-of-two step, the smallest whose 255 steps cover them. The children's planes are stored as 8-bit multiples of the step,
// rounded outwards (lower planes down, upper planes up, in double), so the slab test stays conservative.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UH_HD __host__ __device__
#else
#ifndef UH_HD
#define UH_HD
#endif
#endif

namespace uh {

// biased exponent byte of a power-of-two step -> the step
UH_HD inline double qn_step(uint32_t exps, int axis) { return ldexp(1.0, (int)((exps >> (8 * axis)) & 0xffu) - 127); }

// the frame of a node: origin = the lowest lower plane (rounded down), step = the smallest power of two
// whose 255 steps cover the extent. lo / hi: the children's padded boxes, [child][axis].
UH_HD inline void qn_own_frame(const float lo[4][3], const float hi[4][3], uint32_t n_child, float origin[3], uint32_t& exps) {
   exps = 0;
   for (int a = 0; a < 3; a++) {
      double mn = INFINITY, mx = -INFINITY;
      for (uint32_t k = 0; k < n_child; k++) {
         mn = fmin(mn, (double)lo[k][a]);
         mx = fmax(mx, (double)hi[k][a]);
      }
      if (!(mn <= mx)) mn = mx = 0.0;
      float org = (float)mn;
      if ((double)org > mn) org = nextafterf(org, -INFINITY);
      const double ext = mx - (double)org;
      int e = -100;
      if (!(ext < 1e38)) {
         e = 120;  // non-finite or overflowing extent (only from non-finite world-space geometry): no search
      } else if (ext > 0) {
         int x;
         const double mant = frexp(ext / 255.0, &x);  // ext / 255 = mant * 2^x, mant in [0.5, 1)
         e = (mant == 0.5) ? x - 1 : x;
         while (ldexp(255.0, e) < ext) e++;
         if (e < -100) e = -100;
      }
      origin[a] = org;
      exps |= (uint32_t)(e + 127) << (8 * a);
   }
}

// One node: its children's padded boxes (slots [0, n_child); the rest are empty) against its frame.
// Out: the six plane words (child slot k in byte k; an empty slot is the inverted box 255 / 0).
UH_HD inline void qn_quantise(const float origin[3], uint32_t exps, const float lo[4][3], const float hi[4][3], uint32_t n_child, uint32_t qlo_w[3], uint32_t qhi_w[3]) {
   uint32_t ql[4][3], qh[4][3];
   for (uint32_t k = 0; k < 4; k++)
      for (int a = 0; a < 3; a++) {
         if (k >= n_child) {
            ql[k][a] = 255u;
            qh[k][a] = 0u;
            continue;
         }
         const double s = qn_step(exps, a);
         double a0 = floor(((double)lo[k][a] - (double)origin[a]) / s);
         double a1 = ceil(((double)hi[k][a] - (double)origin[a]) / s);
         if (!(a0 >= 0)) a0 = 0;  // (also NaN)
         if (!(a1 <= 255)) a1 = 255;
         if (a0 > 255) a0 = 255;
         if (!(a1 >= 0)) a1 = 0;
         ql[k][a] = (uint32_t)a0;
         qh[k][a] = (uint32_t)a1;
      }
   for (int a = 0; a < 3; a++) {
      qlo_w[a] = qhi_w[a] = 0;
      for (uint32_t k = 0; k < 4; k++) {
         qlo_w[a] |= ql[k][a] << (8 * k);
         qhi_w[a] |= qh[k][a] << (8 * k);
      }
   }
}

}  // namespace uh
