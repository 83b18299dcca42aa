// post_levels_check.cpp - csrc/post_levels.h (product code: the bloom pyramid's level sizes, behind uh_post_level_size and the pyramid's
// allocation) as a stand-alone host program, meant for -fsanitize=address,undefined: every level's image is allocated at the size the
// header gives and written and read by the index arithmetic of the down and up filters (clamped taps), so that a size that is off by
// one is an out-of-bounds access, at the hybrid size list, at degenerate frames and at the largest width a uint32_t holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "post_levels.h"

using namespace uh;

static int failures = 0;
#define CHECK(cond)                                                   \
   do {                                                               \
      if (!(cond)) {                                                  \
         std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
         failures++;                                                  \
      }                                                               \
   } while (0)

static int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the pyramid of a W x H frame as the library allocates it, walked as the kernels index it
static void walk(uint32_t W, uint32_t H) {
   std::vector<std::vector<float>> level(kPostMaxLevels + 1);
   uint32_t w[kPostMaxLevels + 1] = {}, h[kPostMaxLevels + 1] = {};
   const uint32_t n = post_level_count(W, H, kPostMaxLevels);
   for (uint32_t k = 0; k <= n; k++) {
      CHECK(post_level_dims(W, H, k, &w[k], &h[k]));
      CHECK(post_level_texels(W, H, k) == (size_t)w[k] * h[k]);
      level[k].assign((size_t)w[k] * h[k], 1.0f);
      if (k) CHECK(w[k] == (w[k - 1] + 1) / 2 && h[k] == (h[k - 1] + 1) / 2);
   }
   if (n < kPostMaxLevels) {
      uint32_t a = 7, b = 7;
      CHECK(!post_level_dims(W, H, n + 1, &a, &b) && a == 7 && b == 7);
      CHECK(post_level_texels(W, H, n + 1) == 0);
      CHECK(w[n] == 1 && h[n] == 1);
   }
   for (uint32_t k = 1; k <= n; k++)  // down: 16 clamped taps of the level above; a constant stays a constant
      for (uint32_t Y = 0; Y < h[k]; Y++)
         for (uint32_t X = 0; X < w[k]; X++) {
            float acc = 0.0f;
            for (int j = 0; j < 4; j++)
               for (int i = 0; i < 4; i++) {
                  const int sx = clampi(2 * (int)X - 1 + i, (int)w[k - 1] - 1), sy = clampi(2 * (int)Y - 1 + j, (int)h[k - 1] - 1);
                  acc = acc + (float)(((i == 0 || i == 3) ? 1 : 3) * ((j == 0 || j == 3) ? 1 : 3)) * 0.015625f * level[k - 1][(size_t)sy * w[k - 1] + sx];
               }
            level[k][(size_t)Y * w[k] + X] = acc;
            CHECK(acc == 1.0f);
         }
   for (uint32_t k = n; k-- > 0;)  // up: 4 clamped taps of the level below
      for (uint32_t y = 0; y < h[k]; y++)
         for (uint32_t x = 0; x < w[k]; x++) {
            const int x0 = clampi((x & 1) ? (int)((x - 1) / 2) : (int)(x / 2) - 1, (int)w[k + 1] - 1), x1 = clampi((x & 1) ? (int)((x + 1) / 2) : (int)(x / 2), (int)w[k + 1] - 1);
            const int y0 = clampi((y & 1) ? (int)((y - 1) / 2) : (int)(y / 2) - 1, (int)h[k + 1] - 1), y1 = clampi((y & 1) ? (int)((y + 1) / 2) : (int)(y / 2), (int)h[k + 1] - 1);
            const std::vector<float>& s = level[k + 1];
            const size_t sw = w[k + 1];
            CHECK(0.0625f * s[y0 * sw + x0] + 0.1875f * s[y0 * sw + x1] + 0.1875f * s[y1 * sw + x0] + 0.5625f * s[y1 * sw + x1] == 1.0f);
         }
}

int main() {
   const uint32_t sizes[][2] = {{1, 1}, {1, 45}, {67, 1}, {65, 3}, {257, 3}, {97, 61}, {2, 2}, {3, 3}, {64, 64}, {255, 257}, {1920, 1080}};
   for (const auto& s : sizes) walk(s[0], s[1]);
   uint32_t w = 0, h = 0;
   CHECK(post_level_count(1, 1, 8) == 0 && post_level_count(97, 61, 8) == 7 && post_level_count(97, 61, 3) == 3 && post_level_count(1920, 1080, 6) == 6);
   CHECK(post_level_count(1920, 1080, 100) == 8);
   CHECK(post_level_dims(1920, 1080, 8, &w, &h) && w == 8 && h == 5);
   CHECK(!post_level_dims(1920, 1080, 9, &w, &h) && !post_level_dims(0, 5, 0, &w, &h) && !post_level_dims(5, 0, 1, &w, &h));
   CHECK(!post_level_dims(4, 4, 0xffffffffu, &w, &h));
   // the widest frame: no overflow in the halving
   CHECK(post_level_dims(0xffffffffu, 1, 1, &w, &h) && w == 0x80000000u && h == 1);
   CHECK(post_level_dims(0xffffffffu, 0xffffffffu, 8, &w, &h) && w == (1u << 24) && h == (1u << 24));
   CHECK(post_level_texels(0xffffffffu, 0xffffffffu, 1) == (size_t)0x80000000u * 0x80000000u);
   if (failures) {
      std::printf("%d FAILURES\n", failures);
      return 1;
   }
   std::printf("POST LEVELS CHECK OK\n");
   return 0;
}
