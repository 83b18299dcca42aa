// post_levels.h - the bloom pyramid's level sizes (UH_HYBRID_POST; utopian_hip.h "HDR display chain"): level 0 is the frame, level k is
// (ceil(w / 2), ceil(h / 2)) of level k - 1, and a level exists while the one above it is larger than 1 x 1. Plain host C++ without a
// HIP dependency: uh_post_level_size, the pyramid's allocation and tests/cpp/post_levels_check.cpp all go through these.
#pragma once
#include <cstddef>
#include <cstdint>

namespace uh {

constexpr uint32_t kPostMaxLevels = 8;  // UhPostParams::bloom_levels is 1..8

// the size of `level` (0: the frame) of a W x H frame; false for an empty frame, a level above kPostMaxLevels or one that does not exist
inline bool post_level_dims(uint32_t W, uint32_t H, uint32_t level, uint32_t* w, uint32_t* h) {
   if (W == 0 || H == 0 || level > kPostMaxLevels) return false;
   uint32_t lw = W, lh = H;
   for (uint32_t k = 0; k < level; k++) {
      if (lw == 1 && lh == 1) return false;
      lw = lw / 2 + (lw & 1u), lh = lh / 2 + (lh & 1u);  // (no w + 1: W may be 2^32 - 1)
   }
   *w = lw, *h = lh;
   return true;
}

// the levels 1..min(bloom_levels, kPostMaxLevels) that exist for a W x H frame (0 for a 1 x 1 frame)
inline uint32_t post_level_count(uint32_t W, uint32_t H, uint32_t bloom_levels) {
   uint32_t n = 0, w, h;
   while (n < bloom_levels && n < kPostMaxLevels && post_level_dims(W, H, n + 1, &w, &h)) n++;
   return n;
}

// the texels of `level`, 0 when it does not exist
inline size_t post_level_texels(uint32_t W, uint32_t H, uint32_t level) {
   uint32_t w, h;
   return post_level_dims(W, H, level, &w, &h) ? (size_t)w * h : 0;
}

}  // namespace uh
