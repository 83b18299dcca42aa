// texture_layout.h - how a texture's texels lie in device memory, as host + device functions: uh_add_texture_rgba8 (context.hip)
// repacks with them, sample_texture_pre (device_math.h) addresses with them, and tests/cpp/texture_layout_check.cpp runs THE SAME
// EXPRESSIONS on the host over every footprint of a set of sizes. Nothing here touches the GPU or the HIP runtime.
//
// Overlapped blocks. A bilinear fetch reads the 2 x 2 texels (x0, y0) .. (x1, y1), and with mirrored repeat x1 - x0 and y1 - y0 are
// -1, 0 or +1. A gather from a table far larger than the L2 pays per distinct 128-byte line it touches (profiles/README.md), and a
// footprint that straddles two tiles of a partition touches two or four. So the blocks here OVERLAP by one texel column and one
// texel row: blocks of W x H texels, one block per cache line (or sector), with origins every W - 1 by H - 1 texels. Block (bx, by)
// stores the source texel (min(bx (W-1) + i, w-1), min(by (H-1) + j, h-1)) at (i, j): whatever texel (mx, my) = (min(x0, x1),
// min(y0, y1)) a footprint starts at, the block (mx / (W-1), my / (H-1)) holds it at a column of at most W - 2 and a row of at most
// H - 2, and so holds all four texels. Texels past the texture's edge are clamped fill; no footprint selects them (at the edge
// x0 == x1, and both read the column of mx). The price is memory: W H / ((W-1) (H-1)) times the texels.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "utopian_hip.h"

#if defined(__HIPCC__)
#define UH_HD __host__ __device__
#else
#define UH_HD
#endif

// The geometry the library is built with. 8 x 4 texels of 4 bytes: one 128-byte line; 4 x 4: one 64-byte sector (measured against
// each other in profiles/README.md "Texture blocks that overlap").
#ifndef UH_TEX_BLOCK_W
#define UH_TEX_BLOCK_W 8
#define UH_TEX_BLOCK_H 4
#endif
constexpr uint32_t kTexBlockW = UH_TEX_BLOCK_W, kTexBlockH = UH_TEX_BLOCK_H;

namespace uh {

// utopian/src/texture.rs:85-98 MIRRORED_REPEAT: the texel index in [0, n) of any integer coordinate
UH_HD inline int mirror_index(int i, int n) {
   int period = 2 * n;
   int m = i % period;
   if (m < 0) m += period;
   return m < n ? m : period - 1 - m;
}

template <uint32_t W, uint32_t H>
struct TexBlocks {
   static_assert(W >= 2 && H >= 2, "a block holds a 2 x 2 footprint");
   static constexpr uint32_t kW = W, kH = H, kTexels = W * H;  // texels of a block; a block's texels are row-major, the blocks are row-major

   // blocks per row / per column of a texture w / h texels wide / high (w, h >= 1): the last origin is at or before the last texel
   static UH_HD size_t blocks_x(size_t w) { return (w - 1) / (W - 1) + 1; }
   static UH_HD size_t blocks_y(size_t h) { return (h - 1) / (H - 1) + 1; }
   // texels the blocked texture takes. UH_ERR_CAPACITY when the sampler's 32-bit texel offset cannot reach all of them (more than 2^32).
   static int texel_count(uint32_t w, uint32_t h, size_t* out) {
      if (!w || !h) return UH_ERR_INVALID_ARGUMENT;
      const size_t blocks = blocks_x(w) * blocks_y(h);  // each factor is below 2^32: no overflow in 64 bits
      if (blocks > (((size_t)1 << 32) / kTexels)) return UH_ERR_CAPACITY;
      *out = blocks * kTexels;
      return UH_OK;
   }
   // texel offset of column `col`, row `row` of block (bx, by); blocks_per_row = blocks_x(w)
   static UH_HD uint32_t texel_offset(uint32_t blocks_per_row, uint32_t bx, uint32_t by, uint32_t col, uint32_t row) {
      return (by * blocks_per_row + bx) * kTexels + row * W + col;
   }
   // texel offset of the footprint that starts at texel (mx, my) = (min(x0, x1), min(y0, y1)): its four texels are at this offset and
   // at + 1, + W, + W + 1 (one block, column <= W - 2, row <= H - 2). The divisions are by constants.
   static UH_HD uint32_t footprint_offset(uint32_t blocks_per_row, uint32_t mx, uint32_t my) {
      const uint32_t bx = mx / (W - 1), by = my / (H - 1);
      return texel_offset(blocks_per_row, bx, by, mx - bx * (W - 1), my - by * (H - 1));
   }
   // row-major RGBA8 (w x h texels) -> blocks; `out` holds 4 * texel_count(w, h) bytes
   static void repack(const uint8_t* rgba, uint32_t w, uint32_t h, uint8_t* out) {
      const size_t nbx = blocks_x(w), nby = blocks_y(h);
      for (size_t by = 0; by < nby; by++)
         for (size_t bx = 0; bx < nbx; bx++) {
            uint8_t* block = out + (by * nbx + bx) * kTexels * 4;
            for (size_t j = 0; j < H; j++) {
               const size_t y = by * (H - 1) + j < h ? by * (H - 1) + j : (size_t)h - 1;
               for (size_t i = 0; i < W; i++) {
                  const size_t x = bx * (W - 1) + i < w ? bx * (W - 1) + i : (size_t)w - 1;
                  memcpy(block + (j * W + i) * 4, rgba + (y * w + x) * 4, 4);
               }
            }
         }
   }
};

using TexLayout = TexBlocks<kTexBlockW, kTexBlockH>;

}  // namespace uh
