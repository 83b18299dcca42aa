// texture_layout_check - csrc/texture_layout.h (product code: the host repack of uh_add_texture_rgba8 and the address function of
// sample_texture_pre) on the host, meant to be built with -fsanitize=address,undefined. For a set of sizes and for both block
// geometries (8 x 4 texels: one 128-byte line; 4 x 4: one 64-byte sector), over every integer footprint corner (fx, fy) in
// [-3w, 3w) x [-3h, 3h): the sampler's four texels - footprint_offset of the minima, + 1, + W, + W + 1, picked as the device picks
// them - are the row-major source's texels (x0, y0), (x1, y0), (x0, y1), (x1, y1) under mirror_index; all four offsets stay inside
// the allocation texel_count gives; they lie in one block. Sizes whose blocked texel count exceeds 2^32 are refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "texture_layout.h"

namespace {
int failures = 0;
void fail(const char* what, unsigned bw, unsigned bh, unsigned w, unsigned h, int fx, int fy) {
   if (failures++ < 20) printf("MISMATCH %s: blocks %ux%u, texture %ux%u, footprint (%d, %d)\n", what, bw, bh, w, h, fx, fy);
}

template <uint32_t BW, uint32_t BH>
size_t check_size(uint32_t w, uint32_t h) {
   using L = uh::TexBlocks<BW, BH>;
   // source: no two texels alike (the texel's own index, scrambled so that neighbours differ in every byte)
   std::vector<uint32_t> src((size_t)w * h);
   for (size_t k = 0; k < src.size(); k++) src[k] = (uint32_t)k * 2654435761u + 0x9e3779b9u;
   size_t count = 0;
   if (L::texel_count(w, h, &count) != UH_OK) {
      fail("texel_count refused a small texture", BW, BH, w, h, 0, 0);
      return 0;
   }
   if (count != L::blocks_x(w) * L::blocks_y(h) * L::kTexels) fail("texel_count", BW, BH, w, h, 0, 0);
   // exactly `count` texels on the heap: AddressSanitizer sees a read or a write one texel past either end
   std::vector<uint32_t> packed(count);
   L::repack(reinterpret_cast<const uint8_t*>(src.data()), w, h, reinterpret_cast<uint8_t*>(packed.data()));
   const uint32_t nbx = (uint32_t)L::blocks_x(w);
   size_t footprints = 0;
   for (int fy = -3 * (int)h; fy < 3 * (int)h; fy++)
      for (int fx = -3 * (int)w; fx < 3 * (int)w; fx++) {
         const int x0 = uh::mirror_index(fx, (int)w), x1 = uh::mirror_index(fx + 1, (int)w);
         const int y0 = uh::mirror_index(fy, (int)h), y1 = uh::mirror_index(fy + 1, (int)h);
         if (x1 - x0 < -1 || x1 - x0 > 1 || y1 - y0 < -1 || y1 - y0 > 1) fail("x1 - x0, y1 - y0 in {-1, 0, 1}", BW, BH, w, h, fx, fy);
         const int mx = x0 < x1 ? x0 : x1, my = y0 < y1 ? y0 : y1;
         const size_t at = L::footprint_offset(nbx, (uint32_t)mx, (uint32_t)my);
         if (at + BW + 1 >= count) {  // the last of the four
            fail("address outside the allocation", BW, BH, w, h, fx, fy);
            continue;
         }
         if (at / L::kTexels != (at + BW + 1) / L::kTexels || at % BW > BW - 2 || at % L::kTexels / BW > BH - 2) fail("footprint leaves its block", BW, BH, w, h, fx, fy);
         // the device's selection (device_math.h sample_texture_pre): rows r0, r1 of two texels each
         const uint32_t r0[2] = {packed[at], packed[at + 1]}, r1[2] = {packed[at + BW], packed[at + BW + 1]};
         const uint32_t* ra = y0 != my ? r1 : r0;
         const uint32_t* rb = y1 != my ? r1 : r0;
         const uint32_t w00 = ra[x0 != mx], w10 = ra[x1 != mx], w01 = rb[x0 != mx], w11 = rb[x1 != mx];
         if (w00 != src[(size_t)y0 * w + x0] || w10 != src[(size_t)y0 * w + x1] || w01 != src[(size_t)y1 * w + x0] || w11 != src[(size_t)y1 * w + x1])
            fail("texel", BW, BH, w, h, fx, fy);
         footprints++;
      }
   // every block texel is the clamped source texel the layout promises (the fill included)
   for (size_t by = 0; by < L::blocks_y(h); by++)
      for (size_t bx = 0; bx < nbx; bx++)
         for (uint32_t j = 0; j < BH; j++)
            for (uint32_t i = 0; i < BW; i++) {
               const size_t x = bx * (BW - 1) + i < w ? bx * (BW - 1) + i : w - 1, y = by * (BH - 1) + j < h ? by * (BH - 1) + j : h - 1;
               if (packed[L::texel_offset(nbx, (uint32_t)bx, (uint32_t)by, i, j)] != src[y * w + x]) fail("block texel", BW, BH, w, h, (int)x, (int)y);
            }
   return footprints;
}

template <uint32_t BW, uint32_t BH>
size_t check_geometry() {
   static const uint32_t sizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {7, 3}, {8, 4}, {9, 5}, {15, 22}, {16, 8}, {8, 24}, {64, 64}};  // w, h
   size_t footprints = 0;
   for (const auto& s : sizes) footprints += check_size<BW, BH>(s[0], s[1]);
   using L = uh::TexBlocks<BW, BH>;
   // capacity: 2^32 texels is the most a 32-bit texel offset reaches. 65536 x 65536 source texels are 2^32 already, and more blocked
   size_t count = 12345;
   const struct { uint32_t w, h; bool fits; } cases[] = {
      {65536, 65536, false}, {0xffffffffu, 0xffffffffu, false}, {0xffffffffu, 1, false}, {1, 0xffffffffu, false}, {1u << 27, 1, true}, {1, 1u << 27, true}, {40000, 40000, true}, {60000, 60000, false}};
   for (const auto& c : cases) {
      count = 12345;
      const int st = L::texel_count(c.w, c.h, &count);
      const double blocked = (double)L::blocks_x(c.w) * (double)L::blocks_y(c.h) * L::kTexels;
      if (c.fits != (blocked <= 4294967296.0)) fail("capacity case misjudged by the check itself", BW, BH, c.w, c.h, 0, 0);
      if (c.fits ? (st != UH_OK || (double)count != blocked) : (st != UH_ERR_CAPACITY || count != 12345)) fail("capacity", BW, BH, c.w, c.h, 0, 0);
   }
   if (L::texel_count(0, 4, &count) != UH_ERR_INVALID_ARGUMENT || L::texel_count(4, 0, &count) != UH_ERR_INVALID_ARGUMENT) fail("empty texture", BW, BH, 0, 0, 0, 0);
   return footprints;
}
}  // namespace

int main() {
   const size_t a = check_geometry<8, 4>(), b = check_geometry<4, 4>();
   static_assert(uh::TexLayout::kW == kTexBlockW && uh::TexLayout::kH == kTexBlockH, "the library's geometry");
   static_assert((kTexBlockW == 8 && kTexBlockH == 4) || (kTexBlockW == 4 && kTexBlockH == 4), "the shipped geometry is one of the two checked here");
   printf("footprints checked: %zu (8x4) + %zu (4x4)\n", a, b);
   if (failures) {
      printf("TEXTURE LAYOUT CHECK FAILED: %d\n", failures);
      return 1;
   }
   printf("TEXTURE LAYOUT CHECK OK\n");
   return 0;
}
