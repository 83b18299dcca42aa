// tile_partition_check - csrc/tile_partition.h (product code: which rank owns which tile and pixel of a tile-partitioned frame, how
// many pixels a rank's packed buffer holds and which pixel lies at each of its positions) on the host, meant to be built with
// -fsanitize=address,undefined. The header's closed forms are held to the same partition written out a second time in the plainest
// form - tiles dealt to the ranks one by one, pixels painted tile by tile, 64-bit counters, no division - and to each other: every
// pixel has one owner, the ranks' tiles add up, a packed buffer is whole tiles, its in-frame positions are exactly the pixels the
// owner test gives the rank, and those in ascending order are the list uh_set_tile_partition uploads.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tile_partition.h"

namespace {
int failures = 0;
uint64_t checked = 0;
struct Case {
   uint32_t W, H, tile, world;
};
void fail(const char* what, const Case& c, uint64_t rank, uint64_t at) {
   if (failures++ < 20) printf("MISMATCH %s: %u x %u, tile %u, world %u, rank %llu, at %llu\n", what, c.W, c.H, c.tile, c.world, (unsigned long long)rank, (unsigned long long)at);
}

void check(const Case& c) {
   const uint64_t W = c.W, H = c.H, T = c.tile;
   // ---- the partition, plainly: tiles in row-major order go to rank 0, 1, .. world - 1, 0, ..; each paints its pixels
   std::vector<uint64_t> ref_tile_owner, ref_tile_x0, ref_tile_y0, ref_tiles_of(c.world, 0);
   std::vector<int64_t> ref_pixel_owner(W * H, -1);
   uint64_t next = 0, ref_tiles_x = 0;
   for (uint64_t y0 = 0; y0 < H; y0 += T) {
      ref_tiles_x = 0;
      for (uint64_t x0 = 0; x0 < W; x0 += T) {
         ref_tiles_x++;
         ref_tile_owner.push_back(next), ref_tile_x0.push_back(x0), ref_tile_y0.push_back(y0);
         ref_tiles_of[next]++;
         for (uint64_t y = y0; y < y0 + T && y < H; y++)
            for (uint64_t x = x0; x < x0 + T && x < W; x++) {
               if (ref_pixel_owner[y * W + x] != -1) fail("reference paints a pixel twice", c, next, y * W + x);
               ref_pixel_owner[y * W + x] = (int64_t)next;
            }
         if (++next == c.world) next = 0;
      }
   }
   const uint64_t ref_tiles = ref_tile_owner.size();

   // ---- the header against it
   const uint32_t tiles_x = uh::tiles_across(c.W, c.tile);
   if (tiles_x != ref_tiles_x) fail("tiles_across", c, 0, tiles_x);
   if (uh::tile_count(c.W, c.H, c.tile) != ref_tiles) fail("tile_count", c, 0, uh::tile_count(c.W, c.H, c.tile));
   for (uint64_t t = 0; t < ref_tiles; t++)
      if (uh::tile_owner((uint32_t)t, c.world) != ref_tile_owner[t]) fail("tile_owner", c, ref_tile_owner[t], t);
   for (uint32_t y = 0; y < c.H; y++)
      for (uint32_t x = 0; x < c.W; x++) {
         const uint32_t t = uh::tile_of_pixel(x, y, c.tile, tiles_x);
         if (t >= ref_tiles || ref_tile_x0[t] > x || x >= ref_tile_x0[t] + T || ref_tile_y0[t] > y || y >= ref_tile_y0[t] + T) fail("tile_of_pixel", c, 0, y * W + x);
         if ((int64_t)uh::pixel_owner(x, y, c.tile, tiles_x, c.world) != ref_pixel_owner[y * W + x]) fail("pixel_owner", c, 0, y * W + x);
      }
   uint64_t tiles_sum = 0;
   std::vector<uint32_t> hits(W * H, 0);  // times a pixel appears among all ranks' in-frame packed positions
   for (uint32_t r = 0; r < c.world; r++) {
      const uint32_t owned = uh::tiles_owned((uint32_t)ref_tiles, r, c.world);
      if (owned != ref_tiles_of[r]) fail("tiles_owned", c, r, owned);
      if (owned > ref_tiles_of[0]) fail("a rank owns more tiles than rank 0 (max_pack_pixels asks rank 0)", c, r, owned);
      tiles_sum += owned;
      const uint64_t pack = uh::pack_pixels(c.W, c.H, c.tile, r, c.world);
      if (pack != ref_tiles_of[r] * T * T) fail("pack_pixels is owned tiles x tile^2", c, r, pack);
      // the packed buffer, plainly: the rank's tiles in ascending order, each row by row, whole
      uint64_t k = 0;
      std::vector<uint32_t> in_frame(W * H, 0);  // times a pixel appears among this rank's in-frame positions
      for (uint64_t t = 0; t < ref_tiles; t++) {
         if (ref_tile_owner[t] != r) continue;
         for (uint64_t j = 0; j < T; j++)
            for (uint64_t i = 0; i < T; i++, k++) {
               const uint64_t x = ref_tile_x0[t] + i, y = ref_tile_y0[t] + j;
               if (k >= pack) {
                  fail("packed position beyond pack_pixels", c, r, k);
                  continue;
               }
               const uh::PackedPixel p = uh::packed_pixel(k, c.W, c.H, c.tile, tiles_x, r, c.world);
               if (p.x != x || p.y != y || p.inside != (x < W && y < H)) fail("packed_pixel", c, r, k);
               if (!p.inside) continue;
               if (uh::packed_position((uint32_t)t, p.x, p.y, c.tile, c.world) != k) fail("packed_position undoes packed_pixel", c, r, k);
               if (uh::pixel_owner(p.x, p.y, c.tile, tiles_x, c.world) != r) fail("a packed pixel the owner test gives another rank", c, r, k);
               hits[p.y * W + p.x]++;
               in_frame[p.y * W + p.x]++;
            }
      }
      if (k != pack) fail("the rank's tiles fill its packed buffer", c, r, k);
      checked += k;
      // uh_set_tile_partition's list: the frame in ascending pixel order through the owner test; n_owned its length
      std::vector<uint32_t> own;
      for (uint32_t y = 0; y < c.H; y++)
         for (uint32_t x = 0; x < c.W; x++)
            if (uh::pixel_owner(x, y, c.tile, tiles_x, c.world) == r) own.push_back(y * c.W + x);
      uint64_t n = 0;
      for (uint32_t p = 0; p < W * H; p++)  // the in-frame packed pixels in ascending order
         if (in_frame[p] != 0 && (in_frame[p] != 1 || n >= own.size() || own[n++] != p)) fail("in-frame packed pixels, ascending, are the owned-pixel list", c, r, p);
      if (n != own.size()) fail("owned pixels without a packed position", c, r, n);
      uint64_t ref_owned = 0;
      for (int64_t o : ref_pixel_owner) ref_owned += o == (int64_t)r;
      if (own.size() != ref_owned) fail("n_owned", c, r, own.size());
   }
   if (tiles_sum != ref_tiles) fail("the ranks' tiles add up to the tile count", c, 0, tiles_sum);
   for (uint64_t p = 0; p < W * H; p++)
      if (hits[p] != 1 || ref_pixel_owner[p] < 0) fail("every pixel has exactly one owner", c, 0, p);
}
}  // namespace

int main() {
   const uint32_t sizes[] = {1, 7, 64, 65, 130}, tiles[] = {1, 8, 64, 100}, worlds[] = {1, 2, 3, 8};
   uint32_t idle_ranks = 0;
   for (uint32_t W : sizes)
      for (uint32_t H : sizes)
         for (uint32_t tile : tiles)
            for (uint32_t world : worlds) {
               check(Case{W, H, tile, world});
               if (uh::tile_count(W, H, tile) < world) idle_ranks++;
            }
   check(Case{65, 7, 8, 11});  // 9 tiles, 11 ranks: the last two own nothing
   if (uh::tiles_owned(9, 9, 11) != 0 || uh::pack_pixels(65, 7, 8, 10, 11) != 0 || !idle_ranks) {
      failures++;
      printf("MISMATCH a rank beyond the tile count owns something\n");
   }
   printf("packed positions checked: %llu\n", (unsigned long long)checked);
   if (failures) {
      printf("TILE PARTITION CHECK FAILED: %d\n", failures);
      return 1;
   }
   printf("TILE PARTITION CHECK OK\n");
   return 0;
}
