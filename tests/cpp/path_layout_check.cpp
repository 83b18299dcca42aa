// path_layout_check - csrc/path_layout.h (product code: the sizes Slot::create allocates for a slot's path state and the address of
// every quad and pair the kernels touch, rec_offset behind device_types.h rec_quad / rec_pair) on the host, meant to be built with
// -fsanitize=address,undefined. For a few capacities, the 64-path minimum included, and both layouts (four quads; slim: three quads
// and a pair): a set's allocation is modelled as one heap block of exactly four planes, every record of every queue position is
// written with a tag of its (plane, position) through rec_offset and read back - two records that overlap, or a plane that reaches
// into the next, lose a tag; AddressSanitizer sees an address beyond the set. Every pair must lie inside plane 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_layout.h"

namespace {
int failures = 0;
void fail(const char* what, size_t n, bool pairs, int quad, uint32_t pos) {
   if (failures++ < 20) printf("MISMATCH %s: capacity %zu, %s layout, plane %d, position %u\n", what, n, pairs ? "slim" : "four-quad", quad, pos);
}

size_t check_capacity(size_t n, bool pairs) {
   const uint32_t shard_cap = uh::layout_shard_cap(n);
   if (shard_cap == 0 || shard_cap % 64 != 0) fail("shard_cap is a positive multiple of 64", n, pairs, 0, shard_cap);
   const size_t positions = (size_t)shard_cap * uh::kLayoutShards;  // queue positions: shard segment + position in the shard's queue
   if (positions < n) fail("fewer positions than path ids", n, pairs, 0, 0);
   // every run of 64 ids fits its shard's segment
   std::vector<uint32_t> per_shard(uh::kLayoutShards, 0);
   for (uint32_t r = 0; r < (n + 63) / 64; r++)
      if (++per_shard[uh::layout_shard_of_run(r)] * 64u > shard_cap) fail("a shard receives more runs than its segment holds", n, pairs, 0, r);
   const size_t plane = uh::layout_plane_quads(n, shard_cap);
   if (plane < positions + uh::kPlaneStaggerBytes / uh::kRecQuadBytes) fail("plane stride below positions + stagger", n, pairs, 0, 0);
   const size_t plane_bytes = plane * uh::kRecQuadBytes;
   // one set: exactly four planes on the heap
   std::vector<uint8_t> set(4 * plane_bytes, 0);
   uint8_t* base = set.data();
   size_t records = 0;
   auto size_of = [&](int q) { return (pairs && q == 3) ? uh::kRecPairBytes : uh::kRecQuadBytes; };
   auto tag = [&](int q, uint32_t pos, uint32_t word) { return ((uint32_t)q << 30) ^ (pos * 4u + word) ^ 0x5bd1e995u; };
   for (int q = 0; q < 4; q++)
      for (uint32_t pos = 0; pos < positions; pos++) {
         const size_t at = uh::rec_offset(plane, pos, q, pairs), bytes = size_of(q);
         if (at % bytes != 0) fail("record not aligned to its size", n, pairs, q, pos);
         if (at < (size_t)q * plane_bytes || at + bytes > (size_t)(q + 1) * plane_bytes) {
            fail(q == 3 && pairs ? "pair outside its plane" : "quad outside its plane", n, pairs, q, pos);
            continue;
         }
         for (uint32_t w = 0; w < bytes / 4; w++) {
            const uint32_t t = tag(q, pos, w);
            std::memcpy(base + at + 4 * w, &t, 4);
         }
         records++;
      }
   for (int q = 0; q < 4; q++)
      for (uint32_t pos = 0; pos < positions; pos++) {
         const size_t at = uh::rec_offset(plane, pos, q, pairs), bytes = size_of(q);
         if (at + bytes > set.size()) continue;  // reported above
         for (uint32_t w = 0; w < bytes / 4; w++) {
            uint32_t t = 0;
            std::memcpy(&t, base + at + 4 * w, 4);
            if (t != tag(q, pos, w)) fail("two records overlap", n, pairs, q, pos);
         }
      }
   // the four-quad form of the address is the plain one the kernels were written against
   for (int q = 0; q < 4; q++)
      if (uh::rec_offset(plane, 7, q) != (plane * (size_t)q + 7) * 16) fail("rec_offset is base + plane * quad + pos", n, pairs, q, 7);
   return records;
}
}  // namespace

int main() {
   // 64: the minimum a slot is created with; one run more; sizes that are no multiple of 64 or of the shard count; a 128 x 72 frame,
   // 16 of them, and the 67 x 41 and 200 x 120 frames of the GPU tests
   const size_t capacities[] = {64, 65, 128, 2048, 2049, 2747, 9216, 24000, 147456, 100003};
   size_t records = 0;
   for (size_t n : capacities)
      for (bool pairs : {false, true}) records += check_capacity(n, pairs);
   printf("records checked: %zu\n", records);
   if (failures) {
      printf("PATH LAYOUT CHECK FAILED: %d\n", failures);
      return 1;
   }
   printf("PATH LAYOUT CHECK OK\n");
   return 0;
}
