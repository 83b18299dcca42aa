// path_layout.h — where a path's records lie in a slot's state allocation (device_types.h PathState): the sizes Slot::create
// allocates and the address of every quad and pair the kernels read and write, as plain arithmetic that a host program can check
// (tests/cpp/path_layout_check.cpp). No HIP types: offsets in bytes from the first record of a set.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define UH_LAYOUT_HD __host__ __device__
#else
#define UH_LAYOUT_HD
#endif

namespace uh {

constexpr uint32_t kLayoutShards = 32;      // = kShards (device_types.h asserts it)
constexpr uint32_t kLayoutShardBits = 5;
constexpr uint32_t kRecQuadBytes = 16, kRecPairBytes = 8;
constexpr size_t kPlaneStaggerBytes = 4352;  // 4 KiB + 256 B between the planes: the same index of two planes must not alias in the caches

// Fibonacci hash of the 64-path run index (top 5 bits): the shard a run of 64 path ids lives in (device_types.h shard_of_run)
UH_LAYOUT_HD inline uint32_t layout_shard_of_run(uint32_t run) { return (run * 0x9E3779B1u) >> (32 - kLayoutShardBits); }

// entries of one shard's queue segment for n path ids: exact, the largest number of 64-path runs one shard receives, in paths
inline uint32_t layout_shard_cap(size_t n) {
   const uint32_t runs = (uint32_t)((n + 63) / 64);
   uint32_t per_shard[kLayoutShards] = {0}, cap = 0;
   for (uint32_t r = 0; r < runs; r++) per_shard[layout_shard_of_run(r)]++;
   for (uint32_t s = 0; s < kLayoutShards; s++) cap = per_shard[s] * 64 > cap ? per_shard[s] * 64 : cap;
   return cap;
}
// quads between two planes of a set: the positions a queue can hold (kShards segments; never fewer than the path ids) plus the stagger
inline size_t layout_plane_quads(size_t n, uint32_t shard_cap) {
   const size_t cap_q = (size_t)shard_cap * kLayoutShards;
   return (n > cap_q ? n : cap_q) + kPlaneStaggerBytes / kRecQuadBytes;
}

// Byte offset, from the set's first record, of what lies at queue position `pos` in plane `quad` (0..3). Every plane holds 16-byte
// quads by position - except, with `pairs` (FrameParams::slim_state), plane 3: 8-byte pairs by the same position, in the plane's
// first half. `plane` = quads between two planes (layout_plane_quads).
UH_LAYOUT_HD inline size_t rec_offset(size_t plane, uint32_t pos, int quad, bool pairs = false) {
   return (plane * (size_t)quad) * kRecQuadBytes + (size_t)pos * ((pairs && quad == 3) ? kRecPairBytes : kRecQuadBytes);
}

}  // namespace uh
