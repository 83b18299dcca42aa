// tile_partition.h - which rank of a job owns which pixel of a frame split into square tiles (uh_set_tile_partition), as host + device
// functions: tile t of the row-major tile grid belongs to rank t % world, and a rank's tiles are packed in ascending tile order, each
// whole and row-major (the frame's ragged edge is padding). partition.hip counts and lists with them, tiles.hip packs and composes
// with them, and tests/cpp/tile_partition_check.cpp runs THE SAME EXPRESSIONS on the host against loops over tiles and pixels.
// Pixel and tile indices are 32-bit, packed positions 64-bit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define UH_TILE_HD __host__ __device__
#else
#define UH_TILE_HD
#endif

namespace uh {

// tiles in one row of the tile grid of a frame W wide (with H: in one column); tiles of the frame
UH_TILE_HD inline uint32_t tiles_across(uint32_t W, uint32_t tile) { return (W + tile - 1) / tile; }
UH_TILE_HD inline uint32_t tile_count(uint32_t W, uint32_t H, uint32_t tile) { return tiles_across(W, tile) * tiles_across(H, tile); }
// the tile pixel (x, y) lies in; the rank that owns a tile, and a pixel
UH_TILE_HD inline uint32_t tile_of_pixel(uint32_t x, uint32_t y, uint32_t tile, uint32_t tiles_x) { return (y / tile) * tiles_x + x / tile; }
UH_TILE_HD inline uint32_t tile_owner(uint32_t t, uint32_t world) { return t % world; }
UH_TILE_HD inline uint32_t pixel_owner(uint32_t x, uint32_t y, uint32_t tile, uint32_t tiles_x, uint32_t world) { return tile_owner(tile_of_pixel(x, y, tile, tiles_x), world); }
// tiles `rank` owns out of num_tiles (rank, rank + world, ...: never more than a lower rank), and the pixels of its packed buffer
UH_TILE_HD inline uint32_t tiles_owned(uint32_t num_tiles, uint32_t rank, uint32_t world) { return num_tiles > rank ? (num_tiles - rank + world - 1) / world : 0; }
UH_TILE_HD inline uint64_t pack_pixels(uint32_t W, uint32_t H, uint32_t tile, uint32_t rank, uint32_t world) { return (uint64_t)tiles_owned(tile_count(W, H, tile), rank, world) * tile * tile; }

// the pixel at position i of rank's packed buffer; inside: it lies in the frame (false: padding of a tile at the frame's edge)
struct PackedPixel { uint32_t x, y; bool inside; };
UH_TILE_HD inline PackedPixel packed_pixel(uint64_t i, uint32_t W, uint32_t H, uint32_t tile, uint32_t tiles_x, uint32_t rank, uint32_t world) {
   const uint32_t local = (uint32_t)(i / (tile * tile)), within = (uint32_t)(i % (tile * tile));
   const uint32_t t = rank + local * world;
   const uint32_t x = (t % tiles_x) * tile + within % tile, y = (t / tiles_x) * tile + within / tile;
   return PackedPixel{x, y, x < W && y < H};
}
// ... and back: the position of pixel (x, y) of tile t in its owner's packed buffer
UH_TILE_HD inline uint64_t packed_position(uint32_t t, uint32_t x, uint32_t y, uint32_t tile, uint32_t world) { return (uint64_t)(t / world) * tile * tile + (y % tile) * tile + x % tile; }

}  // namespace uh
