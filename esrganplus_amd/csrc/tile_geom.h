// tile_geom.h — the geometry every tiled end derives from tile, pad and a tile index (include/esrgan_hip.h: esr_tile):
// tile_io.hip, tile_x8.hip and tile_img.hip share it, so that a window is the same window in all of them.
#pragma once
#include "common.h"

namespace {

// One axis of tile i: the owned range [o0, o0 + on) and the start w0 of its window of `win` pixels, in an image of n.
struct TileAxis { int o0, on, w0; };

__host__ __device__ __forceinline__ int tile_window(int n, int tile, int pad) {
  const int64_t w = (int64_t)tile + 2 * (int64_t)pad;
  return w < n ? (int)w : n;
}

__host__ __device__ __forceinline__ int tile_count(int n, int tile) { return (n - 1) / tile + 1; }

__device__ __forceinline__ TileAxis tile_axis(int n, int tile, int pad, int win, int i) {
  TileAxis a;
  a.o0 = i * tile;                                  // i < ceil(n / tile), so o0 <= n - 1
  a.on = n - a.o0 < tile ? n - a.o0 : tile;
  const int w = a.o0 - pad;
  a.w0 = w < 0 ? 0 : (w > n - win ? n - win : w);   // shifted inward at the borders
  return a;
}

}  // namespace
