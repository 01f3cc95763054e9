// tile_geom.h — the geometry every tiled end derives from tile, pad and a tile index (include/esrgan_hip.h: esr_tile), and
// the resolution of "which window is this workgroup's" for the three ways an op names its windows: per image, by a device
// table, or the whole image.  Free of any HIP header, like tile_x8_index.h, so that a host program can walk exactly the
// arithmetic the kernels of tile_ends.h run.
#pragma once
#include <stdint.h>

#include "../../include/esrgan_hip.h"

#if defined(__HIPCC__)
#define TILE_HD __host__ __device__ __forceinline__
#else
#define TILE_HD inline
#endif

namespace {

// One axis of tile i: the owned range [o0, o0 + on) and the start w0 of its window of `win` pixels, in an image of n.
struct TileAxis { int o0, on, w0; };

TILE_HD int tile_window(int n, int tile, int pad) {
  const int64_t w = (int64_t)tile + 2 * (int64_t)pad;
  return w < n ? (int)w : n;
}

TILE_HD int tile_count(int n, int tile) { return (n - 1) / tile + 1; }

TILE_HD TileAxis tile_axis(int n, int tile, int pad, int win, int i) {
  TileAxis a;
  a.o0 = i * tile;                                  // i < ceil(n / tile), so o0 <= n - 1
  a.on = n - a.o0 < tile ? n - a.o0 : tile;
  const int w = a.o0 - pad;
  a.w0 = w < 0 ? 0 : (w > n - win ? n - win : w);   // shifted inward at the borders
  return a;
}

// The window of one workgroup (blockIdx.z = z): its image on this op's side, that image's LR size, the tile and its two
// axes.  live = 0: a filler the stitch neither reads nor writes (the gather fills it like any other window).
struct TileWin {
  void* img;
  int H, W, t, live;
  TileAxis ay, ax;
};

static_assert(sizeof(esr_tile_item) == 24 && sizeof(esr_tile_img_item) == 24 && sizeof(esr_tile_hr_item) == 24 &&
              offsetof(esr_tile_img_item, H) == offsetof(esr_tile_item, H) && offsetof(esr_tile_hr_item, H) == offsetof(esr_tile_item, H) &&
              offsetof(esr_tile_img_item, live) == offsetof(esr_tile_item, live) && offsetof(esr_tile_hr_item, live) == offsetof(esr_tile_item, live),
              "one 24-byte table entry per window, whatever its pointer names");

// The resolvers are plain data with static functions that take them by value: a `this` pointer would keep them in memory
// through the device compiler's address-space inference, and loads through a table's pointers would become flat ones.

// Per image (esr_tile, esr_tile_x8): z = s B + b, slot s is tile t_begin + s of image b of nchw [B][C][H][W], H x W the
// image of this op's side.  th, tw, nx, ntiles come from the entry, which has them anyway.
struct TilePerImage {
  static constexpr int SCALE = 4;
  float* nchw;
  int B, C, H, W, tile, pad, t_begin, th, tw, nx, ntiles;
  // A tail pass (t_begin + s >= ntiles) repeats the last tile, so that the gather leaves no slot with stale data; the
  // repeated windows are not live, so the stitch neither reads nor writes them.  hl x wl: the LR image.
  static TILE_HD TileWin win(const TilePerImage r, int z, int hl, int wl) {
    const int s = z / r.B, b = z - s * r.B;
    const int live = r.t_begin + s < r.ntiles, t = live ? r.t_begin + s : r.ntiles - 1;
    return {r.nchw + (int64_t)b * r.C * ((int64_t)r.H * r.W), hl, wl, t, live, tile_axis(hl, r.tile, r.pad, r.th, t / r.nx),
            tile_axis(wl, r.tile, r.pad, r.tw, t % r.nx)};
  }
  static TILE_HD TileWin gather(const TilePerImage r, int z) { return win(r, z, r.H, r.W); }
  // H, W are the HR image on the stitch side: scale 4, the entry refuses any other
  static TILE_HD TileWin stitch(const TilePerImage r, int z) { return win(r, z, r.H >> 2, r.W >> 2); }
};

// By table (esr_tile_many, esr_tile_img, esr_tile_hr, esr_tile_set_x8): z indexes the table, the item names the image,
// its LR size on both sides and the tile.
struct TileTable {
  static constexpr int SCALE = 4;
  const esr_tile_item* items;
  int tile, pad, th, tw;
  static TILE_HD TileWin gather(const TileTable r, int z) {
    const esr_tile_item it = r.items[z];
    const int nx = tile_count(it.W, r.tile);
    return {it.nchw, it.H, it.W, it.t, it.live, tile_axis(it.H, r.tile, r.pad, r.th, it.t / nx), tile_axis(it.W, r.tile, r.pad, r.tw, it.t % nx)};
  }
  static TILE_HD TileWin stitch(const TileTable r, int z) { return gather(r, z); }
};

// The whole image (esr_dihedral): z = b, the window is the image, its origin 0, there is one tile, and H x W = th x tw
// are those of the op's side already, so the stitch side's scale is 1 whatever the net's is.
struct TileWhole {
  static constexpr int SCALE = 1;
  float* nchw;
  int C, th, tw;
  static TILE_HD TileWin gather(const TileWhole r, int z) {
    return {r.nchw + (int64_t)z * r.C * ((int64_t)r.th * r.tw), r.th, r.tw, 0, 1, TileAxis{0, r.th, 0}, TileAxis{0, r.tw, 0}};
  }
  static TILE_HD TileWin stitch(const TileWhole r, int z) { return gather(r, z); }
};

}  // namespace
