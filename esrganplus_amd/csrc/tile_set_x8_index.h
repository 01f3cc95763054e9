// tile_set_x8_index.h — the index and accumulator arithmetic of esr_tile_set_x8 (include/esrgan_hip.h), free of any HIP
// header so that a host program can include it alone: which batch entry a slot is, where a window pixel lands in slot k,
// which element of slot k's output R_k puts at a window-local HR pixel, where a partial sum lives in acc, when acc is
// read and written, and what the entry refuses about a k range.  tile_set_x8.hip uses exactly these on the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SX8_HD __host__ __device__ __forceinline__
#else
#define SX8_HD inline
#endif

namespace {

constexpr int SX8_TILE = 32;   // 32 x 32 pixels per workgroup, one pixel per thread

struct SX8Pos { int row, col; };

SX8_HD int sx8_flip(bool on, int n, int i) { return on ? n - 1 - i : i; }

// Batch entry of the i-th transform of the range (k = k_begin + i) of window p of P: esr_tile_x8's index at B = 1.
SX8_HD int64_t sx8_entry(int i, int P, int p) { return (int64_t)i * P + p; }

// Gather: the logical pixel of slot k (th x tw for k < 4, tw x th for k >= 4) that takes pixel (sy, sx) of the upright
// th x tw window: slot_k[y][x] = win[ys(y)][xs(x)] (k < 4), slot_k[p][q] = win[ys(q)][xs(p)] (k >= 4), the flips being
// their own inverses.
SX8_HD SX8Pos sx8_gather_pos(int k, int th, int tw, int sy, int sx) {
  const int fy = sx8_flip((k & 2) != 0, th, sy), fx = sx8_flip((k & 1) != 0, tw, sx);
  return (k & 4) ? SX8Pos{fx, fy} : SX8Pos{fy, fx};
}

// Stitch-reduce: the offset inside one channel plane of slot k's output (hh x hw for k < 4, hw x hh for k >= 4;
// hh x hw = 4 th x 4 tw the upright window's output) of the element R_k puts at window-local HR pixel (y, x):
// R_k(o)[y][x] = o_k[ys(y)][xs(x)] (k < 4), o_k[xs(x)][ys(y)] (k >= 4).
SX8_HD int64_t sx8_reduce_src(int k, int hh, int hw, int y, int x) {
  const int fy = sx8_flip((k & 2) != 0, hh, y), fx = sx8_flip((k & 1) != 0, hw, x);
  return (k & 4) ? (int64_t)fx * hh + fy : (int64_t)fy * hw + fx;
}

// acc is fp32 [P][C][hh][hw], upright and window-local.
SX8_HD int64_t sx8_acc_offset(int p, int c, int C, int hh, int hw, int y, int x) {
  return (((int64_t)p * C + c) * hh + y) * hw + x;
}

// The 8-bit form keeps the partial sum of the ranges so far in acc: read with accumulate, written before the last range.
SX8_HD bool sx8_last_range(int k_begin, int k_count) { return k_begin + k_count == 8; }
SX8_HD bool sx8_acc_read(int img, int accumulate) { return img && accumulate; }
SX8_HD bool sx8_acc_write(int img, int k_begin, int k_count) { return img && !sx8_last_range(k_begin, k_count); }
SX8_HD bool sx8_acc_needed(int img, int accumulate, int k_begin, int k_count) {
  return sx8_acc_read(img, accumulate) || sx8_acc_write(img, k_begin, k_count);
}

// A k range: 0 = fine, 1 = outside [0, 8), 2 = across k = 4 with a non-square window (th x tw and tw x th slots in one pass).
SX8_HD int sx8_range_error(int k_begin, int k_count, int th, int tw) {
  if (k_begin < 0 || k_count < 1 || (int64_t)k_begin + k_count > 8) return 1;
  if (k_begin < 4 && k_begin + k_count > 4 && th != tw) return 2;
  return 0;
}

// The dwords of one row of a workgroup's 32 HR pixels, of which the first n (a multiple of 4) are owned: n C / 4.
SX8_HD int sx8_row_dwords(int n, int C) { return n * C / 4; }

}  // namespace
