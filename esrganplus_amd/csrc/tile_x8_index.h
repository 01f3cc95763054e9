// tile_x8_index.h — the index and accumulator arithmetic of the x8 ends (include/esrgan_hip.h: esr_dihedral, esr_tile_x8,
// esr_tile_set_x8), free of any HIP header so that a host program can include it alone: which batch entry a slot is,
// where a window pixel lands in slot k, which element of slot k's output R_k puts at a window-local pixel, where a
// partial sum lives in acc, when acc is read and written, and what the entries refuse about a k range.  tile_ends.h uses
// exactly these on the device, for all three ops: an image is a window that is the whole image.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define X8_HD __host__ __device__ __forceinline__
#else
#define X8_HD inline
#endif

namespace {

constexpr int X8_TILE = 32;   // 32 x 32 pixels per workgroup, one pixel per thread

struct X8Pos { int row, col; };

X8_HD int x8_flip(bool on, int n, int i) { return on ? n - 1 - i : i; }

// Batch entry of the i-th transform of the range (k = k_begin + i) of window p of P.  esr_tile_x8's ((i t_count + s) B + b)
// is this at p = s B + b, P = t_count B; esr_dihedral's i B + b at p = b, P = B.
X8_HD int64_t x8_entry(int i, int P, int p) { return (int64_t)i * P + p; }

// Gather: the logical pixel of slot k (th x tw for k < 4, tw x th for k >= 4) that takes pixel (sy, sx) of the upright
// th x tw window: slot_k[y][x] = win[ys(y)][xs(x)] (k < 4), slot_k[p][q] = win[ys(q)][xs(p)] (k >= 4), the flips being
// their own inverses.
X8_HD X8Pos x8_gather_pos(int k, int th, int tw, int sy, int sx) {
  const int fy = x8_flip((k & 2) != 0, th, sy), fx = x8_flip((k & 1) != 0, tw, sx);
  return (k & 4) ? X8Pos{fx, fy} : X8Pos{fy, fx};
}

// Stitch-reduce: the pixel of slot k's output (hh x hw for k < 4, hw x hh for k >= 4; hh x hw the upright window's
// output) that R_k puts at window-local pixel (y, x): R_k(o)[y][x] = o_k[ys(y)][xs(x)] (k < 4), o_k[xs(x)][ys(y)]
// (k >= 4): the gather's map on the output's size.  x8_reduce_src is its offset inside one channel plane of that output.
X8_HD X8Pos x8_reduce_pos(int k, int hh, int hw, int y, int x) { return x8_gather_pos(k, hh, hw, y, x); }
X8_HD int64_t x8_reduce_src(int k, int hh, int hw, int y, int x) {
  const X8Pos at = x8_reduce_pos(k, hh, hw, y, x);
  return (int64_t)at.row * ((k & 4) ? hh : hw) + at.col;
}

// acc is fp32 [P][C][hh][hw], upright and window-local.
X8_HD int64_t x8_acc_offset(int p, int c, int C, int hh, int hw, int y, int x) {
  return (((int64_t)p * C + c) * hh + y) * hw + x;
}

// The 8-bit form keeps the partial sum of the ranges so far in acc: read with accumulate, written before the last range.
X8_HD bool x8_last_range(int k_begin, int k_count) { return k_begin + k_count == 8; }
X8_HD bool x8_acc_read(int img, int accumulate) { return img && accumulate; }
X8_HD bool x8_acc_write(int img, int k_begin, int k_count) { return img && !x8_last_range(k_begin, k_count); }
X8_HD bool x8_acc_needed(int img, int accumulate, int k_begin, int k_count) {
  return x8_acc_read(img, accumulate) || x8_acc_write(img, k_begin, k_count);
}

// A k range: 0 = fine, 1 = outside [0, 8), 2 = across k = 4 with a non-square window (th x tw and tw x th slots in one pass).
X8_HD int x8_range_error(int k_begin, int k_count, int th, int tw) {
  if (k_begin < 0 || k_count < 1 || (int64_t)k_begin + k_count > 8) return 1;
  if (k_begin < 4 && k_begin + k_count > 4 && th != tw) return 2;
  return 0;
}

// The dwords of one row of a workgroup's 32 pixels, of which the first n (a multiple of 4) are owned: n C / 4.
X8_HD int x8_row_dwords(int n, int C) { return n * C / 4; }

}  // namespace
