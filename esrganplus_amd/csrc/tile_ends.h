// tile_ends.h — the kernel bodies of the seven inference end ops (esr_tile, esr_tile_many, esr_tile_img, esr_tile_hr;
// esr_dihedral, esr_tile_x8, esr_tile_set_x8), one body per job.  A body is templated on how its op names a window (the
// resolvers of tile_geom.h: per image, by table, the whole image) and on the format outside (the pixel and slot readers
// below); the __global__ kernels of tile_io.hip and tile_x8.hip are instantiations.  No body knows which op it serves.
// Geometry: tile_geom.h; the x8 index maps: tile_x8_index.h; both walked on the host by tools/set_x8_index_check.cpp.
// Plain loads, stores and VALU.
#pragma once
#include "common.h"
#include "tile_geom.h"
#include "tile_x8_index.h"

namespace {

constexpr int TB_X = 64, TB_Y = 4;   // the plain pair: 64 pixels along x by 4 rows per workgroup

// metrics.hip's quant8(v, 0, 1): the (v - 0) / (1 - 0) of the general form changes no bit
__device__ __forceinline__ uint32_t quant8_unit(float v) { return (uint32_t)(int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

// One pixel as a finished 32-byte channel group of T: chan(e) for e < n and e < LIM, zero in every channel above.
template <typename T, int LIM, typename F>
__device__ __forceinline__ void make_group(u32x4 g[2], int n, F&& chan) {
  constexpr int CPG = DT<T>::CPG;
  alignas(16) T v[CPG];
#pragma unroll
  for (int e = 0; e < CPG; ++e) v[e] = (T)((e < LIM && e < n) ? chan(e) : 0.f);
  g[0] = ((const u32x4*)v)[0];
  g[1] = ((const u32x4*)v)[1];
}

// Logical pixel (row, col) of batch entry `entry` of a one-group G32 view: the halo is one pixel wide.
__device__ __forceinline__ u32x4* g32_px(const esr_g32& g, int64_t entry, int row, int col) {
  return (u32x4*)((char*)g.ptr + entry * g.batch_stride + ((int64_t)(row + 1) * g.wp + col + 1) * 32);
}

// The resolvers and the k range of a kernel, built from the kernel's own parameter struct p in the kernel itself: a helper
// that took p by reference would hide the kernel arguments from the compiler's address-space inference.
#define TILE_PER_IMAGE(p, th, tw, nx, ntiles) TilePerImage{p.nchw, p.B, p.C, p.H, p.W, p.tile, p.pad, p.t_begin, th, tw, nx, ntiles}
#define TILE_BY_TABLE(p) TileTable{(const esr_tile_item*)p.items, p.tile, p.pad, p.th, p.tw}
#define X8_RANGE(p, n_windows) X8Range{p.k_begin, p.k_count, n_windows, p.accumulate, p.mean_scale}

// ---- pixel readers: image pixel (y, x) of a window's image -> a channel group of T; `in` = 0 reads nothing, all zero.

// fp32 NCHW planes, C strided reads; LIM = the most channels the op admits
template <int LIM>
struct PxF32 {
  template <typename T>
  __device__ __forceinline__ void read(const TileWin w, int C, int y, int x, bool in, u32x4 g[2]) const {
    const int64_t plane = (int64_t)w.H * w.W;
    const float* const src = (const float*)w.img + (int64_t)y * w.W + x;
    make_group<T, LIM>(g, in ? C : 0, [&](int e) { return src[e * plane]; });
  }
};

// uint8 HWC, C = 1 or 3 bytes and one true division each; slot channel 0 is R whatever the order in memory
struct PxU8 {
  int bgr;
  template <typename T>
  __device__ __forceinline__ void read(const TileWin w, int C, int y, int x, bool in, u32x4 g[2]) const {
    const uint8_t* const src = (const uint8_t*)w.img + ((int64_t)y * w.W + x) * C;
    const bool swap = bgr && C == 3;
    make_group<T, 3>(g, in ? C : 0, [&](int e) { return __fdiv_rn((float)src[swap ? 2 - e : e], 255.0f); });
  }
};

// ---- the plain pair

// One thread = one pixel of one window: one finished 32-byte channel group out.
template <typename T, typename R, typename PX>
__device__ __forceinline__ void plain_gather(const R r, const PX& px, int C, const esr_g32 g32) {
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= r.tw || row >= r.th) return;
  const TileWin w = R::gather(r, blockIdx.z);
  u32x4 grp[2];
  px.template read<T>(w, C, w.ay.w0 + row, w.ax.w0 + col, true, grp);
  u32x4* const dst = g32_px(g32, blockIdx.z, row, col);
  dst[0] = grp[0];
  dst[1] = grp[1];
}

// The lane of a plain stitch: one thread = four HR pixels along x (one LR column) of one HR row of a window's owned
// rectangle.  False outside the rectangle; else the 16-byte unit of its first of C source planes, and the index of
// that LR column in the HR image, dst_unit = Y W + x (every HR offset and row pitch is a multiple of four pixels).
template <typename R>
__device__ __forceinline__ bool stitch_lane(const R r, const TileWin w, int C, const float* slots_nchw, const f32x4*& src,
                                            int64_t& src_plane, int64_t& dst_unit) {
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= w.ax.on || row >= 4 * w.ay.on) return false;
  src_plane = (int64_t)4 * r.th * r.tw;   // in 16-byte units
  src = (const f32x4*)slots_nchw + (int64_t)blockIdx.z * C * src_plane + (int64_t)(4 * (w.ay.o0 - w.ay.w0) + row) * r.tw +
        (w.ax.o0 - w.ax.w0) + col;
  dst_unit = (int64_t)(4 * w.ay.o0 + row) * w.W + w.ax.o0 + col;
  return true;
}

// fp32 NCHW out, bit for bit: 16-byte loads and stores, all C channels.
template <typename R>
__device__ __forceinline__ void plain_stitch(const R r, int C, const float* slots_nchw) {
  const TileWin w = R::stitch(r, blockIdx.z);
  if (!w.live) return;
  const f32x4* src;
  int64_t src_plane, dst_unit;
  if (!stitch_lane(r, w, C, slots_nchw, src, src_plane, dst_unit)) return;
  const int64_t dst_plane = (int64_t)4 * w.H * w.W;   // in 16-byte units
  f32x4* const dst = (f32x4*)w.img + dst_unit;
  for (int c = 0; c < C; ++c) dst[c * dst_plane] = src[c * src_plane];
}

// ---- the x8 pair: 32 x 32 pixels per workgroup, one pixel per thread

// The part of an x8 op's parameters the bodies read: transforms [k_begin, k_begin + k_count) of n_windows windows.
struct X8Range {
  int k_begin, k_count, n_windows, accumulate;
  float mean_scale;
};

// Every slot of the range is written from ONE read of the window's 32 x 32 tile: it is staged in the LDS as finished
// 32-byte channel groups, straight slots take their own pixel, transposed slots the mirrored one — so that both the
// reads of the image and the G32 writes run along x.  Window-local coordinates throughout: the transforms turn the
// WINDOW (th x tw).  A filler window is gathered like any other.
template <typename T, typename R, typename PX>
__device__ __forceinline__ void x8_gather(const R r, const PX& px, int C, const esr_g32 g32, const X8Range& kr) {
  __shared__ u32x4 tile[X8_TILE][X8_TILE + 1][2];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x0 = blockIdx.x * X8_TILE, y0 = blockIdx.y * X8_TILE;
  const int z = blockIdx.z, th = r.th, tw = r.tw;
  const TileWin w = R::gather(r, z);
  u32x4 own[2];                       // this thread's window pixel (y0 + ly, x0 + lx) as a finished 32-byte channel group
  {
    const int sy = y0 + ly, sx = x0 + lx;
    const bool in = sy < th && sx < tw;
    px.template read<T>(w, C, w.ay.w0 + (in ? sy : 0), w.ax.w0 + (in ? sx : 0), in, own);
    tile[ly][lx][0] = own[0];
    tile[ly][lx][1] = own[1];
  }
  __syncthreads();
  for (int i = 0; i < kr.k_count; ++i) {
    const int k = kr.k_begin + i;
    const bool tr = (k & 4) != 0;
    // source pixel of this thread: consecutive lanes walk the slot's x
    const int ty = tr ? lx : ly, tx = tr ? ly : lx;
    const int sy = y0 + ty, sx = x0 + tx;
    if (sy >= th || sx >= tw) continue;
    const X8Pos at = x8_gather_pos(k, th, tw, sy, sx);
    u32x4* const dst = g32_px(g32, x8_entry(i, kr.n_windows, z), at.row, at.col);
    // straight slots: the thread's own pixel from registers; transposed slots: the mirrored LDS entry
    dst[0] = tr ? tile[ty][tx][0] : own[0];
    dst[1] = tr ? tile[ty][tx][1] : own[1];
  }
}

// ---- slot readers of the reduce: what R_k puts at window-local pixel (y, x) of an hh x hw output (tile_x8_index.h), out of
// slot k of batch entry `entry`, as the 32 bytes that pass through the LDS; get(raw, e) is its channel e < N.

// fp32 NCHW [entries][C][rows][cols], what a conv's nchw_out leaves
struct SlotNCHW {
  static constexpr int N = 8;
  const float* slots;
  __device__ __forceinline__ void load(int64_t entry, int C, int k, int hh, int hw, int y, int x, u32x4 raw[2]) const {
    const int64_t plane = (int64_t)hh * hw;
    const float* const src = slots + entry * C * plane + x8_reduce_src(k, hh, hw, y, x);
    alignas(16) float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < C ? src[e * plane] : 0.f;
    raw[0] = ((const u32x4*)v)[0];
    raw[1] = ((const u32x4*)v)[1];
  }
  static __device__ __forceinline__ float get(const u32x4 raw[2], int e) { return ((const float*)raw)[e]; }
};

// the logical pixels of a one-group G32 view of T (esr_dihedral without slots_nchw)
template <typename T>
struct SlotG32 {
  static constexpr int N = DT<T>::CPG;
  esr_g32 g32;
  __device__ __forceinline__ void load(int64_t entry, int, int k, int hh, int hw, int y, int x, u32x4 raw[2]) const {
    const X8Pos at = x8_reduce_pos(k, hh, hw, y, x);
    const u32x4* const src = g32_px(g32, entry, at.row, at.col);
    raw[0] = src[0];
    raw[1] = src[1];
  }
  static __device__ __forceinline__ float get(const u32x4 raw[2], int e) { return (float)((const T*)raw)[e]; }
};

// One thread = one pixel of a live window's owned rectangle on the result's side (S = R::SCALE times the LR window), all
// channels: a = accumulate ? PARTIAL : 0; a += R_k(o_k) for k ascending (one fp32 add each), the inverse index taken in
// window-local coordinates; a * mean_scale out.  Transposed slots are read along THEIR x and turned through the LDS.
// NC = 0: the fp32 NCHW result of the window's image carries the partial sum (C channels).  NC = 1, 3: the uint8 HWC
// result cannot; the partial sum lives in acc_buf, and the last range quantises and sends the workgroup's rows out
// through the LDS as aligned dwords.  Every lane is bounded by the owned rectangle.
template <int NC, typename R, typename SR>
__device__ __forceinline__ void x8_reduce(const R r, const SR& slots, int C_, const X8Range& kr, int bgr, float* acc_buf) {
  constexpr int S = R::SCALE, N = SR::N;
  __shared__ u32x4 tile[X8_TILE][X8_TILE + 1][2];
  const int z = blockIdx.z;
  const TileWin w = R::stitch(r, z);
  if (!w.live) return;                              // a filler or repeated window: neither read nor written
  const TileAxis ay = w.ay, ax = w.ax;
  const int oh = S * ay.on, ow = S * ax.on;         // the owned rectangle
  const int x0 = blockIdx.x * X8_TILE, y0 = blockIdx.y * X8_TILE;
  if (x0 >= ow || y0 >= oh) return;                 // whole workgroup outside this window's rectangle
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int hh = S * r.th, hw = S * r.tw;           // the window's output
  const int wy = S * (ay.o0 - ay.w0), wx = S * (ax.o0 - ax.w0);   // the owned rectangle inside it
  const bool own = y0 + ly < oh && x0 + lx < ow;
  const int C = NC ? NC : C_;
  const int64_t src_plane = (int64_t)hh * hw;
  // where the partial sum of this pixel lives, and the pitch of its channels
  const int64_t part_plane = NC ? src_plane : (int64_t)(S * S) * w.H * w.W;
  float* part = nullptr;
  if (own) {
    if constexpr (NC != 0) part = acc_buf ? acc_buf + x8_acc_offset(z, 0, C, hh, hw, wy + y0 + ly, wx + x0 + lx) : nullptr;
    else part = (float*)w.img + (int64_t)(S * ay.o0 + y0 + ly) * (S * w.W) + S * ax.o0 + x0 + lx;
  }
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = (own && kr.accumulate && e < C) ? part[e * part_plane] : 0.f;
  for (int i = 0; i < kr.k_count; ++i) {
    const int k = kr.k_begin + i;
    const int64_t entry = x8_entry(i, kr.n_windows, z);
    alignas(16) u32x4 raw[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (!(k & 4)) {
      if (own) slots.load(entry, C, k, hh, hw, wy + y0 + ly, wx + x0 + lx, raw);
    } else {
      // this thread fetches the value of owned pixel (y0 + lx, x0 + ly): consecutive lanes walk the slot's x
      const int oy = y0 + lx, ox = x0 + ly;
      __syncthreads();                       // the previous turn's reads are done
      if (oy < oh && ox < ow) {
        slots.load(entry, C, k, hh, hw, wy + oy, wx + ox, raw);
        tile[lx][ly][0] = raw[0];
        tile[lx][ly][1] = raw[1];
      }
      __syncthreads();
      if (own) {
        raw[0] = tile[ly][lx][0];
        raw[1] = tile[ly][lx][1];
      }
    }
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = (i == 0 && !kr.accumulate) ? SR::get(raw, e) : __fadd_rn(acc[e], SR::get(raw, e));
  }
  if constexpr (NC == 0) {
    if (!own) return;
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (e < C) part[e * part_plane] = __fmul_rn(acc[e], kr.mean_scale);
  } else {
    if (!x8_last_range(kr.k_begin, kr.k_count)) {
      if (!own) return;
#pragma unroll
      for (int e = 0; e < NC; ++e) part[e * part_plane] = __fmul_rn(acc[e], kr.mean_scale);
      return;
    }
    // the last range: the workgroup's 32 rows of 32 pixels as bytes in the LDS, then one aligned dword per lane
    uint8_t* const bytes = (uint8_t*)&tile[0][0][0];
    __syncthreads();                         // the last turn's reads are done
    if (own) {
      const bool swap = bgr && NC == 3;
#pragma unroll
      for (int e = 0; e < NC; ++e) bytes[(ly * X8_TILE + lx) * NC + (swap ? 2 - e : e)] = (uint8_t)quant8_unit(__fmul_rn(acc[e], kr.mean_scale));
    }
    __syncthreads();
    const int n = ow - x0 < X8_TILE ? ow - x0 : X8_TILE;      // owned pixels of these rows: a multiple of 4
    if (y0 + ly < oh && lx < x8_row_dwords(n, NC)) {
      uint8_t* const row = (uint8_t*)w.img + ((int64_t)(S * ay.o0 + y0 + ly) * (S * w.W) + S * ax.o0 + x0) * NC;
      ((uint32_t*)row)[lx] = ((const uint32_t*)bytes)[ly * (X8_TILE * NC / 4) + lx];
    }
  }
}

}  // namespace
