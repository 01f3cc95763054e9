// tile_io.hip — the two ends of tiled inference: gather = fixed-size windows of an NCHW fp32 image -> G32 slots,
// stitch = the owned rectangle of every window's fp32 NCHW output -> the caller's NCHW image.  Geometry:
// include/esrgan_hip.h (esr_tile); both kernels derive it from tile, pad and the tile index.  Plain loads and stores.
// esr_tile_many is the same pair over an image set: a device table names each slot's image and tile.
#include "tile_geom.h"

namespace {

constexpr int TB_X = 64, TB_Y = 4;   // 64 pixels along x by 4 rows per workgroup

// One thread = one pixel of one window: C strided fp32 reads along x, one finished 32-byte channel group out.
template <typename T>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_gather_kernel(const esr_tile p, int th, int tw, int nx, int ntiles) {
  constexpr int CPG = DT<T>::CPG;
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= tw || row >= th) return;
  const int s = blockIdx.z / p.B, b = blockIdx.z - s * p.B;
  const int t = p.t_begin + s < ntiles ? p.t_begin + s : ntiles - 1;   // a tail pass repeats the last tile
  const TileAxis ay = tile_axis(p.H, p.tile, p.pad, th, t / nx), ax = tile_axis(p.W, p.tile, p.pad, tw, t % nx);
  const int64_t plane = (int64_t)p.H * p.W;
  const float* const src = p.nchw + (int64_t)b * p.C * plane + (int64_t)(ay.w0 + row) * p.W + ax.w0 + col;
  alignas(16) T v[CPG];
#pragma unroll
  for (int e = 0; e < CPG; ++e) v[e] = (T)((e < 8 && e < p.C) ? src[e * plane] : 0.f);
  char* const dst = (char*)p.g32.ptr + (int64_t)blockIdx.z * p.g32.batch_stride + ((int64_t)(row + 1) * p.g32.wp + col + 1) * 32;
  ((u32x4*)dst)[0] = ((const u32x4*)v)[0];
  ((u32x4*)dst)[1] = ((const u32x4*)v)[1];
}

// One thread = four HR pixels along x (one LR column) of one HR row of a tile's owned rectangle, all C channels: 16-byte
// loads and stores (every HR offset and row pitch is a multiple of four floats).  p.H, p.W are the HR image.
__global__ __launch_bounds__(TB_X * TB_Y) void tile_stitch_kernel(const esr_tile p, int th, int tw, int nx, int ntiles) {
  const int s = blockIdx.z / p.B, b = blockIdx.z - s * p.B;
  const int t = p.t_begin + s;
  if (t >= ntiles) return;                          // a tail pass: the repeated windows are not written
  const TileAxis ay = tile_axis(p.H >> 2, p.tile, p.pad, th, t / nx), ax = tile_axis(p.W >> 2, p.tile, p.pad, tw, t % nx);
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= ax.on || row >= 4 * ay.on) return;
  const int64_t src_plane = (int64_t)4 * th * tw, dst_plane = (int64_t)p.H * (p.W >> 2);   // in 16-byte units
  const f32x4* const src = (const f32x4*)p.slots_nchw + (int64_t)blockIdx.z * p.C * src_plane +
                           (int64_t)(4 * (ay.o0 - ay.w0) + row) * tw + (ax.o0 - ax.w0) + col;
  f32x4* const dst = (f32x4*)p.nchw + (int64_t)b * p.C * dst_plane + (int64_t)(4 * ay.o0 + row) * (p.W >> 2) + ax.o0 + col;
  for (int c = 0; c < p.C; ++c) dst[c * dst_plane] = src[c * src_plane];
}

// The table-driven pair (esr_tile_many): blockIdx.z is the slot, and the slot's item — one 24-byte table entry per thread,
// the same for a whole workgroup — names the image and the tile; everything else is the arithmetic of the kernels above.
static_assert(sizeof(esr_tile_item) == 24, "esr_tile_item is a 24-byte table entry");

template <typename T>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_many_gather_kernel(const esr_tile_many p) {
  constexpr int CPG = DT<T>::CPG;
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= p.tw || row >= p.th) return;
  const esr_tile_item it = p.items[blockIdx.z];     // a filler slot is filled like any other
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, p.th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, p.tw, it.t % nx);
  const int64_t plane = (int64_t)it.H * it.W;
  const float* const src = it.nchw + (int64_t)(ay.w0 + row) * it.W + ax.w0 + col;
  alignas(16) T v[CPG];
#pragma unroll
  for (int e = 0; e < CPG; ++e) v[e] = (T)((e < 8 && e < p.C) ? src[e * plane] : 0.f);
  char* const dst = (char*)p.g32.ptr + (int64_t)blockIdx.z * p.g32.batch_stride + ((int64_t)(row + 1) * p.g32.wp + col + 1) * 32;
  ((u32x4*)dst)[0] = ((const u32x4*)v)[0];
  ((u32x4*)dst)[1] = ((const u32x4*)v)[1];
}

// it.H, it.W are the LR image: its HR rows are it.W 16-byte units long.
__global__ __launch_bounds__(TB_X * TB_Y) void tile_many_stitch_kernel(const esr_tile_many p) {
  const esr_tile_item it = p.items[blockIdx.z];
  if (!it.live) return;                             // a filler slot: neither read nor written
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, p.th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, p.tw, it.t % nx);
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= ax.on || row >= 4 * ay.on) return;
  const int64_t src_plane = (int64_t)4 * p.th * p.tw, dst_plane = (int64_t)4 * it.H * it.W;   // in 16-byte units
  const f32x4* const src = (const f32x4*)p.slots_nchw + (int64_t)blockIdx.z * p.C * src_plane +
                           (int64_t)(4 * (ay.o0 - ay.w0) + row) * p.tw + (ax.o0 - ax.w0) + col;
  f32x4* const dst = (f32x4*)it.nchw + (int64_t)(4 * ay.o0 + row) * it.W + ax.o0 + col;
  for (int c = 0; c < p.C; ++c) dst[c * dst_plane] = src[c * src_plane];
}

}  // namespace

extern "C" int esr_tile_op(const esr_tile* p, esr_stream_t stream) {
  if (!p || !p->nchw || (p->to_g32 ? !p->g32.ptr : !p->slots_nchw) || p->B <= 0 || p->C <= 0 || p->H <= 0 || p->W <= 0 ||
      (p->dtype != ESR_F16 && p->dtype != ESR_F32)) {
    esr_set_error("esr_tile_op: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->tile < 1 || p->pad < 0 || (p->scale != 1 && p->scale != 4) || p->H % p->scale || p->W % p->scale) {
    esr_set_error("esr_tile_op: tile = %d (>= 1), pad = %d (>= 0), scale = %d (1 or 4, dividing H and W)", p->tile, p->pad, p->scale);
    return ESR_ERR_INVALID;
  }
  if (p->C > 8) {
    esr_set_error("esr_tile_op: C = %d does not fit one fp32 channel group", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->scale != (p->to_g32 ? 1 : 4)) {
    esr_set_error("esr_tile_op: the gather runs at scale 1 and the stitch at scale 4, got %d", p->scale);
    return ESR_ERR_UNSUPPORTED;
  }
  const int hl = p->H / p->scale, wl = p->W / p->scale;
  const int th = tile_window(hl, p->tile, p->pad), tw = tile_window(wl, p->tile, p->pad);
  const int ny = tile_count(hl, p->tile), nx = tile_count(wl, p->tile);
  const int64_t ntiles = (int64_t)ny * nx;
  if (ntiles > (1 << 30)) {
    esr_set_error("esr_tile_op: %lld tiles are more than one image may have", (long long)ntiles);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->t_begin < 0 || p->t_begin >= ntiles || p->t_count < 1) {
    esr_set_error("esr_tile_op: tiles [%d, %d + %d) of %lld", p->t_begin, p->t_begin, p->t_count, (long long)ntiles);
    return ESR_ERR_INVALID;
  }
  if ((int64_t)p->t_count * p->B > 65535) {
    esr_set_error("esr_tile_op: t_count * B = %lld slots are too many for one launch", (long long)p->t_count * p->B);
    return ESR_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(TB_X * TB_Y);
  const unsigned slots = (unsigned)(p->t_count * p->B);
  if (p->to_g32) {
    if (p->g32.wp < tw + 2 || p->g32.ngroups < 1) {
      esr_set_error("esr_tile_op: the G32 view (wp = %d) is narrower than the %d x %d window", p->g32.wp, th, tw);
      return ESR_ERR_INVALID;
    }
    const dim3 grid((tw + TB_X - 1) / TB_X, (th + TB_Y - 1) / TB_Y, slots);
    if (grid.y > 65535) {
      esr_set_error("esr_tile_op: a window of %d rows is too tall for one launch", th);
      return ESR_ERR_UNSUPPORTED;
    }
    if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_gather_kernel<_Float16>, grid, block, 0, st, *p, th, tw, nx, (int)ntiles);
    else hipLaunchKernelGGL(tile_gather_kernel<float>, grid, block, 0, st, *p, th, tw, nx, (int)ntiles);
  } else {
    if (((uintptr_t)p->nchw | (uintptr_t)p->slots_nchw) & 15) {
      esr_set_error("esr_tile_op: the stitch needs 16-byte aligned nchw and slots_nchw");
      return ESR_ERR_INVALID;
    }
    const int ow = p->tile < wl ? p->tile : wl, oh = p->tile < hl ? p->tile : hl;   // the largest owned rectangle
    const dim3 grid((ow + TB_X - 1) / TB_X, oh, slots);                               // 4 oh HR rows, TB_Y per workgroup
    if (grid.y > 65535) {
      esr_set_error("esr_tile_op: tiles of %d rows are too tall for one launch", oh);
      return ESR_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(tile_stitch_kernel, grid, block, 0, st, *p, th, tw, nx, (int)ntiles);
  }
  return esr_check_launch("tile_kernel");
}

// Per-item fields (image pointer, H, W, t, live) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_many_op(const esr_tile_many* p, esr_stream_t stream) {
  if (!p || !p->items || (p->to_g32 ? !p->g32.ptr : !p->slots_nchw) || p->C <= 0 || p->th <= 0 || p->tw <= 0 ||
      (p->dtype != ESR_F16 && p->dtype != ESR_F32)) {
    esr_set_error("esr_tile_many_op: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->tile < 1 || p->pad < 0 || (p->scale != 1 && p->scale != 4)) {
    esr_set_error("esr_tile_many_op: tile = %d (>= 1), pad = %d (>= 0), scale = %d (1 or 4)", p->tile, p->pad, p->scale);
    return ESR_ERR_INVALID;
  }
  if (p->C > 8) {
    esr_set_error("esr_tile_many_op: C = %d does not fit one fp32 channel group", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->scale != (p->to_g32 ? 1 : 4)) {
    esr_set_error("esr_tile_many_op: the gather runs at scale 1 and the stitch at scale 4, got %d", p->scale);
    return ESR_ERR_UNSUPPORTED;
  }
  const int64_t win = (int64_t)p->tile + 2 * (int64_t)p->pad;
  if (p->th > win || p->tw > win) {
    esr_set_error("esr_tile_many_op: a %d x %d window is larger than tile + 2 pad = %lld", p->th, p->tw, (long long)win);
    return ESR_ERR_INVALID;
  }
  if (p->n_slots < 1) {
    esr_set_error("esr_tile_many_op: n_slots = %d (>= 1)", p->n_slots);
    return ESR_ERR_INVALID;
  }
  if (p->n_slots > 65535) {
    esr_set_error("esr_tile_many_op: n_slots = %d slots are too many for one launch", p->n_slots);
    return ESR_ERR_UNSUPPORTED;
  }
  if ((p->th + TB_Y - 1) / TB_Y > 65535) {
    esr_set_error("esr_tile_many_op: a window of %d rows is too tall for one launch", p->th);
    return ESR_ERR_UNSUPPORTED;
  }
  if ((uintptr_t)p->items & 7) {
    esr_set_error("esr_tile_many_op: the item table needs 8-byte alignment");
    return ESR_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(TB_X * TB_Y);
  if (p->to_g32) {
    if (p->g32.wp < p->tw + 2 || p->g32.ngroups < 1) {
      esr_set_error("esr_tile_many_op: the G32 view (wp = %d) is narrower than the %d x %d window", p->g32.wp, p->th, p->tw);
      return ESR_ERR_INVALID;
    }
    const dim3 grid((p->tw + TB_X - 1) / TB_X, (p->th + TB_Y - 1) / TB_Y, (unsigned)p->n_slots);
    if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_many_gather_kernel<_Float16>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(tile_many_gather_kernel<float>, grid, block, 0, st, *p);
  } else {
    if ((uintptr_t)p->slots_nchw & 15) {
      esr_set_error("esr_tile_many_op: the stitch needs 16-byte aligned slots_nchw (and images)");
      return ESR_ERR_INVALID;
    }
    // the largest owned rectangle of any image with this window: min(tile, H) = min(tile, th), and alike along x
    const int ow = p->tile < p->tw ? p->tile : p->tw, oh = p->tile < p->th ? p->tile : p->th;
    const dim3 grid((ow + TB_X - 1) / TB_X, oh, (unsigned)p->n_slots);                // 4 oh HR rows, TB_Y per workgroup
    if (grid.y > 65535) {
      esr_set_error("esr_tile_many_op: tiles of %d rows are too tall for one launch", oh);
      return ESR_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(tile_many_stitch_kernel, grid, block, 0, st, *p);
  }
  return esr_check_launch("tile_many_kernel");
}
