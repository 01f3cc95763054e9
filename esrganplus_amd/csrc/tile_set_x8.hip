// tile_set_x8.hip — the two ends of the x8 self-ensemble over an image set (esr_tile_set_x8): tile_x8.hip's pair made
// table-driven like tile_io.hip's esr_tile_many, with the outside format as a field.  gather-import = the window of every
// table entry, read once from its fp32 NCHW or uint8 HWC image -> its flip / transpose copies as G32 slots;
// stitch-reduce = the slots' fp32 NCHW outputs -> inverse transforms summed in k order -> the owned rectangle of every
// live window in the fp32 NCHW or uint8 HWC result of its image.  Index maps and the accumulator protocol:
// include/esrgan_hip.h and tile_set_x8_index.h; the geometry is tile_geom.h's.  Plain loads, stores and VALU.
#include "tile_geom.h"
#include "tile_set_x8_index.h"

namespace {

static_assert(sizeof(esr_tile_item) == 24 && sizeof(esr_tile_img_item) == 24, "one 24-byte table entry per window");

// tile_img.hip's quant8_unit
__device__ __forceinline__ uint32_t quant8_unit(float v) { return (uint32_t)(int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

// tile_x8_gather_kernel with the window named by the table (blockIdx.z = the window; the item is the same for the whole
// workgroup) and, for IMG, tile_img_gather_kernel's read: C bytes per pixel, one true division per channel, the bgr swap.
// A filler window is gathered like any other.
template <typename T, bool IMG>
__global__ __launch_bounds__(1024) void tile_set_x8_gather_kernel(const esr_tile_set_x8 p) {
  constexpr int CPG = DT<T>::CPG;
  __shared__ u32x4 tile[SX8_TILE][SX8_TILE + 1][2];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x0 = blockIdx.x * SX8_TILE, y0 = blockIdx.y * SX8_TILE;
  const int w = blockIdx.z, th = p.th, tw = p.tw;
  const esr_tile_item it = p.items[w];
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, tw, it.t % nx);
  u32x4 own[2];                       // this thread's window pixel (y0 + ly, x0 + lx) as a finished 32-byte channel group
  {
    const int sy = y0 + ly, sx = x0 + lx;
    const bool in = sy < th && sx < tw;
    const int64_t pix = (int64_t)(ay.w0 + (in ? sy : 0)) * it.W + ax.w0 + (in ? sx : 0);
    alignas(16) T v[CPG];
    if constexpr (IMG) {
      const uint8_t* const src = (const uint8_t*)it.nchw + pix * p.C;
      const bool swap = p.bgr && p.C == 3;
#pragma unroll
      for (int e = 0; e < CPG; ++e) v[e] = (T)((in && e < 3 && e < p.C) ? __fdiv_rn((float)src[swap ? 2 - e : e], 255.0f) : 0.f);
    } else {
      const int64_t plane = (int64_t)it.H * it.W;
      const float* const src = it.nchw + pix;
#pragma unroll
      for (int e = 0; e < CPG; ++e) v[e] = (T)((in && e < 8 && e < p.C) ? src[e * plane] : 0.f);
    }
    own[0] = ((const u32x4*)v)[0];
    own[1] = ((const u32x4*)v)[1];
    tile[ly][lx][0] = own[0];
    tile[ly][lx][1] = own[1];
  }
  __syncthreads();
  for (int i = 0; i < p.k_count; ++i) {
    const int k = p.k_begin + i;
    const bool tr = (k & 4) != 0;
    // source pixel of this thread: consecutive lanes walk the slot's x
    const int ty = tr ? lx : ly, tx = tr ? ly : lx;
    const int sy = y0 + ty, sx = x0 + tx;
    if (sy >= th || sx >= tw) continue;
    const SX8Pos at = sx8_gather_pos(k, th, tw, sy, sx);
    char* const dst = (char*)p.g32.ptr + sx8_entry(i, p.n_windows, w) * p.g32.batch_stride +
                      ((int64_t)(at.row + 1) * p.g32.wp + at.col + 1) * 32;
    // straight slots: the thread's own pixel from registers; transposed slots: the mirrored LDS entry
    ((u32x4*)dst)[0] = tr ? tile[ty][tx][0] : own[0];
    ((u32x4*)dst)[1] = tr ? tile[ty][tx][1] : own[1];
  }
}

// tile_x8_reduce_kernel over the table: one thread = one HR pixel of a live window's owned rectangle, all channels.
// NC = 0: the fp32 NCHW result of the item carries the partial sum (p.C channels).  NC = 1, 3: the uint8 HWC result
// cannot; the partial sum lives in p.acc, and the last range quantises and sends the workgroup's rows out through the
// LDS as aligned dwords.  it.H, it.W are the LR image; every lane is bounded by the owned rectangle.
template <int NC>
__global__ __launch_bounds__(1024) void tile_set_x8_reduce_kernel(const esr_tile_set_x8 p) {
  __shared__ u32x4 tile[SX8_TILE][SX8_TILE + 1][2];
  const int w = blockIdx.z, th = p.th, tw = p.tw;
  const esr_tile_item it = p.items[w];
  if (!it.live) return;                             // a filler window: neither read nor written
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, tw, it.t % nx);
  const int oh = 4 * ay.on, ow = 4 * ax.on;         // the owned rectangle, HR pixels
  const int x0 = blockIdx.x * SX8_TILE, y0 = blockIdx.y * SX8_TILE;
  if (x0 >= ow || y0 >= oh) return;                 // whole workgroup outside this window's rectangle
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int hh = 4 * th, hw = 4 * tw;               // the window's output
  const int wy = 4 * (ay.o0 - ay.w0), wx = 4 * (ax.o0 - ax.w0);   // the owned rectangle inside it
  const bool own = y0 + ly < oh && x0 + lx < ow;
  const int C = NC ? NC : p.C;
  const int64_t src_plane = (int64_t)hh * hw;
  // where the partial sum of this pixel lives, and the pitch of its channels
  const int64_t part_plane = NC ? src_plane : (int64_t)16 * it.H * it.W;
  float* part = nullptr;
  if (own) {
    if constexpr (NC != 0) part = p.acc ? p.acc + sx8_acc_offset(w, 0, C, hh, hw, wy + y0 + ly, wx + x0 + lx) : nullptr;
    else part = it.nchw + (int64_t)(4 * ay.o0 + y0 + ly) * (4 * it.W) + 4 * ax.o0 + x0 + lx;
  }
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = (own && p.accumulate && e < C) ? part[e * part_plane] : 0.f;
  for (int i = 0; i < p.k_count; ++i) {
    const int k = p.k_begin + i;
    const float* const slot = p.slots_nchw + sx8_entry(i, p.n_windows, w) * C * src_plane;
    alignas(16) float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!(k & 4)) {
      if (own) {
        const float* const src = slot + sx8_reduce_src(k, hh, hw, wy + y0 + ly, wx + x0 + lx);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < C ? src[e * src_plane] : 0.f;
      }
    } else {
      // this thread fetches the value of owned pixel (y0 + lx, x0 + ly): consecutive lanes walk the slot's x
      const int oy = y0 + lx, ox = x0 + ly;
      __syncthreads();                       // the previous turn's reads are done
      if (oy < oh && ox < ow) {
        const float* const src = slot + sx8_reduce_src(k, hh, hw, wy + oy, wx + ox);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < C ? src[e * src_plane] : 0.f;
        tile[lx][ly][0] = ((const u32x4*)v)[0];
        tile[lx][ly][1] = ((const u32x4*)v)[1];
      }
      __syncthreads();
      if (own) {
        ((u32x4*)v)[0] = tile[ly][lx][0];
        ((u32x4*)v)[1] = tile[ly][lx][1];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (i == 0 && !p.accumulate) ? v[e] : __fadd_rn(acc[e], v[e]);
  }
  if constexpr (NC == 0) {
    if (!own) return;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < C) part[e * part_plane] = __fmul_rn(acc[e], p.mean_scale);
  } else {
    if (!sx8_last_range(p.k_begin, p.k_count)) {
      if (!own) return;
#pragma unroll
      for (int e = 0; e < NC; ++e) part[e * part_plane] = __fmul_rn(acc[e], p.mean_scale);
      return;
    }
    // the last range: the workgroup's 32 rows of 32 pixels as bytes in the LDS, then one aligned dword per lane
    uint8_t* const bytes = (uint8_t*)&tile[0][0][0];
    __syncthreads();                         // the last turn's reads are done
    if (own) {
      const bool swap = p.bgr && NC == 3;
#pragma unroll
      for (int e = 0; e < NC; ++e) bytes[(ly * SX8_TILE + lx) * NC + (swap ? 2 - e : e)] = (uint8_t)quant8_unit(__fmul_rn(acc[e], p.mean_scale));
    }
    __syncthreads();
    const int n = ow - x0 < SX8_TILE ? ow - x0 : SX8_TILE;      // owned pixels of these rows: a multiple of 4
    if (y0 + ly < oh && lx < sx8_row_dwords(n, NC)) {
      uint8_t* const row = (uint8_t*)it.nchw + ((int64_t)(4 * ay.o0 + y0 + ly) * (4 * it.W) + 4 * ax.o0 + x0) * NC;
      ((uint32_t*)row)[lx] = ((const uint32_t*)bytes)[ly * (SX8_TILE * NC / 4) + lx];
    }
  }
}

}  // namespace

// Per-item fields (image pointer, H, W, t, live) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_set_x8_op(const esr_tile_set_x8* p, esr_stream_t stream) {
  if (!p || !p->items || (p->to_g32 ? !p->g32.ptr : !p->slots_nchw) || p->C <= 0 || p->th <= 0 || p->tw <= 0 ||
      (p->dtype != ESR_F16 && p->dtype != ESR_F32)) {
    esr_set_error("esr_tile_set_x8_op: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->tile < 1 || p->pad < 0 || (p->scale != 1 && p->scale != 4)) {
    esr_set_error("esr_tile_set_x8_op: tile = %d (>= 1), pad = %d (>= 0), scale = %d (1 or 4)", p->tile, p->pad, p->scale);
    return ESR_ERR_INVALID;
  }
  if (p->scale != (p->to_g32 ? 1 : 4)) {
    esr_set_error("esr_tile_set_x8_op: the gather runs at scale 1 and the stitch at scale 4, got %d", p->scale);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->C > 8) {
    esr_set_error("esr_tile_set_x8_op: C = %d does not fit one fp32 channel group", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->img && p->C != 1 && p->C != 3) {
    esr_set_error("esr_tile_set_x8_op: C = %d: 8-bit images have 1 or 3 channels", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  const int range = sx8_range_error(p->k_begin, p->k_count, p->th, p->tw);
  if (range == 1) {
    esr_set_error("esr_tile_set_x8_op: slots [%d, %d + %d) of 8", p->k_begin, p->k_begin, p->k_count);
    return ESR_ERR_INVALID;
  }
  if (range == 2) {
    esr_set_error("esr_tile_set_x8_op: a range across k = 4 needs square windows, got %d x %d (the transposed slots are %d x %d)",
                  p->th, p->tw, p->tw, p->th);
    return ESR_ERR_INVALID;
  }
  const int64_t win = (int64_t)p->tile + 2 * (int64_t)p->pad;
  if (p->th > win || p->tw > win) {
    esr_set_error("esr_tile_set_x8_op: a %d x %d window is larger than tile + 2 pad = %lld", p->th, p->tw, (long long)win);
    return ESR_ERR_INVALID;
  }
  if (p->n_windows < 1) {
    esr_set_error("esr_tile_set_x8_op: n_windows = %d (>= 1)", p->n_windows);
    return ESR_ERR_INVALID;
  }
  if ((int64_t)p->k_count * p->n_windows > 65535) {
    esr_set_error("esr_tile_set_x8_op: k_count * n_windows = %lld slots are too many for one launch", (long long)p->k_count * p->n_windows);
    return ESR_ERR_UNSUPPORTED;
  }
  if ((uintptr_t)p->items & 7) {
    esr_set_error("esr_tile_set_x8_op: the item table needs 8-byte alignment");
    return ESR_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(SX8_TILE * SX8_TILE);
  const bool turned = p->k_begin + p->k_count > 4;
  if (p->to_g32) {
    if (p->g32.wp < (turned ? p->th : p->tw) + 2 || p->g32.ngroups < 1) {
      esr_set_error("esr_tile_set_x8_op: the G32 view (wp = %d) is narrower than the %d x %d window's slots", p->g32.wp, p->th, p->tw);
      return ESR_ERR_INVALID;
    }
    const dim3 grid((p->tw + SX8_TILE - 1) / SX8_TILE, (p->th + SX8_TILE - 1) / SX8_TILE, (unsigned)p->n_windows);
    if (grid.y > 65535) {
      esr_set_error("esr_tile_set_x8_op: a window of %d rows is too tall for one launch", p->th);
      return ESR_ERR_UNSUPPORTED;
    }
    if (p->img) {
      if (p->dtype == ESR_F16) hipLaunchKernelGGL((tile_set_x8_gather_kernel<_Float16, true>), grid, block, 0, st, *p);
      else hipLaunchKernelGGL((tile_set_x8_gather_kernel<float, true>), grid, block, 0, st, *p);
    } else {
      if (p->dtype == ESR_F16) hipLaunchKernelGGL((tile_set_x8_gather_kernel<_Float16, false>), grid, block, 0, st, *p);
      else hipLaunchKernelGGL((tile_set_x8_gather_kernel<float, false>), grid, block, 0, st, *p);
    }
  } else {
    if ((uintptr_t)p->slots_nchw & 15) {
      esr_set_error("esr_tile_set_x8_op: the stitch needs 16-byte aligned slots_nchw (and images)");
      return ESR_ERR_INVALID;
    }
    if (sx8_acc_needed(p->img, p->accumulate, p->k_begin, p->k_count)) {
      if (!p->acc) {
        esr_set_error("esr_tile_set_x8_op: slots [%d, %d + %d) of an 8-bit result need acc, the partial sums between the ranges",
                      p->k_begin, p->k_begin, p->k_count);
        return ESR_ERR_INVALID;
      }
      if ((uintptr_t)p->acc & 15) {
        esr_set_error("esr_tile_set_x8_op: acc needs 16-byte alignment");
        return ESR_ERR_INVALID;
      }
    }
    // the largest owned rectangle of any image with this window: min(tile, H) = min(tile, th), and alike along x
    const int ow = p->tile < p->tw ? p->tile : p->tw, oh = p->tile < p->th ? p->tile : p->th;
    const dim3 grid((4 * ow + SX8_TILE - 1) / SX8_TILE, (4 * oh + SX8_TILE - 1) / SX8_TILE, (unsigned)p->n_windows);
    if (grid.y > 65535) {
      esr_set_error("esr_tile_set_x8_op: tiles of %d rows are too tall for one launch", oh);
      return ESR_ERR_UNSUPPORTED;
    }
    if (!p->img) hipLaunchKernelGGL(tile_set_x8_reduce_kernel<0>, grid, block, 0, st, *p);
    else if (p->C == 1) hipLaunchKernelGGL(tile_set_x8_reduce_kernel<1>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(tile_set_x8_reduce_kernel<3>, grid, block, 0, st, *p);
  }
  return esr_check_launch("tile_set_x8_kernel");
}
