// tile_img.hip — esr_tile_many's two ends with 8-bit images on the outside (esr_tile_img): gather = fixed-size windows of
// uint8 HWC images -> / 255 -> G32 slots, stitch = the owned rectangle of every window's fp32 NCHW output -> clamp, x 255,
// round -> the uint8 HWC result of its image.  Index maps and the alignment contract: include/esrgan_hip.h (esr_tile_img);
// the geometry is tile_io.hip's.  esr_tile_hr is the same pair with a gather that makes the LR window itself, out of the
// 8-bit HR image through the whole image's bicubic tables; its stitch is esr_tile_img's kernel.  Plain loads, stores and VALU.
#include <cstddef>
#include "tile_geom.h"
#include "resample_taps.h"

namespace {

constexpr int TB_X = 64, TB_Y = 4;   // 64 pixels along x by 4 rows per workgroup, as tile_io.hip

static_assert(sizeof(esr_tile_img_item) == 24 && sizeof(esr_tile_img_item) == sizeof(esr_tile_item),
              "esr_tile_img_item has esr_tile_item's 24-byte layout");
static_assert(sizeof(esr_tile_hr_item) == 24 && offsetof(esr_tile_hr_item, H) == offsetof(esr_tile_img_item, H) &&
              offsetof(esr_tile_hr_item, live) == offsetof(esr_tile_img_item, live), "esr_tile_hr_item has that layout too");
static_assert(sizeof(esr_tile_hr) == sizeof(esr_tile_img) && offsetof(esr_tile_hr, items) == offsetof(esr_tile_img, items) &&
              offsetof(esr_tile_hr, g32) == offsetof(esr_tile_img, g32) && offsetof(esr_tile_hr, bgr) == offsetof(esr_tile_img, bgr),
              "esr_tile_hr has esr_tile_img's fields: its stitch is esr_tile_img's");
static_assert(sizeof(esr_tile_hr_desc) == 64, "one 64-byte descriptor per image");

constexpr int HR_T = 16;                     // one workgroup = one 16 x 16 LR tile of one slot's window, one pixel per thread
constexpr int HR_SPAN = ESR_TILE_HR_SPAN;    // source columns of an LDS row: 15 * 4 + 17 taps at x4, odd
static_assert(HR_SPAN >= (HR_T - 1) * 4 + 17, "the span of 16 consecutive LR columns of a x4 table");

// metrics.hip's quant8(v, 0, 1): the (v - 0) / (1 - 0) of the general form changes no bit
__device__ __forceinline__ uint32_t quant8_unit(float v) { return (uint32_t)(int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

// One thread = one pixel of one window: C bytes in, one true division per channel, one finished 32-byte channel group out.
template <typename T>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_img_gather_kernel(const esr_tile_img p) {
  constexpr int CPG = DT<T>::CPG;
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= p.tw || row >= p.th) return;
  const esr_tile_img_item it = p.items[blockIdx.z];   // a filler slot is filled like any other
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, p.th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, p.tw, it.t % nx);
  const uint8_t* const src = it.hwc + ((int64_t)(ay.w0 + row) * it.W + ax.w0 + col) * p.C;
  const bool swap = p.bgr && p.C == 3;
  alignas(16) T v[CPG];
#pragma unroll
  for (int e = 0; e < CPG; ++e) v[e] = (T)((e < 3 && e < p.C) ? __fdiv_rn((float)src[swap ? 2 - e : e], 255.0f) : 0.f);
  char* const dst = (char*)p.g32.ptr + (int64_t)blockIdx.z * p.g32.batch_stride + ((int64_t)(row + 1) * p.g32.wp + col + 1) * 32;
  ((u32x4*)dst)[0] = ((const u32x4*)v)[0];
  ((u32x4*)dst)[1] = ((const u32x4*)v)[1];
}

// One workgroup = one 16 x 16 LR tile of one window, resampled from the 8-bit HR image of its slot: the span of source
// columns its 16 LR columns touch, the H pass of its rows over that span into the LDS (3 x 16 x 77 floats = 14 784 bytes),
// the W pass out of it, one finished 32-byte channel group per thread.  The loops are batch_assemble.hip's
// (resample_taps.h); rows and columns beyond the window are clamped into the image, computed by nobody or not written.
template <typename T>
__global__ __launch_bounds__(HR_T * HR_T) void tile_hr_gather_kernel(const esr_tile_hr p) {
  constexpr int CPG = DT<T>::CPG;
  __shared__ float rows[3 * HR_T * HR_SPAN];
  __shared__ int span[2 * HR_T];
  const esr_tile_hr_item it = p.items[blockIdx.z];      // a filler slot is filled like any other
  const esr_tile_hr_desc d = *(const esr_tile_hr_desc*)it.ptr;
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, p.th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, p.tw, it.t % nx);
  const int a0 = blockIdx.y * HR_T, b0 = blockIdx.x * HR_T;
  const int lx = threadIdx.x % HR_T, ly = threadIdx.x / HR_T;
  const int s0 = p.bgr ? 2 : 0, sd = p.bgr ? -1 : 1;     // slot channel c reads byte s0 + sd c

  if (threadIdx.x < HR_T) {
    const int o = clampi(ax.w0 + b0 + (int)threadIdx.x, 0, it.W - 1);
    int lo, hi;
    resample_col_span(d.ix + (int64_t)o * d.taps_x, d.taps_x, d.hr_w, lo, hi);
    span[threadIdx.x] = lo;
    span[HR_T + threadIdx.x] = hi;
  }
  __syncthreads();
  int c_lo = span[0], c_hi = span[HR_T];
  for (int k = 1; k < HR_T; ++k) {
    c_lo = span[k] < c_lo ? span[k] : c_lo;
    c_hi = span[HR_T + k] > c_hi ? span[HR_T + k] : c_hi;
  }
  const int ncol = c_hi - c_lo + 1 < HR_SPAN ? c_hi - c_lo + 1 : HR_SPAN;
  const int nrow = p.th - a0 < HR_T ? p.th - a0 : HR_T;
  // H pass of the tile's rows on those columns
  for (int e = threadIdx.x; e < nrow * ncol; e += HR_T * HR_T) {
    const int r = e / ncol, xs = e - r * ncol;
    const int o = clampi(ay.w0 + a0 + r, 0, it.H - 1);
    const uint8_t* const col = d.hr + (int64_t)(c_lo + xs) * 3 + s0;
    float acc[3] = {0.f, 0.f, 0.f};
    resample_h_taps(d.wy + (int64_t)o * d.taps_y, d.iy + (int64_t)o * d.taps_y, d.taps_y, d.hr_h,
                    [&](int c, int sy) { return __fdiv_rn((float)col[(int64_t)sy * d.pitch * 3 + sd * c], 255.0f); }, acc);
#pragma unroll
    for (int c = 0; c < 3; ++c) rows[(c * HR_T + r) * HR_SPAN + xs] = acc[c];
  }
  __syncthreads();
  // W pass from the LDS
  const int row = a0 + ly, colx = b0 + lx;
  if (row >= p.th || colx >= p.tw) return;
  const int o = clampi(ax.w0 + colx, 0, it.W - 1);
  float acc[3] = {0.f, 0.f, 0.f};
  resample_w_taps(d.wx + (int64_t)o * d.taps_x, d.ix + (int64_t)o * d.taps_x, d.taps_x, d.hr_w, c_lo, HR_SPAN,
                  rows + ly * HR_SPAN, HR_T * HR_SPAN, acc);
  alignas(16) T v[CPG];
#pragma unroll
  for (int e = 0; e < CPG; ++e) v[e] = (T)(e < 3 ? acc[e < 3 ? e : 0] : 0.f);
  char* const dst = (char*)p.g32.ptr + (int64_t)blockIdx.z * p.g32.batch_stride + ((int64_t)(row + 1) * p.g32.wp + colx + 1) * 32;
  ((u32x4*)dst)[0] = ((const u32x4*)v)[0];
  ((u32x4*)dst)[1] = ((const u32x4*)v)[1];
}

// One thread = four HR pixels along x (one LR column) of one HR row of a tile's owned rectangle: one 16-byte load per
// channel, NC aligned dwords out.  it.H, it.W are the LR image: its HR rows are 4 it.W pixels = it.W groups of NC dwords.
template <int NC>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_img_stitch_kernel(const esr_tile_img p) {
  const esr_tile_img_item it = p.items[blockIdx.z];
  if (!it.live) return;                             // a filler slot: neither read nor written
  const int nx = tile_count(it.W, p.tile);
  const TileAxis ay = tile_axis(it.H, p.tile, p.pad, p.th, it.t / nx), ax = tile_axis(it.W, p.tile, p.pad, p.tw, it.t % nx);
  const int col = blockIdx.x * TB_X + (threadIdx.x & (TB_X - 1)), row = blockIdx.y * TB_Y + threadIdx.x / TB_X;
  if (col >= ax.on || row >= 4 * ay.on) return;
  const int64_t src_plane = (int64_t)4 * p.th * p.tw;   // in 16-byte units
  const f32x4* const src = (const f32x4*)p.slots_nchw + (int64_t)blockIdx.z * NC * src_plane +
                           (int64_t)(4 * (ay.o0 - ay.w0) + row) * p.tw + (ax.o0 - ax.w0) + col;
  uint32_t q[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const f32x4 v = src[c * src_plane];
    q[c][0] = quant8_unit(v.x); q[c][1] = quant8_unit(v.y); q[c][2] = quant8_unit(v.z); q[c][3] = quant8_unit(v.w);
  }
  uint32_t* const dst = (uint32_t*)it.hwc + ((int64_t)(4 * ay.o0 + row) * it.W + ax.o0 + col) * NC;
  if constexpr (NC == 1) {
    dst[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[0][3] << 24;
  } else {
    if (p.bgr) {                                    // q[0] / q[2]: the channels at bytes 0 / 2 of a pixel
#pragma unroll
      for (int j = 0; j < 4; ++j) { const uint32_t r = q[0][j]; q[0][j] = q[2][j]; q[2][j] = r; }
    }
    dst[0] = q[0][0] | q[1][0] << 8 | q[2][0] << 16 | q[0][1] << 24;
    dst[1] = q[1][1] | q[2][1] << 8 | q[0][2] << 16 | q[1][2] << 24;
    dst[2] = q[2][2] | q[0][3] << 8 | q[1][3] << 16 | q[2][3] << 24;
  }
}

// The two entries: esr_tile_hr has esr_tile_img's fields, `hr` picks its gather; `who` names the entry in the messages.
int tile_img_run(const esr_tile_img* p, esr_stream_t stream, const char* who, bool hr) {
  if (!p || !p->items || (p->to_g32 ? !p->g32.ptr : !p->slots_nchw) || p->C <= 0 || p->th <= 0 || p->tw <= 0 ||
      (p->dtype != ESR_F16 && p->dtype != ESR_F32)) {
    esr_set_error("%s: invalid arguments", who);
    return ESR_ERR_INVALID;
  }
  if (p->tile < 1 || p->pad < 0 || (p->scale != 1 && p->scale != 4)) {
    esr_set_error("%s: tile = %d (>= 1), pad = %d (>= 0), scale = %d (1 or 4)", who, p->tile, p->pad, p->scale);
    return ESR_ERR_INVALID;
  }
  if (hr ? p->C != 3 : (p->C != 1 && p->C != 3)) {
    esr_set_error("%s: C = %d: 8-bit images have %s channels", who, p->C, hr ? "3" : "1 or 3");
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->scale != (p->to_g32 ? 1 : 4)) {
    esr_set_error("%s: the gather runs at scale 1 and the stitch at scale 4, got %d", who, p->scale);
    return ESR_ERR_UNSUPPORTED;
  }
  const int64_t win = (int64_t)p->tile + 2 * (int64_t)p->pad;
  if (p->th > win || p->tw > win) {
    esr_set_error("%s: a %d x %d window is larger than tile + 2 pad = %lld", who, p->th, p->tw, (long long)win);
    return ESR_ERR_INVALID;
  }
  if (p->n_slots < 1) {
    esr_set_error("%s: n_slots = %d (>= 1)", who, p->n_slots);
    return ESR_ERR_INVALID;
  }
  if (p->n_slots > 65535) {
    esr_set_error("%s: n_slots = %d slots are too many for one launch", who, p->n_slots);
    return ESR_ERR_UNSUPPORTED;
  }
  if ((p->th + TB_Y - 1) / TB_Y > 65535) {
    esr_set_error("%s: a window of %d rows is too tall for one launch", who, p->th);
    return ESR_ERR_UNSUPPORTED;
  }
  if ((uintptr_t)p->items & 7) {
    esr_set_error("%s: the item table needs 8-byte alignment", who);
    return ESR_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(TB_X * TB_Y);
  if (p->to_g32) {
    if (p->g32.wp < p->tw + 2 || p->g32.ngroups < 1) {
      esr_set_error("%s: the G32 view (wp = %d) is narrower than the %d x %d window", who, p->g32.wp, p->th, p->tw);
      return ESR_ERR_INVALID;
    }
    if (hr) {
      const esr_tile_hr q = *(const esr_tile_hr*)p;
      const dim3 grid((p->tw + HR_T - 1) / HR_T, (p->th + HR_T - 1) / HR_T, (unsigned)p->n_slots);   // y <= 65535: checked above
      if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_hr_gather_kernel<_Float16>, grid, dim3(HR_T * HR_T), 0, st, q);
      else hipLaunchKernelGGL(tile_hr_gather_kernel<float>, grid, dim3(HR_T * HR_T), 0, st, q);
      return esr_check_launch("tile_hr_gather_kernel");
    }
    const dim3 grid((p->tw + TB_X - 1) / TB_X, (p->th + TB_Y - 1) / TB_Y, (unsigned)p->n_slots);
    if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_img_gather_kernel<_Float16>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(tile_img_gather_kernel<float>, grid, block, 0, st, *p);
  } else {
    if ((uintptr_t)p->slots_nchw & 15) {
      esr_set_error("%s: the stitch needs 16-byte aligned slots_nchw (and 4-byte aligned images)", who);
      return ESR_ERR_INVALID;
    }
    // the largest owned rectangle of any image with this window: min(tile, H) = min(tile, th), and alike along x
    const int ow = p->tile < p->tw ? p->tile : p->tw, oh = p->tile < p->th ? p->tile : p->th;
    const dim3 grid((ow + TB_X - 1) / TB_X, oh, (unsigned)p->n_slots);                // 4 oh HR rows, TB_Y per workgroup
    if (grid.y > 65535) {
      esr_set_error("%s: tiles of %d rows are too tall for one launch", who, oh);
      return ESR_ERR_UNSUPPORTED;
    }
    if (p->C == 1) hipLaunchKernelGGL(tile_img_stitch_kernel<1>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(tile_img_stitch_kernel<3>, grid, block, 0, st, *p);
  }
  return esr_check_launch("tile_img_kernel");
}

}  // namespace

// Per-item fields (image pointer, H, W, t, live) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_img_op(const esr_tile_img* p, esr_stream_t stream) {
  return tile_img_run(p, stream, "esr_tile_img_op", false);
}

// Items and descriptors (pointers, sizes, tables) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_hr_op(const esr_tile_hr* p, esr_stream_t stream) {
  return tile_img_run((const esr_tile_img*)p, stream, "esr_tile_hr_op", true);
}
