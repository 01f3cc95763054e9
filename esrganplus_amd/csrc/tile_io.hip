// tile_io.hip — the plain ends of tiled inference: gather = fixed-size windows of an image -> G32 slots, stitch = the owned
// rectangle of every window's fp32 NCHW output -> the result image.  Four ops share the bodies of tile_ends.h:
//   esr_tile       windows named per image, fp32 NCHW outside
//   esr_tile_many  windows named by a device table (an image set), fp32 NCHW outside
//   esr_tile_img   the table, uint8 HWC outside: / 255 in, clamp, x 255, round out
//   esr_tile_hr    esr_tile_img with a gather that makes the LR window itself, out of the 8-bit HR image through the
//                  whole image's bicubic tables; its stitch is esr_tile_img's kernel
// Geometry and index maps: include/esrgan_hip.h and tile_geom.h.  Plain loads, stores and VALU.
#include "tile_checks.h"
#include "resample_taps.h"

namespace {

static_assert(sizeof(esr_tile_hr) == sizeof(esr_tile_img) && offsetof(esr_tile_hr, items) == offsetof(esr_tile_img, items) &&
              offsetof(esr_tile_hr, g32) == offsetof(esr_tile_img, g32) && offsetof(esr_tile_hr, bgr) == offsetof(esr_tile_img, bgr),
              "esr_tile_hr has esr_tile_img's fields: its stitch is esr_tile_img's");
static_assert(sizeof(esr_tile_hr_desc) == 64, "one 64-byte descriptor per image");

constexpr int HR_T = 16;                     // one workgroup = one 16 x 16 LR tile of one slot's window, one pixel per thread
constexpr int HR_SPAN = ESR_TILE_HR_SPAN;    // source columns of an LDS row: 15 * 4 + 17 taps at x4, odd
static_assert(HR_SPAN >= (HR_T - 1) * 4 + 17, "the span of 16 consecutive LR columns of a x4 table");

template <typename T>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_gather_kernel(const esr_tile p, int th, int tw, int nx, int ntiles) {
  plain_gather<T>(TILE_PER_IMAGE(p, th, tw, nx, ntiles), PxF32<8>{}, p.C, p.g32);
}
__global__ __launch_bounds__(TB_X * TB_Y) void tile_stitch_kernel(const esr_tile p, int th, int tw, int nx, int ntiles) {
  plain_stitch(TILE_PER_IMAGE(p, th, tw, nx, ntiles), p.C, p.slots_nchw);
}

template <typename T>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_many_gather_kernel(const esr_tile_many p) {
  plain_gather<T>(TILE_BY_TABLE(p), PxF32<8>{}, p.C, p.g32);
}
__global__ __launch_bounds__(TB_X * TB_Y) void tile_many_stitch_kernel(const esr_tile_many p) {
  plain_stitch(TILE_BY_TABLE(p), p.C, p.slots_nchw);
}

template <typename T>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_img_gather_kernel(const esr_tile_img p) {
  plain_gather<T>(TILE_BY_TABLE(p), PxU8{p.bgr}, p.C, p.g32);
}

// One workgroup = one 16 x 16 LR tile of one window, resampled from the 8-bit HR image of its slot: the span of source
// columns its 16 LR columns touch, the H pass of its rows over that span into the LDS (3 x 16 x 77 floats = 14 784 bytes),
// the W pass out of it, one finished 32-byte channel group per thread.  The loops are batch_assemble.hip's
// (resample_taps.h); rows and columns beyond the window are clamped into the image, computed by nobody or not written.
template <typename T>
__global__ __launch_bounds__(HR_T * HR_T) void tile_hr_gather_kernel(const esr_tile_hr p) {
  __shared__ float rows[3 * HR_T * HR_SPAN];
  __shared__ int span[2 * HR_T];
  const TileWin w = TileTable::gather(TILE_BY_TABLE(p), blockIdx.z);     // a filler slot is filled like any other
  const esr_tile_hr_desc d = *(const esr_tile_hr_desc*)w.img;
  const TileAxis ay = w.ay, ax = w.ax;
  const int a0 = blockIdx.y * HR_T, b0 = blockIdx.x * HR_T;
  const int lx = threadIdx.x % HR_T, ly = threadIdx.x / HR_T;
  const int s0 = p.bgr ? 2 : 0, sd = p.bgr ? -1 : 1;     // slot channel c reads byte s0 + sd c

  if (threadIdx.x < HR_T) {
    const int o = clampi(ax.w0 + b0 + (int)threadIdx.x, 0, w.W - 1);
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
    const int o = clampi(ay.w0 + a0 + r, 0, w.H - 1);
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
  const int o = clampi(ax.w0 + colx, 0, w.W - 1);
  float acc[3] = {0.f, 0.f, 0.f};
  resample_w_taps(d.wx + (int64_t)o * d.taps_x, d.ix + (int64_t)o * d.taps_x, d.taps_x, d.hr_w, c_lo, HR_SPAN,
                  rows + ly * HR_SPAN, HR_T * HR_SPAN, acc);
  u32x4 grp[2];
  make_group<T, 3>(grp, 3, [&](int e) { return acc[e]; });
  u32x4* const dst = g32_px(p.g32, blockIdx.z, row, colx);
  dst[0] = grp[0];
  dst[1] = grp[1];
}

// uint8 HWC out: one 16-byte load per channel, quantised, NC aligned dwords out.  The image's HR rows are 4 W pixels =
// W groups of NC dwords.
template <int NC>
__global__ __launch_bounds__(TB_X * TB_Y) void tile_img_stitch_kernel(const esr_tile_img p) {
  const TileTable r = TILE_BY_TABLE(p);
  const TileWin w = TileTable::stitch(r, blockIdx.z);
  if (!w.live) return;                              // a filler slot: neither read nor written
  const f32x4* src;
  int64_t src_plane, dst_unit;
  if (!stitch_lane(r, w, NC, p.slots_nchw, src, src_plane, dst_unit)) return;
  uint32_t q[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const f32x4 v = src[c * src_plane];
    q[c][0] = quant8_unit(v.x); q[c][1] = quant8_unit(v.y); q[c][2] = quant8_unit(v.z); q[c][3] = quant8_unit(v.w);
  }
  uint32_t* const dst = (uint32_t*)w.img + dst_unit * NC;
  if constexpr (NC == 1) {
    dst[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[0][3] << 24;
  } else {
    if (p.bgr) {                                    // q[0] / q[2]: the channels at bytes 0 / 2 of a pixel
#pragma unroll
      for (int j = 0; j < 4; ++j) { const uint32_t t = q[0][j]; q[0][j] = q[2][j]; q[2][j] = t; }
    }
    dst[0] = q[0][0] | q[1][0] << 8 | q[2][0] << 16 | q[0][1] << 24;
    dst[1] = q[1][1] | q[2][1] << 8 | q[0][2] << 16 | q[1][2] << 24;
    dst[2] = q[2][2] | q[0][3] << 8 | q[1][3] << 16 | q[2][3] << 24;
  }
}

// What the plain pair launches, once the op's own checks are through: th x tw the window, oh x ow the largest owned
// rectangle (LR pixels).  gather / stitch launch on (grid, block); gather may still refuse, and returns the status.
template <typename G, typename S>
int plain_launch(const char* who, int to_g32, const esr_g32& g32, int th, int tw, int oh, int ow, unsigned slots,
                 uintptr_t align_bits, const char* align_what, G&& gather, S&& stitch) {
  const dim3 block(TB_X * TB_Y);
  if (to_g32) {
    TILE_TRY(chk_g32(who, g32, tw, th, tw, ""));
    TILE_TRY(gather(dim3((tw + TB_X - 1) / TB_X, (th + TB_Y - 1) / TB_Y, slots), block));
  } else {
    TILE_TRY(chk_aligned(who, align_bits, align_what));
    const dim3 grid((ow + TB_X - 1) / TB_X, oh, slots);   // 4 oh HR rows, TB_Y per workgroup
    TILE_TRY(chk_tile_rows(who, oh, grid.y));
    stitch(grid, block);
  }
  return 0;
}

// The table ops' common checks (esr_tile_many, esr_tile_img, esr_tile_hr: the same fields); c8 = the 8-bit forms' channels.
template <typename P>
int table_checks(const char* who, const P* p, bool c8, bool only3) {
  if (!p) return chk_args(who, false, 0, nullptr, nullptr, 0, 0);
  TILE_TRY(chk_args(who, p->items && p->th > 0 && p->tw > 0, p->to_g32, &p->g32, p->slots_nchw, p->C, p->dtype));
  TILE_TRY(chk_tile_pad_scale(who, p->tile, p->pad, p->scale, false, 0, 0));
  TILE_TRY(c8 ? chk_channels_8bit(who, p->C, only3) : chk_channels(who, p->C));
  TILE_TRY(chk_side_scale(who, p->to_g32, p->scale));
  TILE_TRY(chk_window(who, p->th, p->tw, p->tile, p->pad));
  TILE_TRY(chk_count(who, "n_slots", p->n_slots));
  TILE_TRY(chk_slots(who, "n_slots", p->n_slots));
  TILE_TRY(chk_window_rows(who, p->th, TB_Y));
  return chk_items(who, p->items);
}

// The two 8-bit entries: esr_tile_hr has esr_tile_img's fields, `hr` picks its gather.
int tile_img_run(const esr_tile_img* p, esr_stream_t stream, const char* who, bool hr) {
  TILE_TRY(table_checks(who, p, true, hr));
  hipStream_t st = (hipStream_t)stream;
  if (hr && p->to_g32) {
    TILE_TRY(chk_g32(who, p->g32, p->tw, p->th, p->tw, ""));
    const esr_tile_hr q = *(const esr_tile_hr*)p;
    const dim3 grid((p->tw + HR_T - 1) / HR_T, (p->th + HR_T - 1) / HR_T, (unsigned)p->n_slots);   // y <= 65535: checked above
    if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_hr_gather_kernel<_Float16>, grid, dim3(HR_T * HR_T), 0, st, q);
    else hipLaunchKernelGGL(tile_hr_gather_kernel<float>, grid, dim3(HR_T * HR_T), 0, st, q);
    return esr_check_launch("tile_hr_gather_kernel");
  }
  // the largest owned rectangle of any image with this window: min(tile, H) = min(tile, th), and alike along x
  const int ow = p->tile < p->tw ? p->tile : p->tw, oh = p->tile < p->th ? p->tile : p->th;
  TILE_TRY(plain_launch(who, p->to_g32, p->g32, p->th, p->tw, oh, ow, (unsigned)p->n_slots, (uintptr_t)p->slots_nchw,
                        "slots_nchw (and 4-byte aligned images)",
                        [&](dim3 grid, dim3 block) {
                          if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_img_gather_kernel<_Float16>, grid, block, 0, st, *p);
                          else hipLaunchKernelGGL(tile_img_gather_kernel<float>, grid, block, 0, st, *p);
                          return 0;
                        },
                        [&](dim3 grid, dim3 block) {
                          if (p->C == 1) hipLaunchKernelGGL(tile_img_stitch_kernel<1>, grid, block, 0, st, *p);
                          else hipLaunchKernelGGL(tile_img_stitch_kernel<3>, grid, block, 0, st, *p);
                        }));
  return esr_check_launch("tile_img_kernel");
}

}  // namespace

extern "C" int esr_tile_op(const esr_tile* p, esr_stream_t stream) {
  const char* const who = "esr_tile_op";
  if (!p) return chk_args(who, false, 0, nullptr, nullptr, 0, 0);
  TILE_TRY(chk_args(who, p->nchw && p->B > 0 && p->H > 0 && p->W > 0, p->to_g32, &p->g32, p->slots_nchw, p->C, p->dtype));
  TILE_TRY(chk_tile_pad_scale(who, p->tile, p->pad, p->scale, true, p->H, p->W));
  TILE_TRY(chk_channels(who, p->C));
  TILE_TRY(chk_side_scale(who, p->to_g32, p->scale));
  TileImageGeom g;
  TILE_TRY(chk_per_image(who, p->H, p->W, p->tile, p->pad, p->scale, p->t_begin, p->t_count, &g));
  TILE_TRY(chk_slots(who, "t_count * B", (int64_t)p->t_count * p->B));
  hipStream_t st = (hipStream_t)stream;
  const int ow = p->tile < g.wl ? p->tile : g.wl, oh = p->tile < g.hl ? p->tile : g.hl;   // the largest owned rectangle
  TILE_TRY(plain_launch(who, p->to_g32, p->g32, g.th, g.tw, oh, ow, (unsigned)(p->t_count * p->B),
                        (uintptr_t)p->nchw | (uintptr_t)p->slots_nchw, "nchw and slots_nchw",
                        [&](dim3 grid, dim3 block) {
                          TILE_TRY(chk_window_rows(who, g.th, TB_Y));   // the table ops refuse this before they come here
                          if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_gather_kernel<_Float16>, grid, block, 0, st, *p, g.th, g.tw, g.nx, g.ntiles);
                          else hipLaunchKernelGGL(tile_gather_kernel<float>, grid, block, 0, st, *p, g.th, g.tw, g.nx, g.ntiles);
                          return 0;
                        },
                        [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(tile_stitch_kernel, grid, block, 0, st, *p, g.th, g.tw, g.nx, g.ntiles); }));
  return esr_check_launch("tile_kernel");
}

// Per-item fields (image pointer, H, W, t, live) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_many_op(const esr_tile_many* p, esr_stream_t stream) {
  const char* const who = "esr_tile_many_op";
  TILE_TRY(table_checks(who, p, false, false));
  hipStream_t st = (hipStream_t)stream;
  // the largest owned rectangle of any image with this window: min(tile, H) = min(tile, th), and alike along x
  const int ow = p->tile < p->tw ? p->tile : p->tw, oh = p->tile < p->th ? p->tile : p->th;
  TILE_TRY(plain_launch(who, p->to_g32, p->g32, p->th, p->tw, oh, ow, (unsigned)p->n_slots, (uintptr_t)p->slots_nchw,
                        "slots_nchw (and images)",
                        [&](dim3 grid, dim3 block) {
                          if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_many_gather_kernel<_Float16>, grid, block, 0, st, *p);
                          else hipLaunchKernelGGL(tile_many_gather_kernel<float>, grid, block, 0, st, *p);
                          return 0;
                        },
                        [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(tile_many_stitch_kernel, grid, block, 0, st, *p); }));
  return esr_check_launch("tile_many_kernel");
}

extern "C" int esr_tile_img_op(const esr_tile_img* p, esr_stream_t stream) {
  return tile_img_run(p, stream, "esr_tile_img_op", false);
}

// Items and descriptors (pointers, sizes, tables) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_hr_op(const esr_tile_hr* p, esr_stream_t stream) {
  return tile_img_run((const esr_tile_img*)p, stream, "esr_tile_hr_op", true);
}
