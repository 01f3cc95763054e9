// tile_x8.hip — the ends of the x8 geometric self-ensemble (reference codes/models/SR_model.py:82-120, `test_x8`):
// gather-import = the windows of an image, each read once -> their eight flip / transpose copies as G32 slots,
// stitch-reduce = the slots' outputs -> inverse transforms summed in k order -> the owned rectangle of every window in the
// result.  Three ops share the two bodies of tile_ends.h:
//   esr_dihedral     the window is the whole image; the reduce reads fp32 NCHW slots or the G32 view itself
//   esr_tile_x8      windows named per image, fp32 NCHW outside
//   esr_tile_set_x8  windows named by a device table (an image set), fp32 NCHW or uint8 HWC outside
// Geometry, index maps and the accumulator protocol: include/esrgan_hip.h, tile_geom.h and tile_x8_index.h.
#include "tile_checks.h"

namespace {

template <typename T>
__global__ __launch_bounds__(1024) void dihedral_import_kernel(const esr_dihedral p) {
  // one channel group of T: C up to 16 in fp16
  x8_gather<T>(TileWhole{p.nchw, p.C, p.H, p.W}, PxF32<DT<T>::CPG>{}, p.C, p.g32, X8Range{p.k_begin, p.k_count, p.B, 0, 0.f});
}

// NCHW_SRC: the slots are slots_nchw; else the G32 view of T itself, up to 16 fp16 channels where the plan left them
template <typename T, bool NCHW_SRC>
__global__ __launch_bounds__(1024) void dihedral_reduce_kernel(const esr_dihedral p) {
  const TileWhole r{p.nchw, p.C, p.H, p.W};
  const X8Range kr{p.k_begin, p.k_count, p.B, p.accumulate, p.scale};
  if constexpr (NCHW_SRC) x8_reduce<0>(r, SlotNCHW{p.slots_nchw}, p.C, kr, 0, nullptr);
  else x8_reduce<0>(r, SlotG32<T>{p.g32}, p.C, kr, 0, nullptr);
}

template <typename T>
__global__ __launch_bounds__(1024) void tile_x8_gather_kernel(const esr_tile_x8 p, int th, int tw, int nx, int ntiles) {
  x8_gather<T>(TILE_PER_IMAGE(p, th, tw, nx, ntiles), PxF32<8>{}, p.C, p.g32, X8_RANGE(p, p.t_count * p.B));
}
__global__ __launch_bounds__(1024) void tile_x8_reduce_kernel(const esr_tile_x8 p, int th, int tw, int nx, int ntiles) {
  x8_reduce<0>(TILE_PER_IMAGE(p, th, tw, nx, ntiles), SlotNCHW{p.slots_nchw}, p.C, X8_RANGE(p, p.t_count * p.B), 0, nullptr);
}

// IMG: uint8 HWC images outside (img = 1), else fp32 NCHW
template <typename T, bool IMG>
__global__ __launch_bounds__(1024) void tile_set_x8_gather_kernel(const esr_tile_set_x8 p) {
  if constexpr (IMG) x8_gather<T>(TILE_BY_TABLE(p), PxU8{p.bgr}, p.C, p.g32, X8_RANGE(p, p.n_windows));
  else x8_gather<T>(TILE_BY_TABLE(p), PxF32<8>{}, p.C, p.g32, X8_RANGE(p, p.n_windows));
}
// NC = 0: fp32 NCHW results (img = 0); NC = 1, 3: uint8 HWC results of NC channels
template <int NC>
__global__ __launch_bounds__(1024) void tile_set_x8_reduce_kernel(const esr_tile_set_x8 p) {
  x8_reduce<NC>(TILE_BY_TABLE(p), SlotNCHW{p.slots_nchw}, p.C, X8_RANGE(p, p.n_windows), p.bgr, p.acc);
}

// What the two tiled x8 entries launch, once the op's own checks are through: th x tw the upright window, oh x ow the
// largest owned rectangle (LR pixels).  gather / reduce launch on (grid, block).
template <typename G, typename S>
int x8_launch(const char* who, int to_g32, const esr_g32& g32, int k_begin, int k_count, int th, int tw, int oh, int ow, unsigned windows,
              uintptr_t align_bits, const char* align_what, const float* acc, bool acc_needed, G&& gather, S&& reduce) {
  const dim3 block(X8_TILE * X8_TILE);
  if (to_g32) {
    TILE_TRY(chk_g32(who, g32, k_begin + k_count > 4 ? th : tw, th, tw, "'s slots"));   // turned slots are tw x th
    TILE_TRY(chk_window_rows(who, th, X8_TILE));
    gather(dim3((tw + X8_TILE - 1) / X8_TILE, (th + X8_TILE - 1) / X8_TILE, windows), block);
  } else {
    TILE_TRY(chk_aligned(who, align_bits, align_what));
    if (acc_needed) {
      if (!acc) {
        esr_set_error("%s: slots [%d, %d + %d) of an 8-bit result need acc, the partial sums between the ranges", who, k_begin, k_begin, k_count);
        return ESR_ERR_INVALID;
      }
      if ((uintptr_t)acc & 15) {
        esr_set_error("%s: acc needs 16-byte alignment", who);
        return ESR_ERR_INVALID;
      }
    }
    const dim3 grid((4 * ow + X8_TILE - 1) / X8_TILE, (4 * oh + X8_TILE - 1) / X8_TILE, windows);
    TILE_TRY(chk_tile_rows(who, oh, grid.y));
    reduce(grid, block);
  }
  return 0;
}

}  // namespace

extern "C" int esr_dihedral_op(const esr_dihedral* p, esr_stream_t stream) {
  if (!p || !p->nchw || (!p->g32.ptr && !(p->slots_nchw && !p->to_g32)) || p->B <= 0 || p->C <= 0 || p->H <= 0 || p->W <= 0 ||
      x8_range_error(p->k_begin, p->k_count, 0, 0) || (p->dtype != ESR_F16 && p->dtype != ESR_F32) || (p->to_g32 && p->slots_nchw)) {
    esr_set_error("esr_dihedral_op: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (x8_range_error(p->k_begin, p->k_count, p->H, p->W)) {
    esr_set_error("esr_dihedral_op: a range across k = 4 needs H == W (the transposed slots are W x H)");
    return ESR_ERR_INVALID;
  }
  const bool nchw_src = !p->to_g32 && p->slots_nchw;
  if (p->C > (nchw_src ? 8 : p->dtype == ESR_F16 ? 16 : 8)) {
    esr_set_error("esr_dihedral_op: C = %d does not fit one channel group", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->B > 65535 || (p->H + X8_TILE - 1) / X8_TILE > 65535) {
    esr_set_error("esr_dihedral_op: B or H too large for one launch");
    return ESR_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((p->W + X8_TILE - 1) / X8_TILE, (p->H + X8_TILE - 1) / X8_TILE, p->B), block(X8_TILE * X8_TILE);
  if (p->to_g32) {
    if (p->dtype == ESR_F16) hipLaunchKernelGGL(dihedral_import_kernel<_Float16>, grid, block, 0, st, *p);
    else hipLaunchKernelGGL(dihedral_import_kernel<float>, grid, block, 0, st, *p);
  } else if (nchw_src) {
    hipLaunchKernelGGL((dihedral_reduce_kernel<float, true>), grid, block, 0, st, *p);
  } else {
    if (p->dtype == ESR_F16) hipLaunchKernelGGL((dihedral_reduce_kernel<_Float16, false>), grid, block, 0, st, *p);
    else hipLaunchKernelGGL((dihedral_reduce_kernel<float, false>), grid, block, 0, st, *p);
  }
  return esr_check_launch("dihedral_kernel");
}

extern "C" int esr_tile_x8_op(const esr_tile_x8* p, esr_stream_t stream) {
  const char* const who = "esr_tile_x8_op";
  if (!p) return chk_args(who, false, 0, nullptr, nullptr, 0, 0);
  TILE_TRY(chk_args(who, p->nchw && p->B > 0 && p->H > 0 && p->W > 0, p->to_g32, &p->g32, p->slots_nchw, p->C, p->dtype));
  TILE_TRY(chk_tile_pad_scale(who, p->tile, p->pad, p->scale, true, p->H, p->W));
  TILE_TRY(chk_k_range(who, p->k_begin, p->k_count));
  TILE_TRY(chk_channels(who, p->C));
  TILE_TRY(chk_side_scale(who, p->to_g32, p->scale));
  TileImageGeom g;
  TILE_TRY(chk_per_image(who, p->H, p->W, p->tile, p->pad, p->scale, p->t_begin, p->t_count, &g));
  TILE_TRY(chk_k_square(who, p->k_begin, p->k_count, g.th, g.tw));
  TILE_TRY(chk_slots(who, "k_count * t_count * B", (int64_t)p->k_count * p->t_count * p->B));
  hipStream_t st = (hipStream_t)stream;
  const int ow = p->tile < g.wl ? p->tile : g.wl, oh = p->tile < g.hl ? p->tile : g.hl;   // the largest owned rectangle
  TILE_TRY(x8_launch(who, p->to_g32, p->g32, p->k_begin, p->k_count, g.th, g.tw, oh, ow, (unsigned)(p->t_count * p->B),
                     (uintptr_t)p->nchw | (uintptr_t)p->slots_nchw, "nchw and slots_nchw", nullptr, false,
                     [&](dim3 grid, dim3 block) {
                       if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_x8_gather_kernel<_Float16>, grid, block, 0, st, *p, g.th, g.tw, g.nx, g.ntiles);
                       else hipLaunchKernelGGL(tile_x8_gather_kernel<float>, grid, block, 0, st, *p, g.th, g.tw, g.nx, g.ntiles);
                     },
                     [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(tile_x8_reduce_kernel, grid, block, 0, st, *p, g.th, g.tw, g.nx, g.ntiles); }));
  return esr_check_launch("tile_x8_kernel");
}

// Per-item fields (image pointer, H, W, t, live) are device memory and cannot be checked here: see the header.
extern "C" int esr_tile_set_x8_op(const esr_tile_set_x8* p, esr_stream_t stream) {
  const char* const who = "esr_tile_set_x8_op";
  if (!p) return chk_args(who, false, 0, nullptr, nullptr, 0, 0);
  TILE_TRY(chk_args(who, p->items && p->th > 0 && p->tw > 0, p->to_g32, &p->g32, p->slots_nchw, p->C, p->dtype));
  TILE_TRY(chk_tile_pad_scale(who, p->tile, p->pad, p->scale, false, 0, 0));
  TILE_TRY(chk_side_scale(who, p->to_g32, p->scale));
  TILE_TRY(chk_channels(who, p->C));
  if (p->img) TILE_TRY(chk_channels_8bit(who, p->C, false));
  TILE_TRY(chk_k_range(who, p->k_begin, p->k_count));
  TILE_TRY(chk_k_square(who, p->k_begin, p->k_count, p->th, p->tw));
  TILE_TRY(chk_window(who, p->th, p->tw, p->tile, p->pad));
  TILE_TRY(chk_count(who, "n_windows", p->n_windows));
  TILE_TRY(chk_slots(who, "k_count * n_windows", (int64_t)p->k_count * p->n_windows));
  TILE_TRY(chk_items(who, p->items));
  hipStream_t st = (hipStream_t)stream;
  // the largest owned rectangle of any image with this window: min(tile, H) = min(tile, th), and alike along x
  const int ow = p->tile < p->tw ? p->tile : p->tw, oh = p->tile < p->th ? p->tile : p->th;
  TILE_TRY(x8_launch(who, p->to_g32, p->g32, p->k_begin, p->k_count, p->th, p->tw, oh, ow, (unsigned)p->n_windows,
                     (uintptr_t)p->slots_nchw, "slots_nchw (and images)", p->acc, x8_acc_needed(p->img, p->accumulate, p->k_begin, p->k_count),
                     [&](dim3 grid, dim3 block) {
                       if (p->img) {
                         if (p->dtype == ESR_F16) hipLaunchKernelGGL((tile_set_x8_gather_kernel<_Float16, true>), grid, block, 0, st, *p);
                         else hipLaunchKernelGGL((tile_set_x8_gather_kernel<float, true>), grid, block, 0, st, *p);
                       } else {
                         if (p->dtype == ESR_F16) hipLaunchKernelGGL((tile_set_x8_gather_kernel<_Float16, false>), grid, block, 0, st, *p);
                         else hipLaunchKernelGGL((tile_set_x8_gather_kernel<float, false>), grid, block, 0, st, *p);
                       }
                     },
                     [&](dim3 grid, dim3 block) {
                       if (!p->img) hipLaunchKernelGGL(tile_set_x8_reduce_kernel<0>, grid, block, 0, st, *p);
                       else if (p->C == 1) hipLaunchKernelGGL(tile_set_x8_reduce_kernel<1>, grid, block, 0, st, *p);
                       else hipLaunchKernelGGL(tile_set_x8_reduce_kernel<3>, grid, block, 0, st, *p);
                     }));
  return esr_check_launch("tile_set_x8_kernel");
}
