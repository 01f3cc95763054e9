// tile_x8.hip — the two ends of the tiled x8 self-ensemble, tile_io.hip and dihedral.hip fused: gather-import = the
// fixed-size windows of an NCHW fp32 image -> their flip / transpose copies as G32 slots, stitch-reduce = the slots' fp32
// NCHW outputs -> inverse transforms summed in k order -> the owned rectangle of every tile in the caller's NCHW image.
// Geometry and index maps: include/esrgan_hip.h (esr_tile, esr_dihedral, esr_tile_x8).  Plain loads, stores and VALU.
#include "tile_geom.h"

namespace {

constexpr int TX_TILE = 32;   // 32 x 32 pixels per workgroup, one pixel per thread

__device__ __forceinline__ int flip(bool on, int n, int i) { return on ? n - 1 - i : i; }

// Every slot of the range is written from ONE read of the window's 32 x 32 tile: it is staged in the LDS as finished
// 32-byte channel groups, straight slots take their own pixel, transposed slots the mirrored one — so that both the NCHW
// reads and the G32 writes run along x.  Window-local coordinates throughout: the transforms turn the WINDOW (th x tw).
template <typename T>
__global__ __launch_bounds__(1024) void tile_x8_gather_kernel(const esr_tile_x8 p, int th, int tw, int nx, int ntiles) {
  constexpr int CPG = DT<T>::CPG;
  __shared__ u32x4 tile[TX_TILE][TX_TILE + 1][2];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x0 = blockIdx.x * TX_TILE, y0 = blockIdx.y * TX_TILE;
  const int s = blockIdx.z / p.B, b = blockIdx.z - s * p.B;
  const int t = p.t_begin + s < ntiles ? p.t_begin + s : ntiles - 1;   // a tail pass repeats the last tile
  const TileAxis ay = tile_axis(p.H, p.tile, p.pad, th, t / nx), ax = tile_axis(p.W, p.tile, p.pad, tw, t % nx);
  u32x4 own[2];                       // this thread's window pixel (y0 + ly, x0 + lx) as a finished 32-byte channel group
  {
    const int sy = y0 + ly, sx = x0 + lx;
    const bool in = sy < th && sx < tw;
    const int64_t plane = (int64_t)p.H * p.W;
    const float* const src = p.nchw + (int64_t)b * p.C * plane + (int64_t)(ay.w0 + (in ? sy : 0)) * p.W + ax.w0 + (in ? sx : 0);
    alignas(16) T v[CPG];
#pragma unroll
    for (int e = 0; e < CPG; ++e) v[e] = (T)((in && e < 8 && e < p.C) ? src[e * plane] : 0.f);
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
    const int fy = flip((k & 2) != 0, th, sy), fx = flip((k & 1) != 0, tw, sx);   // where it lands after the flips
    const int row = tr ? fx : fy, col = tr ? fy : fx;
    char* const dst = (char*)p.g32.ptr + (((int64_t)i * p.t_count + s) * p.B + b) * p.g32.batch_stride +
                      ((int64_t)(row + 1) * p.g32.wp + col + 1) * 32;
    // straight slots: the thread's own pixel from registers; transposed slots: the mirrored LDS entry
    ((u32x4*)dst)[0] = tr ? tile[ty][tx][0] : own[0];
    ((u32x4*)dst)[1] = tr ? tile[ty][tx][1] : own[1];
  }
}

// One thread = one HR pixel of a tile's owned rectangle, all C channels: acc = [nchw]; acc += R_k(o_k) for k ascending
// (one fp32 add each), the inverse index taken in window-local HR coordinates; nchw = acc * mean_scale.  Transposed
// slots are read along THEIR x and turned through the LDS.  p.H, p.W are the HR image; every lane is bounded by the
// owned rectangle.
__global__ __launch_bounds__(1024) void tile_x8_reduce_kernel(const esr_tile_x8 p, int th, int tw, int nx, int ntiles) {
  __shared__ u32x4 tile[TX_TILE][TX_TILE + 1][2];
  const int s = blockIdx.z / p.B, b = blockIdx.z - s * p.B;
  const int t = p.t_begin + s;
  if (t >= ntiles) return;                          // a tail pass: the repeated windows are neither read nor written
  const TileAxis ay = tile_axis(p.H >> 2, p.tile, p.pad, th, t / nx), ax = tile_axis(p.W >> 2, p.tile, p.pad, tw, t % nx);
  const int oh = 4 * ay.on, ow = 4 * ax.on;         // the owned rectangle, HR pixels
  const int x0 = blockIdx.x * TX_TILE, y0 = blockIdx.y * TX_TILE;
  if (x0 >= ow || y0 >= oh) return;                 // whole workgroup outside this tile's rectangle
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int hh = 4 * th, hw = 4 * tw;               // the window's output
  const int wy = 4 * (ay.o0 - ay.w0), wx = 4 * (ax.o0 - ax.w0);   // the owned rectangle inside it
  const bool own = y0 + ly < oh && x0 + lx < ow;
  const int64_t dst_plane = (int64_t)p.H * p.W, src_plane = (int64_t)hh * hw;
  float* const dst = p.nchw + (int64_t)b * p.C * dst_plane + (int64_t)(4 * ay.o0 + y0 + ly) * p.W + 4 * ax.o0 + x0 + lx;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = (own && p.accumulate && e < p.C) ? dst[e * dst_plane] : 0.f;
  for (int i = 0; i < p.k_count; ++i) {
    const int k = p.k_begin + i;
    const bool fv = (k & 1) != 0, fh = (k & 2) != 0;
    const float* const slot = p.slots_nchw + (((int64_t)i * p.t_count + s) * p.B + b) * p.C * src_plane;
    alignas(16) float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!(k & 4)) {
      if (own) {
        const float* const src = slot + (int64_t)flip(fh, hh, wy + y0 + ly) * hw + flip(fv, hw, wx + x0 + lx);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < p.C ? src[e * src_plane] : 0.f;
      }
    } else {
      // this thread fetches the value of owned pixel (y0 + lx, x0 + ly): o_k[xs(x)][ys(y)], a 4 tw x 4 th slot
      const int oy = y0 + lx, ox = x0 + ly;
      __syncthreads();                       // the previous turn's reads are done
      if (oy < oh && ox < ow) {
        const float* const src = slot + (int64_t)flip(fv, hw, wx + ox) * hh + flip(fh, hh, wy + oy);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < p.C ? src[e * src_plane] : 0.f;
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
  if (!own) return;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < p.C) dst[e * dst_plane] = __fmul_rn(acc[e], p.mean_scale);
}

}  // namespace

extern "C" int esr_tile_x8_op(const esr_tile_x8* p, esr_stream_t stream) {
  if (!p || !p->nchw || (p->to_g32 ? !p->g32.ptr : !p->slots_nchw) || p->B <= 0 || p->C <= 0 || p->H <= 0 || p->W <= 0 ||
      (p->dtype != ESR_F16 && p->dtype != ESR_F32)) {
    esr_set_error("esr_tile_x8_op: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->tile < 1 || p->pad < 0 || (p->scale != 1 && p->scale != 4) || p->H % p->scale || p->W % p->scale) {
    esr_set_error("esr_tile_x8_op: tile = %d (>= 1), pad = %d (>= 0), scale = %d (1 or 4, dividing H and W)", p->tile, p->pad, p->scale);
    return ESR_ERR_INVALID;
  }
  if (p->k_begin < 0 || p->k_count < 1 || (int64_t)p->k_begin + p->k_count > 8) {
    esr_set_error("esr_tile_x8_op: slots [%d, %d + %d) of 8", p->k_begin, p->k_begin, p->k_count);
    return ESR_ERR_INVALID;
  }
  if (p->C > 8) {
    esr_set_error("esr_tile_x8_op: C = %d does not fit one fp32 channel group", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->scale != (p->to_g32 ? 1 : 4)) {
    esr_set_error("esr_tile_x8_op: the gather runs at scale 1 and the stitch at scale 4, got %d", p->scale);
    return ESR_ERR_UNSUPPORTED;
  }
  const int hl = p->H / p->scale, wl = p->W / p->scale;
  const int th = tile_window(hl, p->tile, p->pad), tw = tile_window(wl, p->tile, p->pad);
  const int ny = tile_count(hl, p->tile), nx = tile_count(wl, p->tile);
  const int64_t ntiles = (int64_t)ny * nx;
  if (ntiles > (1 << 30)) {
    esr_set_error("esr_tile_x8_op: %lld tiles are more than one image may have", (long long)ntiles);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->t_begin < 0 || p->t_begin >= ntiles || p->t_count < 1) {
    esr_set_error("esr_tile_x8_op: tiles [%d, %d + %d) of %lld", p->t_begin, p->t_begin, p->t_count, (long long)ntiles);
    return ESR_ERR_INVALID;
  }
  const bool straight = p->k_begin < 4, turned = p->k_begin + p->k_count > 4;
  if (straight && turned && th != tw) {
    esr_set_error("esr_tile_x8_op: a range across k = 4 needs square windows, got %d x %d (the transposed slots are %d x %d)", th, tw, tw, th);
    return ESR_ERR_INVALID;
  }
  if ((int64_t)p->k_count * p->t_count * p->B > 65535) {
    esr_set_error("esr_tile_x8_op: k_count * t_count * B = %lld slots are too many for one launch", (long long)p->k_count * p->t_count * p->B);
    return ESR_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(TX_TILE * TX_TILE);
  const unsigned windows = (unsigned)(p->t_count * p->B);
  if (p->to_g32) {
    if (p->g32.wp < (turned ? th : tw) + 2 || p->g32.ngroups < 1) {
      esr_set_error("esr_tile_x8_op: the G32 view (wp = %d) is narrower than the %d x %d window's slots", p->g32.wp, th, tw);
      return ESR_ERR_INVALID;
    }
    const dim3 grid((tw + TX_TILE - 1) / TX_TILE, (th + TX_TILE - 1) / TX_TILE, windows);
    if (grid.y > 65535) {
      esr_set_error("esr_tile_x8_op: a window of %d rows is too tall for one launch", th);
      return ESR_ERR_UNSUPPORTED;
    }
    if (p->dtype == ESR_F16) hipLaunchKernelGGL(tile_x8_gather_kernel<_Float16>, grid, block, 0, st, *p, th, tw, nx, (int)ntiles);
    else hipLaunchKernelGGL(tile_x8_gather_kernel<float>, grid, block, 0, st, *p, th, tw, nx, (int)ntiles);
  } else {
    if (((uintptr_t)p->nchw | (uintptr_t)p->slots_nchw) & 15) {
      esr_set_error("esr_tile_x8_op: the stitch needs 16-byte aligned nchw and slots_nchw");
      return ESR_ERR_INVALID;
    }
    const int ow = p->tile < wl ? p->tile : wl, oh = p->tile < hl ? p->tile : hl;   // the largest owned rectangle
    const dim3 grid((4 * ow + TX_TILE - 1) / TX_TILE, (4 * oh + TX_TILE - 1) / TX_TILE, windows);
    if (grid.y > 65535) {
      esr_set_error("esr_tile_x8_op: tiles of %d rows are too tall for one launch", oh);
      return ESR_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(tile_x8_reduce_kernel, grid, block, 0, st, *p, th, tw, nx, (int)ntiles);
  }
  return esr_check_launch("tile_x8_kernel");
}
