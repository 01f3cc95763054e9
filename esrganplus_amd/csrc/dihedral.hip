// dihedral.hip — the two ends of the geometric self-ensemble (reference codes/models/SR_model.py:82-120, `test_x8`):
// import = NCHW fp32 -> the eight flip / transpose copies as G32 slots, reduce = slots -> inverse transforms summed in
// k order -> NCHW fp32.  Index maps: include/esrgan_hip.h (esr_dihedral).  Plain loads, stores and VALU.
#include "common.h"

namespace {

constexpr int DT_TILE = 32;   // 32 x 32 pixels per workgroup, one pixel per thread

__device__ __forceinline__ int flip(bool on, int n, int i) { return on ? n - 1 - i : i; }

// Every slot is written from ONE read of the NCHW tile: the tile is staged in the LDS as finished 32-byte channel
// groups, straight slots take their own pixel, transposed slots the mirrored one — so that both the NCHW reads and
// the G32 writes run along x.
template <typename T>
__global__ __launch_bounds__(1024) void dihedral_import_kernel(const esr_dihedral p) {
  constexpr int CPG = DT<T>::CPG;
  __shared__ u32x4 tile[DT_TILE][DT_TILE + 1][2];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x0 = blockIdx.x * DT_TILE, y0 = blockIdx.y * DT_TILE, b = blockIdx.z;
  u32x4 own[2];                       // this thread's pixel (y0 + ly, x0 + lx) as a finished 32-byte channel group
  {
    const int sy = y0 + ly, sx = x0 + lx;
    const bool in = sy < p.H && sx < p.W;
    alignas(16) T v[CPG];
#pragma unroll
    for (int e = 0; e < CPG; ++e)
      v[e] = (T)((in && e < p.C) ? p.nchw[(((int64_t)b * p.C + e) * p.H + sy) * p.W + sx] : 0.f);
    own[0] = ((const u32x4*)v)[0];
    own[1] = ((const u32x4*)v)[1];
    tile[ly][lx][0] = own[0];
    tile[ly][lx][1] = own[1];
  }
  __syncthreads();
  for (int s = 0; s < p.k_count; ++s) {
    const int k = p.k_begin + s;
    const bool tr = (k & 4) != 0;
    // source pixel of this thread: consecutive lanes walk the slot's x
    const int ty = tr ? lx : ly, tx = tr ? ly : lx;
    const int sy = y0 + ty, sx = x0 + tx;
    if (sy >= p.H || sx >= p.W) continue;
    const int fy = flip((k & 2) != 0, p.H, sy), fx = flip((k & 1) != 0, p.W, sx);   // where it lands after the flips
    const int row = tr ? fx : fy, col = tr ? fy : fx;
    char* const dst = (char*)p.g32.ptr + ((int64_t)s * p.B + b) * p.g32.batch_stride + ((int64_t)(row + 1) * p.g32.wp + col + 1) * 32;
    // straight slots: the thread's own pixel from registers; transposed slots: the mirrored LDS entry
    ((u32x4*)dst)[0] = tr ? tile[ty][tx][0] : own[0];
    ((u32x4*)dst)[1] = tr ? tile[ty][tx][1] : own[1];
  }
}

// One pixel of slot s, image b at logical (row, col) of a rows x cols slot, as CPG values (channels >= C: zero).
template <typename T, bool NCHW_SRC>
__device__ __forceinline__ void load_slot_px(const esr_dihedral& p, int s, int b, int row, int col, int rows, int cols, u32x4 raw[2]) {
  if constexpr (NCHW_SRC) {
    alignas(16) float v[8];
    const float* const base = p.slots_nchw + ((int64_t)s * p.B + b) * p.C * rows * cols + (int64_t)row * cols + col;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < p.C ? base[(int64_t)e * rows * cols] : 0.f;
    raw[0] = ((const u32x4*)v)[0];
    raw[1] = ((const u32x4*)v)[1];
  } else {
    const char* const src = (const char*)p.g32.ptr + ((int64_t)s * p.B + b) * p.g32.batch_stride + ((int64_t)(row + 1) * p.g32.wp + col + 1) * 32;
    raw[0] = ((const u32x4*)src)[0];
    raw[1] = ((const u32x4*)src)[1];
  }
}

// acc = [nchw]; acc += R_k(o_k) for k ascending (one fp32 add each); nchw = acc * scale.  Transposed slots are read
// along THEIR x and turned through the LDS.
template <typename T, bool NCHW_SRC>
__global__ __launch_bounds__(1024) void dihedral_reduce_kernel(const esr_dihedral p) {
  constexpr int CPG = DT<T>::CPG;
  __shared__ u32x4 tile[DT_TILE][DT_TILE + 1][2];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x0 = blockIdx.x * DT_TILE, y0 = blockIdx.y * DT_TILE, b = blockIdx.z;
  const int y = y0 + ly, x = x0 + lx;
  const bool own = y < p.H && x < p.W;
  float acc[CPG];
#pragma unroll
  for (int e = 0; e < CPG; ++e)
    acc[e] = (own && p.accumulate && e < p.C) ? p.nchw[(((int64_t)b * p.C + e) * p.H + y) * p.W + x] : 0.f;
  for (int s = 0; s < p.k_count; ++s) {
    const int k = p.k_begin + s;
    const bool fv = (k & 1) != 0, fh = (k & 2) != 0;
    alignas(16) u32x4 raw[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (!(k & 4)) {
      if (own) load_slot_px<T, NCHW_SRC>(p, s, b, flip(fh, p.H, y), flip(fv, p.W, x), p.H, p.W, raw);
    } else {
      // this thread fetches the value of output pixel (y0 + lx, x0 + ly): o_k[xs(x)][ys(y)], a W x H slot
      const int oy = y0 + lx, ox = x0 + ly;
      __syncthreads();                       // the previous turn's reads are done
      if (oy < p.H && ox < p.W) {
        load_slot_px<T, NCHW_SRC>(p, s, b, flip(fv, p.W, ox), flip(fh, p.H, oy), p.W, p.H, raw);
        tile[lx][ly][0] = raw[0];
        tile[lx][ly][1] = raw[1];
      }
      __syncthreads();
      if (own) { raw[0] = tile[ly][lx][0]; raw[1] = tile[ly][lx][1]; }
    }
    const T* const v = (const T*)raw;
#pragma unroll
    for (int e = 0; e < CPG; ++e) acc[e] = (s == 0 && !p.accumulate) ? (float)v[e] : __fadd_rn(acc[e], (float)v[e]);
  }
  if (!own) return;
#pragma unroll
  for (int e = 0; e < CPG; ++e)
    if (e < p.C) p.nchw[(((int64_t)b * p.C + e) * p.H + y) * p.W + x] = __fmul_rn(acc[e], p.scale);
}

}  // namespace

extern "C" int esr_dihedral_op(const esr_dihedral* p, esr_stream_t stream) {
  if (!p || !p->nchw || (!p->g32.ptr && !(p->slots_nchw && !p->to_g32)) || p->B <= 0 || p->C <= 0 || p->H <= 0 || p->W <= 0 ||
      p->k_begin < 0 || p->k_count <= 0 || p->k_begin + p->k_count > 8 || (p->dtype != ESR_F16 && p->dtype != ESR_F32) ||
      (p->to_g32 && p->slots_nchw)) {
    esr_set_error("esr_dihedral_op: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->k_begin < 4 && p->k_begin + p->k_count > 4 && p->H != p->W) {
    esr_set_error("esr_dihedral_op: a range across k = 4 needs H == W (the transposed slots are W x H)");
    return ESR_ERR_INVALID;
  }
  const bool nchw_src = !p->to_g32 && p->slots_nchw;
  if (p->C > (nchw_src ? 8 : p->dtype == ESR_F16 ? 16 : 8)) {
    esr_set_error("esr_dihedral_op: C = %d does not fit one channel group", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->B > 65535 || (p->H + DT_TILE - 1) / DT_TILE > 65535) {
    esr_set_error("esr_dihedral_op: B or H too large for one launch");
    return ESR_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((p->W + DT_TILE - 1) / DT_TILE, (p->H + DT_TILE - 1) / DT_TILE, p->B), block(DT_TILE * DT_TILE);
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
