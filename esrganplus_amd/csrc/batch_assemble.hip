// batch_assemble.hip — one training batch out of a device-resident image pool in ONE launch: what B calls of
// LRHRDataset.__getitem__ do on CPU workers (codes/data/LRHR_dataset.py:81-121, util.py:79,94-106,276-343) — the
// per-sample crop windows, the flips / transpose, uint8 -> float, BGR -> RGB — and, where a sample has no LR image, the
// LR window resampled straight from the HR image with the whole image's MATLAB-bicubic tables.
// Argument struct and index maps: include/esrgan_hip.h (esr_batch, esr_batch_item).  Plain loads, stores and VALU.
#include "common.h"
#include "resample_taps.h"

namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_COPY = 32;     // a copied tile: 32 x 32 window pixels, 4 per thread and channel
constexpr int BA_GEN = 16;      // a generated tile: 16 x 16 LR pixels, one per thread
// Source columns the W pass of 16 consecutive LR columns can touch: 15 * scale + taps <= 15 * 8 + 33 = 153 at scale 8
// (mirrored taps fold back inside that range); 161 = the 128 + 33 of a tile's plain footprint, odd.
constexpr int BA_SPAN = 161;
// LDS of one workgroup, the same at every scale: the H-pass rows of a generated tile, 3 x 16 x 161 floats = 30 912
// bytes (a copied tile's 3 x 32 x 33 floats live in the same words), and the finished 3 x 16 x 17 tile of a generated
// one = 3 264 bytes, with the 128 bytes of its column bounds: 34 304 bytes in all.
constexpr int BA_ROWS_WORDS = 3 * BA_GEN * BA_SPAN;
constexpr int BA_TILE_WORDS = 3 * BA_GEN * (BA_GEN + 1);
static_assert(3 * BA_COPY * (BA_COPY + 1) <= BA_ROWS_WORDS, "a copied tile fits the H-pass rows");

// Pixel (y, x) of source channel c of an image of h x w: float32 CHW planes, or uint8 HWC with packed rows — a TRUE
// division, so that the value is numpy's astype(float32) / 255. (util.py:79) bit for bit.
template <int FMT>
__device__ __forceinline__ float fetch(const void* img, int h, int w, int c, int y, int x) {
  if (FMT == 0) return ((const float*)img)[((int64_t)c * h + y) * w + x];
  return __fdiv_rn((float)((const uint8_t*)img)[((int64_t)y * w + x) * 3 + c], 255.0f);
}

// blockIdx = (tile, 0: the HR window / 1: the LR window, sample).  Every tile is cut in WINDOW coordinates (a, b) —
// before the flips — and staged in the LDS; it is written out with consecutive lanes along the output's x, which for a
// transposed sample is the window's row index: neither the reads nor the writes stride by an image row per lane.
template <int FMT>
__global__ __launch_bounds__(BA_THREADS) void batch_assemble_kernel(const esr_batch p) {
  __shared__ float rows[BA_ROWS_WORDS];
  __shared__ float done[BA_TILE_WORDS];
  __shared__ int span[2 * BA_GEN];
  const esr_batch_item it = p.items[blockIdx.z];
  const bool is_lr = blockIdx.y == 1;
  const bool gen = is_lr && it.lr == nullptr;
  const int n = is_lr ? p.lr_size : p.lr_size * p.scale;        // the window's side
  const int T = gen ? BA_GEN : BA_COPY;
  const int nt = (n + T - 1) / T;
  if (blockIdx.x >= (unsigned)(nt * nt)) return;                 // the grid is sized for the kind with most tiles
  const int a0 = (int)(blockIdx.x / nt) * T, b0 = (int)(blockIdx.x % nt) * T;
  const int lx = threadIdx.x % T, ly = threadIdx.x / T, step = BA_THREADS / T;
  const bool hf = it.flags & 1, vf = it.flags & 2, tr = it.flags & 4;
  float* tile = gen ? done : rows;                                // [3][T][T + 1], window coordinates
  const int pitch = T + 1;

  if (!gen) {
    const void* img = is_lr ? it.lr : it.hr;
    const int h = is_lr ? it.lr_h : it.hr_h, w = is_lr ? it.lr_w : it.hr_w;
    const int oy = is_lr ? it.y0 : it.y0 * p.scale, ox = is_lr ? it.x0 : it.x0 * p.scale;
    for (int r = ly; r < T; r += step) {
      const int a = a0 + r, b = b0 + lx;
      if (a < n && b < n) {
#pragma unroll
        for (int c = 0; c < 3; ++c) tile[(c * T + r) * pitch + lx] = fetch<FMT>(img, h, w, c, oy + a, ox + b);
      }
    }
  } else {
    // source columns [c_lo, c_lo + BA_SPAN) cover every tap of the tile's LR columns (tables of valid sizes: see
    // BA_SPAN; the clamps below keep any table inside the image and the LDS)
    if (threadIdx.x < BA_GEN) {
      const int o = clampi(it.x0 + b0 + (int)threadIdx.x, 0, it.lr_w - 1);
      int lo, hi;
      resample_col_span(it.ix + (int64_t)o * it.taps_x, it.taps_x, it.hr_w, lo, hi);
      span[threadIdx.x] = lo;
      span[BA_GEN + threadIdx.x] = hi;
    }
    __syncthreads();
    int c_lo = span[0], c_hi = span[BA_GEN];
    for (int k = 1; k < BA_GEN; ++k) {
      c_lo = span[k] < c_lo ? span[k] : c_lo;
      c_hi = span[BA_GEN + k] > c_hi ? span[BA_GEN + k] : c_hi;
    }
    const int ncol = c_hi - c_lo + 1 < BA_SPAN ? c_hi - c_lo + 1 : BA_SPAN;
    // H pass (util.py:323-331) of the tile's rows on those columns: taps ascending, acc += w * x
    for (int e = threadIdx.x; e < BA_GEN * ncol; e += BA_THREADS) {
      const int r = e / ncol, xs = e - r * ncol;
      const int o = clampi(it.y0 + a0 + r, 0, it.lr_h - 1);
      float acc[3] = {0.f, 0.f, 0.f};
      resample_h_taps(it.wy + (int64_t)o * it.taps_y, it.iy + (int64_t)o * it.taps_y, it.taps_y, it.hr_h,
                      [&](int c, int sy) { return fetch<FMT>(it.hr, it.hr_h, it.hr_w, c, sy, c_lo + xs); }, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) rows[(c * BA_GEN + r) * BA_SPAN + xs] = acc[c];
    }
    __syncthreads();
    // W pass (util.py:333-341) from the LDS
    const int a = a0 + ly, b = b0 + lx;
    if (a < n && b < n) {
      const int o = clampi(it.x0 + b, 0, it.lr_w - 1);
      float acc[3] = {0.f, 0.f, 0.f};
      resample_w_taps(it.wx + (int64_t)o * it.taps_x, it.ix + (int64_t)o * it.taps_x, it.taps_x, it.hr_w, c_lo, BA_SPAN,
                      rows + ly * BA_SPAN, BA_GEN * BA_SPAN, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) tile[(c * T + ly) * pitch + lx] = acc[c];
    }
  }
  __syncthreads();

  // out[c][i][j] = t[c][a][b] with (a, b) = (j, i) when transposed; t = the window after hflip (b) then vflip (a)
  float* out = (is_lr ? p.lr_out : p.hr_out) + (int64_t)blockIdx.z * 3 * n * n;
  for (int r = ly; r < T; r += step) {
    const int ra = tr ? lx : r, rb = tr ? r : lx;               // the staged pixel this thread writes
    const int a = a0 + ra, b = b0 + rb;
    if (a >= n || b >= n) continue;
    const int fa = vf ? n - 1 - a : a, fb = hf ? n - 1 - b : b;
    const int i = tr ? fb : fa, j = tr ? fa : fb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int oc = p.swap_rb ? 2 - c : c;                      // output channel oc reads source channel 2 - oc
      out[((int64_t)oc * n + i) * n + j] = tile[(c * T + ra) * pitch + rb];
    }
  }
}

}  // namespace

extern "C" int esr_batch_assemble(const esr_batch* p, esr_stream_t stream) {
  if (!p || !p->items || !p->lr_out || !p->hr_out || p->B < 1 || p->lr_size < 1 ||
      (p->src_format != 0 && p->src_format != 1)) {
    esr_set_error("esr_batch_assemble: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->scale != 1 && p->scale != 2 && p->scale != 3 && p->scale != 4 && p->scale != 8) {
    esr_set_error("esr_batch_assemble: scale = %d (1, 2, 3, 4 or 8)", p->scale);
    return ESR_ERR_INVALID;
  }
  if (p->C != 3) {
    esr_set_error("esr_batch_assemble: C = %d, only 3-channel images are assembled", p->C);
    return ESR_ERR_UNSUPPORTED;
  }
  if (p->B > 65535) {
    esr_set_error("esr_batch_assemble: B = %d samples are too many for one launch", p->B);
    return ESR_ERR_UNSUPPORTED;
  }
  const int64_t hs = (int64_t)p->lr_size * p->scale;
  const int64_t hr_tiles = ((hs + BA_COPY - 1) / BA_COPY) * ((hs + BA_COPY - 1) / BA_COPY);
  const int64_t lr_tiles = (((int64_t)p->lr_size + BA_GEN - 1) / BA_GEN) * (((int64_t)p->lr_size + BA_GEN - 1) / BA_GEN);
  const int64_t tiles = hr_tiles > lr_tiles ? hr_tiles : lr_tiles;
  if (hs > 0x7fffffff || tiles > 0x7fffffff) {
    esr_set_error("esr_batch_assemble: windows of %lld x %lld HR pixels are %lld tiles, too many for one launch",
                  (long long)hs, (long long)hs, (long long)tiles);
    return ESR_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)tiles, 2, (unsigned)p->B);
  if (p->src_format == 0) hipLaunchKernelGGL(batch_assemble_kernel<0>, grid, dim3(BA_THREADS), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(batch_assemble_kernel<1>, grid, dim3(BA_THREADS), 0, (hipStream_t)stream, *p);
  return esr_check_launch("batch_assemble_kernel");
}
