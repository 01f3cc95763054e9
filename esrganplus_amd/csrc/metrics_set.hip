// metrics_set.hip — PSNR, SSIM, PSNR_Y and SSIM_Y of a whole image SET in one launch set (esr_image_set_metrics): what
// codes/test.py:69-110 and the validation loop of codes/train.py:121-159 compute per image, from 8-bit HWC image pairs
// that stay on the device (forward_images' results against their ground truth).  Table-driven like tile_io.hip: one
// item per pair in device memory, one workgroup per 16 x 32 tile of one image's cropped region.  The bytes are read once:
// a workgroup stages its tile plus the 10-pixel window halo of both images in LDS, derives the unrounded luma there and
// produces all four sums from that staging — no fp64 plane and no float image goes to memory.  The 11 x 11 window is
// outer(k, k), so it runs as a row filter into LDS and a column filter out of it: 22 taps where metrics.hip's plain
// window takes 121.  No floating-point atomics: every workgroup stores its four partial sums, a second small kernel adds
// an image's partials in a fixed order (see set_metrics_sum_kernel).  Layout and contract: include/esrgan_hip.h.
#include "common.h"

namespace {

constexpr int TH = ESR_SET_METRICS_TILE_H, TW = ESR_SET_METRICS_TILE_W;   // 16 x 32: SSIM outputs / owned pixels of one tile
constexpr int HALO = 10;                 // the 11-tap window reaches 10 pixels past an output
constexpr int SH = TH + HALO, SW = TW + HALO;     // staged pixels: 26 x 42 of each image
constexpr int NT = 256;
constexpr int ROW_DW = (3 + SW * 3 + 3) / 4;      // dwords that hold a staged row at any byte alignment: 33

static_assert(sizeof(esr_set_metrics_item) == 32, "esr_set_metrics_item is a 32-byte entry");
static_assert(ROW_DW * 4 >= 3 + SW * 3, "a staged row with its byte shift fits its dwords");

// metrics.hip's y_of_bgr: the unrounded luma codes/test.py:85-86 compares
__device__ __forceinline__ double luma(int b, int g, int r) {
  return ((double)b * 24.966 + (double)g * 128.553 + (double)r * 65.481) / 255.0 + 16.0;
}

// Sum of v over the workgroup in a fixed order (lanes by halving, then the four waves in turn); the result is valid in
// thread 0.  `red` holds one double per wave.
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();                                  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < NT / 64; ++i) s += red[i];
  return s;
}

// One workgroup = one tile of one image: cropped pixels [y0, y0 + TH) x [x0, x0 + TW) are its share of the two squared-
// error sums, and the SSIM outputs at those positions (window rows y0 .. y0 + TH + 9) its share of the two SSIM sums.
__global__ __launch_bounds__(NT) void set_metrics_tile_kernel(const esr_set_metrics p) {
  __shared__ uint32_t raw[2][SH][ROW_DW];     // the staged bytes of sr / hr, every row at its own alignment in memory
  __shared__ uint8_t shift[2][SH];            // byte offset of a row's first pixel inside raw[s][r]
  __shared__ double pv[2][SH][SW];            // the plane in work (Y, then the three channels) of sr / hr
  __shared__ double hb[5][SH][TW];            // the row-filtered moments of that plane
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  int lo = 0, hi = p.n - 1;                   // the last item whose first unit is <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.items[mid].first <= b) lo = mid; else hi = mid - 1;
  }
  const esr_set_metrics_item it = p.items[lo];
  const int ch = it.H - 2 * p.crop, cw = it.W - 2 * p.crop;
  const int ntx = (cw + TW - 1) / TW, nty = (ch + TH - 1) / TH;
  const int u = b - it.first;
  int rows = 0, cols = 0, y0 = 0, x0 = 0;     // a unit outside its image's tiles (a table that contradicts the sizes) stages nothing
  if (ch > 0 && cw > 0 && u >= 0 && u < ntx * nty) {
    y0 = (u / ntx) * TH; x0 = (u % ntx) * TW;
    rows = min(SH, ch - y0); cols = min(SW, cw - x0);
  }
  // ---- stage: whole aligned dwords that hold bytes of the row (an aligned dword never leaves the pages of its bytes)
  for (int idx = tid; idx < 2 * SH * ROW_DW; idx += NT) {
    const int s = idx / (SH * ROW_DW), r = (idx / ROW_DW) % SH, k = idx % ROW_DW;
    if (r >= rows) continue;
    const uint8_t* const row = (s ? it.hr : it.sr) + ((int64_t)(y0 + p.crop + r) * it.W + x0 + p.crop) * 3;
    const int sh = (int)((uintptr_t)row & 3);
    if (k == 0) shift[s][r] = (uint8_t)sh;
    if (4 * k < sh + 3 * cols) raw[s][r][k] = *(const uint32_t*)(row - sh + 4 * k);
  }
  __syncthreads();
  // ---- squared errors of the owned pixels, and the Y plane
  const int ib = p.bgr ? 0 : 2;               // byte of a pixel that holds B; R is the other end
  uint32_t sse = 0;
  double sse_y = 0.0;
  for (int idx = tid; idx < SH * SW; idx += NT) {
    const int r = idx / SW, x = idx % SW;
    if (r >= rows || x >= cols) continue;
    const uint8_t* const a = (const uint8_t*)raw[0][r] + shift[0][r] + 3 * x;
    const uint8_t* const t = (const uint8_t*)raw[1][r] + shift[1][r] + 3 * x;
    const double ya = luma(a[ib], a[1], a[2 - ib]), yt = luma(t[ib], t[1], t[2 - ib]);
    pv[0][r][x] = ya; pv[1][r][x] = yt;
    if (r < TH && x < TW) {
      const int d0 = (int)a[0] - (int)t[0], d1 = (int)a[1] - (int)t[1], d2 = (int)a[2] - (int)t[2];
      sse += (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2);       // exact: at most 6 pixels per thread
      sse_y += (ya - yt) * (ya - yt);
    }
  }
  // ---- SSIM of the four planes: plane 0 is Y (in pv already), planes 1..3 the bytes 0..2 of a pixel
  const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
  double ssim_c = 0.0, ssim_y = 0.0;
  for (int plane = 0; plane < 4; ++plane) {
    if (plane > 0) {                           // pv is free: every thread is past the row filter of the plane before
      for (int idx = tid; idx < SH * SW; idx += NT) {
        const int r = idx / SW, x = idx % SW;
        if (r >= rows || x >= cols) continue;
        pv[0][r][x] = (double)((const uint8_t*)raw[0][r])[shift[0][r] + 3 * x + plane - 1];
        pv[1][r][x] = (double)((const uint8_t*)raw[1][r])[shift[1][r] + 3 * x + plane - 1];
      }
    }
    __syncthreads();                           // pv written; hb no longer read by the column filter of the plane before
    for (int idx = tid; idx < SH * TW; idx += NT) {
      const int r = idx / TW, x = idx % TW;
      if (r >= rows || x + HALO >= cols) continue;
      double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int j = 0; j <= HALO; ++j) {
        const double a = pv[0][r][x + j], t = pv[1][r][x + j];
        const double wa = p.win[j] * a, wt = p.win[j] * t;
        m1 += wa; m2 += wt; s11 += wa * a; s22 += wt * t; s12 += wa * t;
      }
      hb[0][r][x] = m1; hb[1][r][x] = m2; hb[2][r][x] = s11; hb[3][r][x] = s22; hb[4][r][x] = s12;
    }
    __syncthreads();
    double acc = 0.0;
    for (int idx = tid; idx < TH * TW; idx += NT) {
      const int y = idx / TW, x = idx % TW;
      if (y + HALO >= rows || x + HALO >= cols) continue;
      double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int i = 0; i <= HALO; ++i) {
        const double w = p.win[i];
        m1 += w * hb[0][y + i][x]; m2 += w * hb[1][y + i][x];
        s11 += w * hb[2][y + i][x]; s22 += w * hb[3][y + i][x]; s12 += w * hb[4][y + i][x];
      }
      const double v1 = s11 - m1 * m1, v2 = s22 - m2 * m2, cv = s12 - m1 * m2;
      acc += ((2 * m1 * m2 + c1) * (2 * cv + c2)) / ((m1 * m1 + m2 * m2 + c1) * (v1 + v2 + c2));
    }
    if (plane == 0) ssim_y = acc; else ssim_c += acc;
  }
  const double t0 = block_sum((double)sse, red), t1 = block_sum(sse_y, red);
  const double t2 = block_sum(ssim_c, red), t3 = block_sum(ssim_y, red);
  if (tid == 0) {
    double* const dst = p.scratch + (int64_t)b * 4;
    dst[0] = t0; dst[1] = t1; dst[2] = t2; dst[3] = t3;
  }
}

// One workgroup = one image: thread t adds the partials of the image's units t, t + NT, ... in that order, then the
// workgroup adds its threads as block_sum does.  The order depends on the image's number of units alone, and a unit's
// partials on the image's bytes alone: the four sums carry no trace of the other images or of the place in the table.
__global__ __launch_bounds__(NT) void set_metrics_sum_kernel(const esr_set_metrics p) {
  __shared__ double red[NT / 64];
  const int i = blockIdx.x;
  const int first = p.items[i].first, end = i + 1 < p.n ? p.items[i + 1].first : p.n_units;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int u = first + (int)threadIdx.x; u < end && u < p.n_units; u += NT) {
    if (u < 0) continue;
    const double* const src = p.scratch + (int64_t)u * 4;
    s[0] += src[0]; s[1] += src[1]; s[2] += src[2]; s[3] += src[3];
  }
  double t[4];
  for (int k = 0; k < 4; ++k) t[k] = block_sum(s[k], red);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) p.out[(int64_t)i * 4 + k] = t[k];
}

}  // namespace

// Items live in device memory and cannot be read here; sizes_host repeats their H, W so that the crop, the unit count
// and the launch limits are checked before anything runs (see the header).
extern "C" int esr_image_set_metrics(const esr_set_metrics* p, esr_stream_t stream) {
  if (!p || !p->items || !p->sizes_host || !p->out || !p->scratch) {
    esr_set_error("esr_image_set_metrics: invalid arguments (a null pointer)");
    return ESR_ERR_INVALID;
  }
  if (p->n <= 0 || p->crop < 0) {
    esr_set_error("esr_image_set_metrics: n = %d (>= 1), crop = %d (>= 0)", p->n, p->crop);
    return ESR_ERR_INVALID;
  }
  if (((uintptr_t)p->items & 7) || ((uintptr_t)p->out & 7) || ((uintptr_t)p->scratch & 7)) {
    esr_set_error("esr_image_set_metrics: the item table, out and scratch need 8-byte alignment");
    return ESR_ERR_INVALID;
  }
  int64_t units = 0;
  for (int i = 0; i < p->n; ++i) {
    const int64_t H = p->sizes_host[2 * i], W = p->sizes_host[2 * i + 1];
    const int64_t ch = H - 2 * (int64_t)p->crop, cw = W - 2 * (int64_t)p->crop;
    if (H < 1 || W < 1 || ch < 1 || cw < 1) {
      esr_set_error("esr_image_set_metrics: crop = %d leaves no pixels of image %d (%lld x %lld)", p->crop, i, (long long)H, (long long)W);
      return ESR_ERR_INVALID;
    }
    units += ((ch + TH - 1) / TH) * ((cw + TW - 1) / TW);
  }
  if (units != p->n_units) {
    esr_set_error("esr_image_set_metrics: n_units = %d, the sizes give %lld tiles of %d x %d", p->n_units, (long long)units, TH, TW);
    return ESR_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_metrics_tile_kernel, dim3((unsigned)units), dim3(NT), 0, st, *p);
  hipLaunchKernelGGL(set_metrics_sum_kernel, dim3((unsigned)p->n), dim3(NT), 0, st, *p);
  return esr_check_launch("esr_image_set_metrics");
}
