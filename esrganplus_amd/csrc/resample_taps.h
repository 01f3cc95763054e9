// resample_taps.h — the two tap loops of the in-kernel MATLAB-bicubic resample (util.py:323-341), shared by
// batch_assemble.hip's generated LR and tile_io.hip's HR gather so that both give the same bits: an fp32 sum over the
// taps in ascending order, acc += w * x, for three channels at a time.  The clamps keep any table inside the image and
// the LDS row.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// H pass of one output row on one source column: wy / iy are the row's taps, fetch(c, sy) source channel c at row sy.
template <typename Fetch>
__device__ __forceinline__ void resample_h_taps(const float* wy, const int32_t* iy, int taps, int hr_h, Fetch fetch,
                                                float acc[3]) {
  for (int t = 0; t < taps; ++t) {
    const int sy = clampi(iy[t], 0, hr_h - 1);
    const float wt = wy[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wt * fetch(c, sy);
  }
}

// W pass of one output pixel out of the staged H-pass rows: row[c * plane + xs] is channel c at source column c_lo + xs.
__device__ __forceinline__ void resample_w_taps(const float* wx, const int32_t* ix, int taps, int hr_w, int c_lo, int span,
                                                const float* row, int plane, float acc[3]) {
  for (int t = 0; t < taps; ++t) {
    const int xs = clampi(clampi(ix[t], 0, hr_w - 1) - c_lo, 0, span - 1);
    const float wt = wx[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += wt * row[c * plane + xs];
  }
}

// The source columns [lo, hi] the taps of one output column touch.
__device__ __forceinline__ void resample_col_span(const int32_t* ix, int taps, int hr_w, int& lo, int& hi) {
  lo = hr_w - 1;
  hi = 0;
  for (int t = 0; t < taps; ++t) {
    const int s = clampi(ix[t], 0, hr_w - 1);
    lo = s < lo ? s : lo;
    hi = s > hi ? s : hi;
  }
}

}  // namespace
