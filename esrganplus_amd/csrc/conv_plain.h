// conv_plain.h — the epilogue of the PLAIN instantiations of conv_kernel (conv_mfma.hip): fp16 forward layers that
// are nothing but bias + activation into ONE output, the G32 map or the fp32 NCHW planes (the up-convs, HR_conv0,
// HR_conv1, every D / VGG conv in inference; not the head conv, which also stores the trunk's shortcut).  launch()
// tests that on the host, so nothing of the general epilogue (residual, noise, aux / second / third output, all
// selected at run time) is compiled into these kernels, and what is left is set up once per wave instead of once per
// row:
//   - activation kind and slope are wave-uniform and chosen in front of the rows;
//   - the lane's store address is formed once per cout block, each further row is an added stride;
//   - the rows a wave owns inside the map are counted once (one scalar compare per row);
//   - G32: a lane's 16 values travel as 8 aligned pairs (v_pk_add_f32, v_pk_mul_f32, one v_cvt_pk_f16_f32 per dword),
//     and the two half-waves exchange halves of their pixels so that a store instruction covers whole lines of one
//     channel group instead of every other 16 bytes of two;
//   - NCHW: a half-wave whose 16 channels lie past nchw_out_c does nothing, and of the others only the existing
//     channels are biased, activated and stored (scalar tests); a store instruction is 32 consecutive floats of one
//     row and channel, its address a scalar plane base + the lane's 32-bit offset.
// Per element the fp32 operations and their order are those of epilogue_block's straight-line path:
//   x = acc + bias;  v = max(x, x * slope)  (slope 0.2 | 1)  or  max(x, 0);  one round-to-nearest-even conversion
// so a plain kernel and the general one (debug_flags & 0x18 keeps a call there) store the same bits.
#pragma once
#include "mfma_tile.h"

namespace {

typedef float pl_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 pl_f16x2 __attribute__((ext_vector_type(2)));

// bias + activation of one accumulator: 16 channels of a pixel as 8 pairs
template <bool RELU>
__device__ __forceinline__ void plain_act16(const f32x16& a, const f32x4 (&bq)[4], float slope, pl_f32x2 (&w)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = 2 * i;
    const pl_f32x2 x = pl_f32x2{a[e], a[e + 1]} + pl_f32x2{bq[e >> 2][e & 3], bq[e >> 2][(e & 3) + 1]};
    if constexpr (RELU) {
      w[i] = pl_f32x2{fmaxf(x[0], 0.f), fmaxf(x[1], 0.f)};
    } else {
      const pl_f32x2 y = x * slope;
      w[i] = pl_f32x2{fmaxf(x[0], y[0]), fmaxf(x[1], y[1])};
    }
  }
}

// the rows of one cout block into the G32 map.  A lane (pixel j, half h) holds the 32 bytes of its pixel in group
// 2 cb + h; one v_permlane32_swap per dword hands the upper half-wave's first 16 bytes to the lower half-wave's second
// 16, after which lanes 0..31 / 32..63 hold bytes 0..15 / 16..31 of the pixels of ONE group and each store instruction
// writes whole lines of that group (the two lanes of a pair have the same column, so both are active or neither).
// o0 / o1 = the lane's 16 bytes (offset 16 h) of its pixel in groups 2 cb / 2 cb + 1, first row; g1: group 2 cb + 1
// lies inside the view (wave-uniform).
template <int R, int NCW, int CW, bool RELU>
__device__ __forceinline__ void plain_rows_g32(Acc8& acc, const f32x4 (&bq)[4], float slope, char* o0, char* o1, bool g1,
                                               int64_t row_bytes, int nrows) {
  sfor<R>([&](auto RR) __attribute__((always_inline)) {
    constexpr int r = decltype(RR)::value;
    if (r >= nrows) return;
    pl_f32x2 w[8];
    plain_act16<RELU>(accsel<r * NCW + CW>(acc), bq, slope, w);
    u32x4 q0, q1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(w[i], pl_f16x2));
      const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(w[4 + i], pl_f16x2));
      const auto s = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
      q0[i] = s[0]; q1[i] = s[1];
    }
    *(u32x4*)o0 = q0;
    if (g1) *(u32x4*)o1 = q1;
    o0 += row_bytes;
    o1 += row_bytes;
  });
}

// R rows (RS apart, from oyb) x this lane's pixel ox x NCW blocks of 32 couts (from cb0).  The caller has dropped the
// lanes whose column lies past the map.
template <int R, int NCW, int RS>
__device__ __forceinline__ void plain_epilogue(const esr_conv& p, Acc8& acc, int b, int cb0, int h, int oyb, int ox) {
  const bool relu = p.act == ESR_ACT_RELU;
  const float slope = p.act == ESR_ACT_LRELU ? ESR_LRELU_SLOPE : 1.f;
  const int nrows = (p.H - oyb + RS - 1) / RS;          // rows of this wave inside the map (<= 0: none)
  f32x4 bq[NCW][4];
#pragma unroll
  for (int cw = 0; cw < NCW; ++cw)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      bq[cw][i] = p.bias && cb0 + cw < p.cout_blocks ? *(const f32x4*)(p.bias + (cb0 + cw) * 32 + 16 * h + 4 * i)
                                                     : f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.nchw_out_c <= 0) {
    const int64_t row_bytes = (int64_t)RS * p.out.wp * 32;
    const int64_t pix = (int64_t)(oyb + 1) * p.out.wp + ox + 1;
    sfor<NCW>([&](auto CW) __attribute__((always_inline)) {
      constexpr int cw = decltype(CW)::value;
      const int cb = cb0 + cw;
      if (cb >= p.cout_blocks || 2 * cb >= p.out.ngroups) return;
      const bool g1 = 2 * cb + 1 < p.out.ngroups;
      char* const o0 = (char*)p.out.ptr + b * p.out.batch_stride + (int64_t)(2 * cb) * p.out.group_stride + pix * 32 + 16 * h;
      char* const o1 = o0 + p.out.group_stride;
      if (relu) plain_rows_g32<R, NCW, cw, true>(acc, bq[cw], slope, o0, o1, g1, row_bytes, nrows);
      else plain_rows_g32<R, NCW, cw, false>(acc, bq[cw], slope, o0, o1, g1, row_bytes, nrows);
    });
    return;
  }
  const int C = p.nchw_out_c;
  const int64_t plane_bytes = (int64_t)p.H * p.W * 4;
  const uint32_t row_bytes = (uint32_t)(RS * p.W) * 4u;
  const uint32_t voff0 = (uint32_t)(oyb * p.W + ox) * 4u;   // inside one plane: below 2^28 (esr_conv_forward's limit on `in`)
  sfor<NCW>([&](auto CW) __attribute__((always_inline)) {
    constexpr int cw = decltype(CW)::value;
    const int cb = cb0 + cw;
    if (cb >= p.cout_blocks) return;
#pragma unroll 1
    for (int hh = 0; hh < 2; ++hh) {
      const int c0 = cb * 32 + 16 * hh, n = C - c0;     // channels of this half-wave that exist (wave-uniform)
      if (n <= 0) break;
      if (h != hh) continue;
      char* const base = (char*)p.nchw_out + ((int64_t)b * C + c0) * plane_bytes;
      uint32_t voff = voff0;
      sfor<R>([&](auto RR) __attribute__((always_inline)) {
        constexpr int r = decltype(RR)::value;
        if (r >= nrows) return;
        const f32x16 a = accsel<r * NCW + cw>(acc);
        sfor<16>([&](auto EE) __attribute__((always_inline)) {
          constexpr int e = decltype(EE)::value;
          if (e >= n) return;
          const float x = a[e] + bq[cw][e >> 2][e & 3];
          *(float*)(base + e * plane_bytes + voff) = relu ? fmaxf(x, 0.f) : fmaxf(x, x * slope);
        });
        voff += row_bytes;
      });
    }
  });
}

}  // namespace
