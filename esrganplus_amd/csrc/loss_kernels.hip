// loss_kernels.hip — the losses of the ESRGAN+ train step (SRRaGAN_model.py:124-137,150-156) with their gradients, one
// launch each:  L1Loss / MSELoss (nn.L1Loss, nn.MSELoss: cri_pix, cri_fea 'l1' / 'l2') and the relativistic-average
// GAN term  ( BCEWithLogits(x - mean(y), tx) + BCEWithLogits(y - mean(x), ty) ) / 2  (GANLoss 'vanilla',
// loss.py:6-38).  As torch ops these are ~70 tiny dependent launches per step (sub, abs, mean, sigmoid, ...,
// and their backward) — more chip time in launch gaps than in arithmetic.  HBM-bound, tiny.
#include "common.h"

namespace {

// L2 = false: loss = weight * mean|a - b| ; grad_a = weight * sign(a - b) / n                     (nn.L1Loss)
// L2 = true:  loss = weight * mean (a - b)^2 ; grad_a = weight * 2 (a - b) / n                    (nn.MSELoss)
// One pass; the last workgroup to arrive turns the fp64 sum into the loss and clears the scratch for the next call.
// L2: d = a - b is formed in fp32 and squared in fp64 (exact there: 24 x 24 bits), so a |d| up to fp32's largest still
// sums without overflow; the gradient's factor is ((2 weight / n) grad_scale) scale_dev, three roundings, times d.
template <bool L2>
__global__ __launch_bounds__(256) void pixel_loss_kernel(const esr_l1_loss p) {
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  double s = 0.0;
  const float gw = (L2 ? 2.f * p.weight : p.weight) / (float)p.n * (p.grad_scale != 0.f ? p.grad_scale : 1.f) * (p.grad_scale_dev ? *p.grad_scale_dev : 1.f);
  // 16-byte vector accesses only when all three pointers allow them (a view with an odd storage offset takes the
  // scalar path: same sums, same order per thread)
  const bool vec = (((uintptr_t)p.a | (uintptr_t)p.b | (uintptr_t)p.grad_a) & 15) == 0;
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < p.n; i0 += stride) {
    if (vec && i0 + 4 <= p.n) {
      const f32x4 a = *(const f32x4*)(p.a + i0), b = *(const f32x4*)(p.b + i0);
      f32x4 g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = a[e] - b[e];
        if (L2) {
          s += (double)d * (double)d;
          g[e] = gw * d;
        } else {
          s += fabsf(d);
          g[e] = d > 0.f ? gw : (d < 0.f ? -gw : 0.f);
        }
      }
      if (p.grad_a) *(f32x4*)(p.grad_a + i0) = g;
    } else {
      for (int64_t i = i0; i < p.n && i < i0 + 4; ++i) {
        const float d = p.a[i] - p.b[i];
        if (L2) {
          s += (double)d * (double)d;
          if (p.grad_a) p.grad_a[i] = gw * d;
        } else {
          s += fabsf(d);
          if (p.grad_a) p.grad_a[i] = d > 0.f ? gw : (d < 0.f ? -gw : 0.f);
        }
      }
    }
  }
  __shared__ double red[4];
  __shared__ bool last;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(p.scratch, red[0] + red[1] + red[2] + red[3]);
    __threadfence();
    const unsigned long long t = atomicAdd((unsigned long long*)(p.scratch + 1), 1ull);
    last = t == (unsigned long long)gridDim.x - 1;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    const double tot = atomicAdd(p.scratch, 0.0);
    *p.loss = (float)(tot / (double)p.n) * p.weight;
    p.scratch[0] = 0.0;
    *(unsigned long long*)(p.scratch + 1) = 0ull;
  }
}

__device__ __forceinline__ float softplus(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

// one workgroup; n logits per side (the discriminator's outputs: 16 per GPU).
// p.mode (data-parallel runs keep the batch means GLOBAL, SRRaGAN_model.py:136-137,151-152 — the two tiny sums
// cross the ranks between launches of this kernel, esrganplus_amd/losses.py):
//   0  everything from the local batch: means, loss, gradients                         (one GPU)
//   1  sums[0..1] = {sum x, sum y}                                                      (-> all-reduce with n)
//   2  means = ext[0] / ext[2], ext[1] / ext[2]: loss, mean_x/y, bce_x/y, sums[0..1] = {sum (sigmoid(z1) - tx),
//      sum (sigmoid(z2) - ty)} over the local batch                                     (-> all-reduce)
//   3  gradients from the global means and ext[3..4] = those two sums over ALL ranks, ext[2] = global n
__global__ __launch_bounds__(256) void ragan_loss_kernel(const esr_ragan_loss p) {
  __shared__ float red[4][4];
  auto block_sum4 = [&](float v0, float v1, float v2, float v3, float* out) {
    float v[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    for (int k = 0; k < 4; ++k) out[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  };
  const float inv = 1.f / (float)p.n;
  float mx, my, ninv_glob = inv;
  if (p.mode == 0 || p.mode == 1) {
    float sx = 0.f, sy = 0.f;
    for (int i = threadIdx.x; i < p.n; i += 256) { sx += p.x[i]; sy += p.y[i]; }
    float m[4];
    block_sum4(sx, sy, 0.f, 0.f, m);
    if (p.mode == 1) {
      if (threadIdx.x == 0) { p.sums[0] = m[0]; p.sums[1] = m[1]; }
      return;
    }
    mx = m[0] * inv; my = m[1] * inv;
  } else {
    ninv_glob = 1.f / p.ext[2];
    mx = p.ext[0] * ninv_glob; my = p.ext[1] * ninv_glob;
  }
  // z1 = x - mean(y) against tx, z2 = y - mean(x) against ty
  const float hw = 0.5f * p.weight;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.mode != 3) {
    float l1 = 0.f, l2 = 0.f, d1 = 0.f, d2 = 0.f;
    for (int i = threadIdx.x; i < p.n; i += 256) {
      const float z1 = p.x[i] - my, z2 = p.y[i] - mx;
      l1 += softplus(z1) - p.tx * z1;
      l2 += softplus(z2) - p.ty * z2;
      d1 += sigmoidf(z1) - p.tx;
      d2 += sigmoidf(z2) - p.ty;
    }
    block_sum4(l1, l2, d1, d2, t);
    if (threadIdx.x == 0) {
      *p.loss = hw * (t[0] + t[1]) * inv;
      if (p.mean_x) *p.mean_x = mx;
      if (p.mean_y) *p.mean_y = my;
      if (p.bce_x) *p.bce_x = t[0] * inv;
      if (p.bce_y) *p.bce_y = t[1] * inv;
      if (p.mode == 2) { p.sums[0] = t[2]; p.sums[1] = t[3]; }
    }
    if (p.mode == 2) return;
  } else {
    t[2] = p.ext[3]; t[3] = p.ext[4];
  }
  // d loss / d x_i = hw/n [ (sigmoid(z1_i) - tx) - (sum_j (sigmoid(z2_j) - ty)) / N ]: the second term is the mean's share
  // (N and the sum run over all ranks in mode 3 — every rank's loss sees the mean, gradients are averaged over ranks)
  const float gs = hw * inv * (p.grad_scale != 0.f ? p.grad_scale : 1.f) * (p.grad_scale_dev ? *p.grad_scale_dev : 1.f);
  for (int i = threadIdx.x; i < p.n; i += 256) {
    const float z1 = p.x[i] - my, z2 = p.y[i] - mx;
    if (p.grad_x) p.grad_x[i] = gs * ((sigmoidf(z1) - p.tx) - t[3] * ninv_glob);
    if (p.grad_y) p.grad_y[i] = gs * ((sigmoidf(z2) - p.ty) - t[2] * ninv_glob);
  }
}

// GANLoss.forward (loss.py:6-38) on one or two operands, the standard-GAN step's criterion (SRGAN_model.py:129-146):
//   kind 0 (vanilla)  l(x, t) = mean_i [ max(x_i, 0) - x_i t + log1p(exp(-|x_i|)) ]   d/dx_i = (sigmoid(x_i) - t) / n
//   kind 1 (lsgan)    l(x, t) = mean_i (x_i - t)^2                                      d/dx_i = 2 (x_i - t) / n
// loss = weight * (l(x, tx) [+ l(y, ty)]); the gradients carry weight * grad_scale [* grad_scale_dev[0]].  One
// workgroup (n is the discriminator's batch); the elements are formed in fp32, their sums run in fp64 (lsgan: the
// square too, exact there).  exp(-|x|) <= 1 and the sigmoid is formed from it on either side of 0: nothing overflows.
// No scratch: every output is written once, by thread 0.
template <bool LS>
__global__ __launch_bounds__(256) void gan_loss_kernel(const esr_gan_loss p) {
  __shared__ double red[4][4];
  const float kw = LS ? 2.f * p.weight : p.weight;
  const float gs = p.grad_scale != 0.f ? p.grad_scale : 1.f, gsd = p.grad_scale_dev ? *p.grad_scale_dev : 1.f;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};          // sum l(x_i), sum x_i, sum l(y_i), sum y_i
  for (int side = 0; side < 2; ++side) {
    const float* v = side ? p.y : p.x;
    if (!v) continue;
    const int n = side ? p.n_y : p.n_x;
    const float t = side ? p.ty : p.tx;
    float* g = side ? p.grad_y : p.grad_x;
    const float gw = kw / (float)n * gs * gsd;
    double l = 0.0, s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float x = v[i];
      s += x;
      if (LS) {
        const float d = x - t;
        l += (double)d * (double)d;
        if (g) g[i] = gw * d;
      } else {
        const float e = expf(-fabsf(x));
        l += fmaxf(x, 0.f) - x * t + log1pf(e);
        if (g) g[i] = gw * ((x >= 0.f ? 1.f : e) / (1.f + e) - t);
      }
    }
    acc[2 * side] = l;
    acc[2 * side + 1] = s;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = acc[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot[4];
    for (int k = 0; k < 4; ++k) tot[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    const double lx = tot[0] / (double)p.n_x, ly = p.y ? tot[2] / (double)p.n_y : 0.0;
    *p.loss = (float)(lx + ly) * p.weight;
    if (p.term_x) *p.term_x = (float)lx;
    if (p.term_y) *p.term_y = (float)ly;
    if (p.mean_x) *p.mean_x = (float)(tot[1] / (double)p.n_x);
    if (p.mean_y) *p.mean_y = p.y ? (float)(tot[3] / (double)p.n_y) : 0.f;
  }
}

}  // namespace

template <bool L2>
static int pixel_loss_launch(const esr_l1_loss* p, esr_stream_t stream, const char* entry, const char* kernel) {
  if (!p || !p->a || !p->b || !p->loss || !p->scratch || p->n <= 0) {
    esr_set_error("%s: invalid arguments", entry);
    return ESR_ERR_INVALID;
  }
  int64_t wgs = (p->n + 4095) / 4096;           // 16 elements per thread
  if (wgs > 1024) wgs = 1024;
  hipLaunchKernelGGL(pixel_loss_kernel<L2>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, *p);
  return esr_check_launch(kernel);
}

extern "C" int esr_l1_loss_forward(const esr_l1_loss* p, esr_stream_t stream) {
  return pixel_loss_launch<false>(p, stream, "esr_l1_loss_forward", "l1_loss_kernel");
}

extern "C" int esr_l2_loss_forward(const esr_l1_loss* p, esr_stream_t stream) {
  return pixel_loss_launch<true>(p, stream, "esr_l2_loss_forward", "l2_loss_kernel");
}

extern "C" int esr_ragan_loss_forward(const esr_ragan_loss* p, esr_stream_t stream) {
  if (!p || !p->x || !p->y || p->n <= 0 || p->mode < 0 || p->mode > 3 || ((p->mode == 0 || p->mode == 2) && !p->loss) ||
      ((p->mode == 1 || p->mode == 2) && !p->sums) || (p->mode >= 2 && !p->ext)) {
    esr_set_error("esr_ragan_loss_forward: invalid arguments");
    return ESR_ERR_INVALID;
  }
  hipLaunchKernelGGL(ragan_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *p);
  return esr_check_launch("ragan_loss_kernel");
}

extern "C" int esr_gan_loss_forward(const esr_gan_loss* p, esr_stream_t stream) {
  if (!p || !p->x || p->n_x < 1 || (p->y && p->n_y < 1) || (p->kind != 0 && p->kind != 1) || !p->loss) {
    esr_set_error("esr_gan_loss_forward: invalid arguments");
    return ESR_ERR_INVALID;
  }
  if (p->kind == 1)
    hipLaunchKernelGGL(gan_loss_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(gan_loss_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, *p);
  return esr_check_launch("gan_loss_kernel");
}
