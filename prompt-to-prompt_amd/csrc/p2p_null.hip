// Batched null-text inversion (null_text.py:574-606 for B images at once): the per-image loss with
// its gradient, and a per-image gated Adam step with the early stop of null_text.py:597 taken on
// the device, so that one captured graph serves a batch in which some images have stopped.
//
// null_loss_kernel: one workgroup per image.  Per element, in f32 on the widened inputs,
//   eps = eps_u + g (eps_c - eps_u),  prev = c2 ((x - c0 eps) / c1) + c3 eps,  r = prev - target
// (the statements of DDIMScheduler.prev_step, in its order), grad = kg r with the one scalar
// kg = (2 / n) (1 - g) (c3 - c2 c0 / c1) formed in f64 (its two terms nearly cancel between
// neighbouring timesteps) and rounded to f32; the f32 product is rounded once to the eps dtype.
// loss = (sum r^2) / n: every thread adds its squares in f64 in element order, the 64 lanes of a
// wave are folded by a fixed butterfly, the four waves are added in wave order -- no atomics, and
// nothing depends on B or on where the image stands in the batch.  An inactive image gets its loss
// and a gradient of +0.
//
// null_adam_kernel + null_gate_kernel: torch.optim.Adam's update for every image whose flag is set
// at launch, then the flags.  The flag and the step count are read by every workgroup of an image,
// so they are not written by the kernel that reads them: p2p_null_adam launches a second, tiny
// kernel (one thread per image) behind the update, which advances step and steps_run and clears
// the flag where loss < threshold.  An inactive image is not touched by either.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {
namespace {

__device__ __forceinline__ f32x4_t load4(const float* p, int64_t iv) { return reinterpret_cast<const f32x4_t*>(p)[iv]; }
__device__ __forceinline__ f32x4_t load4(const uint16_t* p, int64_t iv) {
  const uint2 u = reinterpret_cast<const uint2*>(p)[iv];
  return f32x4_t{bf2f((uint16_t)(u.x & 0xffffu)), bf2f((uint16_t)(u.x >> 16)), bf2f((uint16_t)(u.y & 0xffffu)),
                 bf2f((uint16_t)(u.y >> 16))};
}
__device__ __forceinline__ void store4(float* p, int64_t iv, const f32x4_t& v) { reinterpret_cast<f32x4_t*>(p)[iv] = v; }
__device__ __forceinline__ void store4(uint16_t* p, int64_t iv, const f32x4_t& v) {
  uint2 u;
  u.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
  u.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
  reinterpret_cast<uint2*>(p)[iv] = u;
}

template <typename T>
__global__ __launch_bounds__(256) void null_loss_kernel(const T* __restrict__ eps_u, const T* __restrict__ eps_c,
                                                        const float* __restrict__ x, const float* __restrict__ target,
                                                        const float* __restrict__ coef, float g,
                                                        const uint8_t* __restrict__ active, float* __restrict__ loss,
                                                        T* __restrict__ grad, int n) {
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t base4 = (int64_t)b * (n / 4);
  const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3];
  const bool on = active[b] != 0;
  const float kg =
      on ? (float)((2.0 / (double)n) * (1.0 - (double)g) * ((double)c3 - (double)c2 * (double)c0 / (double)c1)) : 0.f;
  double acc = 0.0;
  for (int iv = tid; iv < n / 4; iv += 256) {
    const f32x4_t eu = load4(eps_u, base4 + iv), ec = load4(eps_c, base4 + iv);
    const f32x4_t xv = load4(x, base4 + iv), tv = load4(target, base4 + iv);
    f32x4_t gv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float eps = eu[j] + g * (ec[j] - eu[j]);
      const float x0 = (xv[j] - c0 * eps) / c1;
      const float prev = c2 * x0 + c3 * eps;
      const float r = prev - tv[j];
      acc += (double)r * (double)r;
      gv[j] = on ? kg * r : 0.f;   // (not kg * r with kg = 0: a NaN residual stays out of a stopped image)
    }
    store4(grad, base4 + iv, gv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) loss[b] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / (double)n);
}

// b^t for t >= 0 by squaring: a handful of f64 multiplies, the same in every thread
__device__ __forceinline__ double powi(double b, int t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// grid (ceil(m / 4 / 256), B).  torch.optim.Adam (single tensor, f32): the bias corrections in f64
// as torch forms them in Python floats, lr / (1 - beta1^t) and sqrt(1 - beta2^t) then used as f32
// scalars; 1 - beta1 and 1 - beta2 likewise formed in f64 and rounded.
__global__ __launch_bounds__(256) void null_adam_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                        const float* __restrict__ lr, const int32_t* __restrict__ step,
                                                        const uint8_t* __restrict__ active, int m4, double beta1,
                                                        double beta2, double eps) {
  const int b = blockIdx.y;
  const int iv = blockIdx.x * 256 + threadIdx.x;
  if (iv >= m4 || !active[b]) return;
  const int t = step[b] + 1;
  const float b1 = (float)beta1, b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float step_size = (float)((double)lr[0] / (1.0 - powi(beta1, t)));
  const float bc2_sqrt = (float)sqrt(1.0 - powi(beta2, t));
  const float e = (float)eps;
  const int64_t i = (int64_t)b * m4 + iv;
  const f32x4_t gv = load4(grad, i);
  f32x4_t mv = load4(exp_avg, i), vv = load4(exp_avg_sq, i), pv = load4(param, i);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mv[j] = b1 * mv[j] + omb1 * gv[j];
    vv[j] = b2 * vv[j] + omb2 * (gv[j] * gv[j]);
    const float denom = sqrtf(vv[j]) / bc2_sqrt + e;
    pv[j] = pv[j] - step_size * (mv[j] / denom);
  }
  store4(exp_avg, i, mv);
  store4(exp_avg_sq, i, vv);
  store4(param, i, pv);
}

__global__ __launch_bounds__(64) void null_gate_kernel(int32_t* __restrict__ step, int32_t* __restrict__ steps_run,
                                                       uint8_t* __restrict__ active, const float* __restrict__ loss,
                                                       const float* __restrict__ threshold, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B || !active[b]) return;
  step[b] += 1;
  steps_run[b] += 1;
  if (loss[b] < threshold[b]) active[b] = 0;
}

constexpr int kMaxImages = 65535;   // grid.y of the Adam launch

}  // namespace

int run_null_loss(const P2PNullLossArgs& a, hipStream_t st) {
  if (!a.eps_u || !a.eps_c || !a.x || !a.target || !a.coef || !a.active || !a.loss || !a.grad_eps_u) return P2P_E_ARG;
  if (a.B <= 0 || a.n <= 0) return P2P_E_ARG;
  if (a.eps_dtype != P2P_DTYPE_F32 && a.eps_dtype != P2P_DTYPE_BF16) return P2P_E_DTYPE;   // fp16 included
  if (a.B > kMaxImages) return P2P_E_BATCH;
  if (a.n % 4) return P2P_E_ALIGN;
  if (((uintptr_t)a.eps_u | (uintptr_t)a.eps_c | (uintptr_t)a.x | (uintptr_t)a.target | (uintptr_t)a.coef |
       (uintptr_t)a.grad_eps_u) & 15)
    return P2P_E_ALIGN;
  if ((uintptr_t)a.loss & 3) return P2P_E_ALIGN;
  // (four elements per access: 16 bytes of f32, 8 of bf16, and every image starts on such a boundary)
  if (a.eps_dtype == P2P_DTYPE_F32)
    launch_kernel(null_loss_kernel<float>, dim3((unsigned)a.B), dim3(256), 0, st, (const float*)a.eps_u,
                  (const float*)a.eps_c, a.x, a.target, a.coef, a.guidance, a.active, a.loss, (float*)a.grad_eps_u,
                  (int)a.n);
  else
    launch_kernel(null_loss_kernel<uint16_t>, dim3((unsigned)a.B), dim3(256), 0, st, (const uint16_t*)a.eps_u,
                  (const uint16_t*)a.eps_c, a.x, a.target, a.coef, a.guidance, a.active, a.loss,
                  (uint16_t*)a.grad_eps_u, (int)a.n);
  return (int)hipGetLastError();
}

int run_null_adam(const P2PNullAdamArgs& a, hipStream_t st) {
  if (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq || !a.lr || !a.step || !a.active || !a.loss ||
      !a.threshold || !a.steps_run)
    return P2P_E_ARG;
  if (a.B <= 0 || a.m <= 0) return P2P_E_ARG;
  if (!(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0) || !(a.eps >= 0.0)) return P2P_E_ARG;
  if (a.B > kMaxImages) return P2P_E_BATCH;
  if (a.m % 4) return P2P_E_ALIGN;
  if (((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) & 15) return P2P_E_ALIGN;
  if (((uintptr_t)a.lr | (uintptr_t)a.step | (uintptr_t)a.loss | (uintptr_t)a.threshold | (uintptr_t)a.steps_run) & 3)
    return P2P_E_ALIGN;
  const int m4 = a.m / 4;
  launch_kernel(null_adam_kernel, dim3((unsigned)((m4 + 255) / 256), (unsigned)a.B), dim3(256), 0, st, a.param, a.grad,
                a.exp_avg, a.exp_avg_sq, a.lr, (const int32_t*)a.step, (const uint8_t*)a.active, m4, a.beta1, a.beta2,
                a.eps);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  launch_kernel(null_gate_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a.step, a.steps_run, a.active,
                a.loss, a.threshold, (int)a.B);
  return (int)hipGetLastError();
}

}  // namespace p2p
