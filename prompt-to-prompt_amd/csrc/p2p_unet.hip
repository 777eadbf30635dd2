// U-Net glue between the convolutions and GEMMs (bandwidth-bound, no MFMA): GroupNorm with the
// per-channel adds in front of it and SiLU behind it, the residual add with its conv biases, and
// GEGLU.  16-bit I/O (bf16 or f16), f32 arithmetic, one rounding at the store; every reduction
// runs in a fixed order (no atomics), so two launches on the same input are bit-identical.
//
// GroupNorm is two launches (three for the VAE's large slabs, below): gn_stats_kernel reads each (n, group) slab twice -- mean, then the
// centred sum of squares; the second sweep of the <= 245 KB slab hits the L2 -- and leaves
// {mean, rstd} in a caller-owned workspace; the apply kernel is then tiled freely over the whole
// tensor (the slab count n x groups says nothing about its grid), which is what lets the
// token-major store go through an LDS transpose with 128-byte runs per pixel.
//
// Slabs of kGnStatsSplit elements or more (p2p_kernels.h; the VAE's, up to 2 M elements with as few as
// 32 slabs per launch) take the split form instead: gn_stats_split_kernel runs one workgroup per
// chunk of a slab -- gn_stats_chunks(slab) equal chunks, a function of the slab size only -- and
// leaves {count, mean, M2} per chunk behind the {mean, rstd} pairs of the workspace;
// gn_stats_combine_kernel then folds each slab's partials in chunk order with Chan's formula.  No
// atomics, the same order on every launch: bit-identical from launch to launch as well.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {
namespace {

typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;

template <bool F16>
__device__ __forceinline__ float ld16(uint16_t b) {
  return F16 ? h2f(b) : bf2f(b);
}
template <bool F16>
__device__ __forceinline__ uint16_t st16(float x) {
  return F16 ? f2h(x) : f2bf(x);
}

__device__ __forceinline__ float silu(float x) { return x / (1.f + __expf(-x)); }

// sum over the workgroup, the same value in every thread: xor-shuffles inside a wave, then the
// waves' partials in wave order
__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

// one workgroup per (n, group): the slab x[n, g*cpg .. (g+1)*cpg, :] is contiguous, L = cpg*hw
template <bool F16>
__global__ void gn_stats_kernel(p2p_group_norm_args a) {
  __shared__ float red[16];
  const int G = a.groups, C = a.channels, cpg = C / G;
  const int n = blockIdx.x / G, g = blockIdx.x - n * G;
  const int hwv = a.hw >> 3;
  const int nv = cpg * hwv;
  const int64_t row0 = (int64_t)n * C + g * cpg;
  const u16x8_t* x = reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.x) + row0 * a.hw);
  const uint16_t* add = static_cast<const uint16_t*>(a.chan_add);
  const uint16_t* bias = static_cast<const uint16_t*>(a.chan_bias);
  if (add) add += (int64_t)n * a.chan_add_stride + g * cpg;
  if (bias) bias += g * cpg;
  const bool shifted = add || bias;
  auto chan_shift = [&](int iv) {
    const int c = iv / hwv;
    return (add ? ld16<F16>(add[c]) : 0.f) + (bias ? ld16<F16>(bias[c]) : 0.f);
  };
  float s = 0.f;
  for (int iv = threadIdx.x; iv < nv; iv += blockDim.x) {
    const u16x8_t v = x[iv];
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) t += ld16<F16>(v[j]);
    if (shifted) t += 8.f * chan_shift(iv);
    s += t;
  }
  const float inv_l = 1.f / ((float)cpg * (float)a.hw);
  const float mean = block_sum(s, red) * inv_l;
  float q = 0.f;
  for (int iv = threadIdx.x; iv < nv; iv += blockDim.x) {
    const u16x8_t v = x[iv];
    const float m = shifted ? mean - chan_shift(iv) : mean;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = ld16<F16>(v[j]) - m;
      q += d * d;
    }
  }
  const float var = block_sum(q, red) * inv_l;
  if (threadIdx.x == 0) {
    a.stats[2 * blockIdx.x] = mean;
    a.stats[2 * blockIdx.x + 1] = 1.f / sqrtf(var + a.eps);
  }
}

// one workgroup per (slab, chunk): the chunk's count, mean and centred sum of squares (two sweeps
// of <= 64 KB), to part[(slab * chunks + chunk) * 3 ..]
template <bool F16>
__global__ __launch_bounds__(1024) void gn_stats_split_kernel(p2p_group_norm_args a, int chunks, int vpc) {
  __shared__ float red[16];
  const int G = a.groups, C = a.channels, cpg = C / G;
  const int slab_id = blockIdx.x / chunks, chunk = blockIdx.x - slab_id * chunks;
  const int n = slab_id / G, g = slab_id - n * G;
  const int hwv = a.hw >> 3;
  const int nv = cpg * hwv;
  const int v0 = chunk * vpc;
  const int v1 = min(nv, v0 + vpc);
  const int64_t row0 = (int64_t)n * C + g * cpg;
  const u16x8_t* x = reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.x) + row0 * a.hw);
  const uint16_t* add = static_cast<const uint16_t*>(a.chan_add);
  const uint16_t* bias = static_cast<const uint16_t*>(a.chan_bias);
  if (add) add += (int64_t)n * a.chan_add_stride + g * cpg;
  if (bias) bias += g * cpg;
  const bool shifted = add || bias;
  auto chan_shift = [&](int iv) {
    const int c = iv / hwv;
    return (add ? ld16<F16>(add[c]) : 0.f) + (bias ? ld16<F16>(bias[c]) : 0.f);
  };
  const float cnt = 8.f * (float)max(v1 - v0, 0);
  float s = 0.f;
  for (int iv = v0 + threadIdx.x; iv < v1; iv += blockDim.x) {
    const u16x8_t v = x[iv];
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) t += ld16<F16>(v[j]);
    if (shifted) t += 8.f * chan_shift(iv);
    s += t;
  }
  const float mean = cnt > 0.f ? block_sum(s, red) / cnt : 0.f;
  float q = 0.f;
  for (int iv = v0 + threadIdx.x; iv < v1; iv += blockDim.x) {
    const u16x8_t v = x[iv];
    const float m = shifted ? mean - chan_shift(iv) : mean;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = ld16<F16>(v[j]) - m;
      q += d * d;
    }
  }
  const float m2 = block_sum(q, red);
  if (threadIdx.x == 0) {
    float* const part = a.stats + 2 * (int64_t)a.n * G + (int64_t)blockIdx.x * 3;
    part[0] = cnt;
    part[1] = mean;
    part[2] = m2;
  }
}

// one thread per slab: Chan's pairwise update over the chunks, in chunk order
__global__ __launch_bounds__(256) void gn_stats_combine_kernel(p2p_group_norm_args a, int chunks) {
  const int slab_id = blockIdx.x * 256 + threadIdx.x;
  const int slabs = a.n * a.groups;
  if (slab_id >= slabs) return;
  const float* part = a.stats + 2 * (int64_t)slabs + (int64_t)slab_id * chunks * 3;
  float cnt = 0.f, mean = 0.f, m2 = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float nb = part[3 * c], mb = part[3 * c + 1], qb = part[3 * c + 2];
    if (nb == 0.f) continue;
    const float tot = cnt + nb;
    const float delta = mb - mean;
    mean += delta * (nb / tot);
    m2 += qb + delta * delta * (cnt * (nb / tot));
    cnt = tot;
  }
  a.stats[2 * slab_id] = mean;
  a.stats[2 * slab_id + 1] = 1.f / sqrtf(m2 / cnt + a.eps);
}

// what one channel of one batch entry needs: y = ((x + shift) - mean) * rstd * gamma + beta
struct ChanCoef {
  float shift, mean, rstd, gamma, beta;
};

template <bool F16>
__device__ __forceinline__ ChanCoef chan_coef(const p2p_group_norm_args& a, int n, int c) {
  const uint16_t* add = static_cast<const uint16_t*>(a.chan_add);
  const uint16_t* bias = static_cast<const uint16_t*>(a.chan_bias);
  const int g = c / (a.channels / a.groups);
  ChanCoef k;
  k.shift = (add ? ld16<F16>(add[(int64_t)n * a.chan_add_stride + c]) : 0.f) + (bias ? ld16<F16>(bias[c]) : 0.f);
  k.mean = a.stats[2 * (n * a.groups + g)];
  k.rstd = a.stats[2 * (n * a.groups + g) + 1];
  k.gamma = ld16<F16>(static_cast<const uint16_t*>(a.gamma)[c]);
  k.beta = ld16<F16>(static_cast<const uint16_t*>(a.beta)[c]);
  return k;
}

template <bool F16, bool SILU>
__device__ __forceinline__ u16x8_t gn_apply8(u16x8_t v, const ChanCoef& k) {
  u16x8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float y = ((ld16<F16>(v[j]) + k.shift) - k.mean) * k.rstd * k.gamma + k.beta;
    if (SILU) y = silu(y);
    o[j] = st16<F16>(y);
  }
  return o;
}

// NCHW -> NCHW: one 8-element vector per thread, vectors never straddle a channel (hw % 8 == 0)
template <bool F16, bool SILU>
__global__ __launch_bounds__(256) void gn_apply_nchw_kernel(p2p_group_norm_args a, int64_t n_vec) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int hwv = a.hw >> 3;
  const int64_t row = iv / hwv;              // n * C + c
  const int n = (int)(row / a.channels), c = (int)(row - (int64_t)n * a.channels);
  const ChanCoef k = chan_coef<F16>(a, n, c);
  const u16x8_t v = static_cast<const u16x8_t*>(a.x)[iv];
  static_cast<u16x8_t*>(a.y)[iv] = gn_apply8<F16, SILU>(v, k);
}

// 64 channels x 64 pixels per workgroup through LDS; rows of kTileLd elements keep every
// 16-byte row segment aligned and spread the transposed 2-byte accesses over the banks
constexpr int kTile = 64;
constexpr int kTileLd = kTile + 8;

// NCHW -> token-major [n, hw, C]: loads run along the pixels of a channel, stores along the
// channels of a pixel (128 contiguous bytes per pixel and tile).  grid (hw tiles, C tiles, n)
template <bool F16, bool SILU>
__global__ __launch_bounds__(256) void gn_apply_tok_kernel(p2p_group_norm_args a) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTile * kTileLd];   // [pixel][channel]
  const int p0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile, n = blockIdx.z;
  const int C = a.channels, hw = a.hw;
  const uint16_t* x = static_cast<const uint16_t*>(a.x) + (int64_t)n * C * hw;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int ch = v >> 3, p = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw) {
      const ChanCoef kc = chan_coef<F16>(a, n, c0 + ch);
      const u16x8_t in = *reinterpret_cast<const u16x8_t*>(x + (int64_t)(c0 + ch) * hw + p0 + p);
      const u16x8_t o = gn_apply8<F16, SILU>(in, kc);
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[(p + j) * kTileLd + ch] = o[j];
    }
  }
  __syncthreads();
  uint16_t* y = static_cast<uint16_t*>(a.y) + (int64_t)n * hw * C;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int p = v >> 3, ch = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw)
      *reinterpret_cast<u16x8_t*>(y + (int64_t)(p0 + p) * C + c0 + ch) =
          *reinterpret_cast<const u16x8_t*>(&tile[p * kTileLd + ch]);
  }
}

template <bool F16>
__device__ __forceinline__ float bias_of(const p2p_bias_residual_args& a, int c) {
  const uint16_t* b1 = static_cast<const uint16_t*>(a.bias);
  const uint16_t* b2 = static_cast<const uint16_t*>(a.bias2);
  return (b1 ? ld16<F16>(b1[c]) : 0.f) + (b2 ? ld16<F16>(b2[c]) : 0.f);
}

// out = a + b + bias, all NCHW
template <bool F16>
__global__ __launch_bounds__(256) void bias_residual_nchw_kernel(p2p_bias_residual_args a, int64_t n_vec) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int c = (int)((iv / (a.hw >> 3)) % a.channels);
  const float bias = bias_of<F16>(a, c);
  const u16x8_t va = static_cast<const u16x8_t*>(a.a)[iv];
  const u16x8_t vb = static_cast<const u16x8_t*>(a.b)[iv];
  u16x8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = st16<F16>(ld16<F16>(va[j]) + ld16<F16>(vb[j]) + bias);
  static_cast<u16x8_t*>(a.out)[iv] = o;
}

// out (NCHW) = a (NCHW) + b (token-major [n, hw, C]) + bias: b's tile is read along the channels
// and transposed through LDS.  grid (hw tiles, C tiles, n)
template <bool F16>
__global__ __launch_bounds__(256) void bias_residual_tok_kernel(p2p_bias_residual_args a) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTile * kTileLd];   // [pixel][channel]
  const int p0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile, n = blockIdx.z;
  const int C = a.channels, hw = a.hw;
  const uint16_t* b = static_cast<const uint16_t*>(a.b) + (int64_t)n * hw * C;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int p = v >> 3, ch = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw)
      *reinterpret_cast<u16x8_t*>(&tile[p * kTileLd + ch]) =
          *reinterpret_cast<const u16x8_t*>(b + (int64_t)(p0 + p) * C + c0 + ch);
  }
  __syncthreads();
  const int64_t base = (int64_t)n * C * hw;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int ch = v >> 3, p = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw) {
      const float bias = bias_of<F16>(a, c0 + ch);
      const int64_t off = base + (int64_t)(c0 + ch) * hw + p0 + p;
      const u16x8_t va = *reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.a) + off);
      u16x8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = st16<F16>(ld16<F16>(va[j]) + ld16<F16>(tile[(p + j) * kTileLd + ch]) + bias);
      *reinterpret_cast<u16x8_t*>(static_cast<uint16_t*>(a.out) + off) = o;
    }
  }
}

// out[m, j] = in[m, j] * gelu(in[m, d + j]), exact erf form
template <bool F16>
__global__ __launch_bounds__(256) void geglu_kernel(p2p_geglu_args a, int64_t n_vec) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int dv = a.d >> 3;
  const int64_t m = iv / dv;
  const int j = (int)(iv - m * dv) * 8;
  const uint16_t* row = static_cast<const uint16_t*>(a.in) + m * a.in_row_stride;
  const u16x8_t h = *reinterpret_cast<const u16x8_t*>(row + j);
  const u16x8_t g = *reinterpret_cast<const u16x8_t*>(row + a.d + j);
  u16x8_t o;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float gate = ld16<F16>(g[i]);
    const float gelu = 0.5f * gate * (1.f + erff(gate * 0.70710678118654752f));
    o[i] = st16<F16>(ld16<F16>(h[i]) * gelu);
  }
  *reinterpret_cast<u16x8_t*>(static_cast<uint16_t*>(a.out) + m * a.out_row_stride + j) = o;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool io16(int dtype) { return dtype == P2P_DTYPE_BF16 || dtype == P2P_DTYPE_F16; }

template <bool F16>
void launch_group_norm(const p2p_group_norm_args& a, hipStream_t st) {
  // a slab of at least kGnStatsWide elements takes 1024 threads, a smaller one 256
  const int64_t slab = (int64_t)(a.channels / a.groups) * a.hw;
  const int chunks = gn_stats_chunks(slab);
  if (chunks > 1) {
    const int nv = (int)(slab / 8);
    const int vpc = (nv + chunks - 1) / chunks;   // 8-element vectors per chunk (the last may hold fewer)
    launch_kernel(gn_stats_split_kernel<F16>, dim3((unsigned)(a.n * a.groups * chunks)), dim3(1024), 0, st, a, chunks,
                  vpc);
    launch_kernel(gn_stats_combine_kernel, dim3((unsigned)((a.n * a.groups + 255) / 256)), dim3(256), 0, st, a, chunks);
  } else {
    launch_kernel(gn_stats_kernel<F16>, dim3((unsigned)(a.n * a.groups)), dim3(slab >= kGnStatsWide ? 1024 : 256), 0,
                  st, a);
  }
  const bool act = a.act == P2P_ACT_SILU;
  if (a.y_layout == P2P_LAYOUT_NCHW) {
    const int64_t n_vec = (int64_t)a.n * a.channels * a.hw / 8;
    const dim3 grid((unsigned)((n_vec + 255) / 256));
    if (act) launch_kernel((gn_apply_nchw_kernel<F16, true>), grid, dim3(256), 0, st, a, n_vec);
    else launch_kernel((gn_apply_nchw_kernel<F16, false>), grid, dim3(256), 0, st, a, n_vec);
  } else {
    const dim3 grid((a.hw + kTile - 1) / kTile, (a.channels + kTile - 1) / kTile, a.n);
    if (act) launch_kernel((gn_apply_tok_kernel<F16, true>), grid, dim3(256), 0, st, a);
    else launch_kernel((gn_apply_tok_kernel<F16, false>), grid, dim3(256), 0, st, a);
  }
}

template <bool F16>
void launch_bias_residual(const p2p_bias_residual_args& a, hipStream_t st) {
  if (a.b_layout == P2P_LAYOUT_NCHW) {
    const int64_t n_vec = (int64_t)a.n * a.channels * a.hw / 8;
    launch_kernel(bias_residual_nchw_kernel<F16>, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, st, a, n_vec);
  } else {
    const dim3 grid((a.hw + kTile - 1) / kTile, (a.channels + kTile - 1) / kTile, a.n);
    launch_kernel(bias_residual_tok_kernel<F16>, grid, dim3(256), 0, st, a);
  }
}

}  // namespace

int run_group_norm(const p2p_group_norm_args& a, hipStream_t st) {
  if (!a.x || !a.gamma || !a.beta || !a.y || !a.stats) return P2P_E_ARG;
  if (a.n < 1 || a.channels < 1 || a.hw < 1 || a.groups < 1 || a.channels % a.groups) return P2P_E_ARG;
  if (a.n > 65535 || (int64_t)a.n * a.groups > INT32_MAX / 2) return P2P_E_ARG;
  // the statistics kernels index a slab's 8-element vectors, and the split form's grid, in 32 bits
  if ((int64_t)(a.channels / a.groups) * a.hw > INT32_MAX ||
      (int64_t)a.n * a.groups * gn_stats_chunks((int64_t)(a.channels / a.groups) * a.hw) > INT32_MAX / 4)
    return P2P_E_ARG;
  if (a.chan_add && a.chan_add_stride != 0 && a.chan_add_stride != a.channels) return P2P_E_ARG;
  if (a.act != P2P_ACT_NONE && a.act != P2P_ACT_SILU) return P2P_E_ARG;
  if (a.y_layout != P2P_LAYOUT_NCHW && a.y_layout != P2P_LAYOUT_TOKENS) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  // 16-byte vectors along the pixels (and, token-major, along the channels)
  if (a.hw % 8 || (a.y_layout == P2P_LAYOUT_TOKENS && a.channels % 8)) return P2P_E_ALIGN;
  if (!aligned16(a.x) || !aligned16(a.y) || ((uintptr_t)a.stats & 3)) return P2P_E_ALIGN;
  if (a.dtype == P2P_DTYPE_F16) launch_group_norm<true>(a, st);
  else launch_group_norm<false>(a, st);
  return (int)hipGetLastError();
}

int run_bias_residual(const p2p_bias_residual_args& a, hipStream_t st) {
  if (!a.a || !a.b || !a.out) return P2P_E_ARG;
  if (a.n < 1 || a.channels < 1 || a.hw < 1 || a.n > 65535) return P2P_E_ARG;
  if (a.b_layout != P2P_LAYOUT_NCHW && a.b_layout != P2P_LAYOUT_TOKENS) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.hw % 8 || (a.b_layout == P2P_LAYOUT_TOKENS && a.channels % 8)) return P2P_E_ALIGN;
  if (!aligned16(a.a) || !aligned16(a.b) || !aligned16(a.out)) return P2P_E_ALIGN;
  if (a.dtype == P2P_DTYPE_F16) launch_bias_residual<true>(a, st);
  else launch_bias_residual<false>(a, st);
  return (int)hipGetLastError();
}

int run_geglu(const p2p_geglu_args& a, hipStream_t st) {
  if (!a.in || !a.out) return P2P_E_ARG;
  if (a.rows < 1 || a.d < 1 || a.in_row_stride < 2 * (int64_t)a.d || a.out_row_stride < a.d) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.d % 8 || a.in_row_stride % 8 || a.out_row_stride % 8) return P2P_E_ALIGN;
  if (!aligned16(a.in) || !aligned16(a.out)) return P2P_E_ALIGN;
  const int64_t n_vec = (int64_t)a.rows * (a.d / 8);
  if ((n_vec + 255) / 256 > INT32_MAX) return P2P_E_ARG;
  const dim3 grid((unsigned)((n_vec + 255) / 256));
  if (a.dtype == P2P_DTYPE_F16) launch_kernel(geglu_kernel<true>, grid, dim3(256), 0, st, a, n_vec);
  else launch_kernel(geglu_kernel<false>, grid, dim3(256), 0, st, a, n_vec);
  return (int)hipGetLastError();
}

}  // namespace p2p
