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

template <bool F16, typename Args>
__device__ __forceinline__ ChanCoef chan_coef(const Args& a, int n, int c) {
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

// ---- backward (with respect to the tensors only: x of GroupNorm, the input of GEGLU, the tokens
// of the residual).  GroupNorm, for y = act(xh * gamma + beta), xh = ((x + shift) - mean) * rstd:
//   g = dy * act'(z), gh = g * gamma, m1 = mean_slab(gh), m2 = mean_slab(gh * xh),
//   dx = rstd * (gh - m1 - xh * m2)
// in three launches.  The reduce kernels leave {sum g, sum g * xh} per (n, channel, part) -- one
// part per channel from NCHW dy, one per 64-pixel tile from token-major dy; the fold kernel (one
// wave per slab) weights them with gamma and leaves {m1, m2} behind the partials; the apply
// kernels recompute z and g from x and dy.  Every sum is taken inside one sample, in an order
// that (channels, hw, groups) fix: a sample's bits do not depend on n or on the other samples.

__device__ __forceinline__ float silu_grad(float z) {
  const float s = 1.f / (1.f + __expf(-z));
  return s * (1.f + z * (1.f - s));
}

// xh and g of eight elements of one channel
template <bool F16, bool SILU>
__device__ __forceinline__ void gn_bwd_g8(u16x8_t vx, u16x8_t vdy, const ChanCoef& k, float* xh, float* g) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xh[j] = ((ld16<F16>(vx[j]) + k.shift) - k.mean) * k.rstd;
    float gj = ld16<F16>(vdy[j]);
    if (SILU) gj *= silu_grad(xh[j] * k.gamma + k.beta);
    g[j] = gj;
  }
}

template <bool F16, bool SILU>
__device__ __forceinline__ u16x8_t gn_bwd_dx8(u16x8_t vx, u16x8_t vdy, const ChanCoef& k, float m1, float m2) {
  float xh[8], g[8];
  gn_bwd_g8<F16, SILU>(vx, vdy, k, xh, g);
  u16x8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = st16<F16>(k.rstd * ((g[j] * k.gamma - m1) - xh[j] * m2));
  return o;
}

// NCHW dy: T threads (one wave, or the four of a workgroup) per (n, channel) row of hw elements
template <bool F16, bool SILU, int T>
__global__ __launch_bounds__(256) void gn_bwd_reduce_nchw_kernel(p2p_group_norm_bwd_args a) {
  __shared__ float red[8];
  const int64_t rows = (int64_t)a.n * a.channels;
  const int64_t row = (int64_t)blockIdx.x * (256 / T) + threadIdx.x / T;
  const int lane = threadIdx.x % T;
  const int hwv = a.hw >> 3;
  float s1 = 0.f, s2 = 0.f;
  if (row < rows) {
    const int n = (int)(row / a.channels), c = (int)(row - (int64_t)n * a.channels);
    const ChanCoef k = chan_coef<F16>(a, n, c);
    const u16x8_t* x = reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.x) + row * a.hw);
    const u16x8_t* dy = reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.dy) + row * a.hw);
    for (int iv = lane; iv < hwv; iv += T) {
      float xh[8], g[8];
      gn_bwd_g8<F16, SILU>(x[iv], dy[iv], k, xh, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s1 += g[j];
        s2 += g[j] * xh[j];
      }
    }
  }
  for (int o = 32; o; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (T == 64) {
    if (lane == 0 && row < rows) {
      a.workspace[2 * row] = s1;
      a.workspace[2 * row + 1] = s2;
    }
  } else {   // one row per workgroup: the four waves' sums in wave order
    if ((threadIdx.x & 63) == 0) {
      red[2 * (threadIdx.x >> 6)] = s1;
      red[2 * (threadIdx.x >> 6) + 1] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0 && row < rows) {
      a.workspace[2 * row] = ((red[0] + red[2]) + red[4]) + red[6];
      a.workspace[2 * row + 1] = ((red[1] + red[3]) + red[5]) + red[7];
    }
  }
}

// token-major dy [n, hw, C]: the tile is loaded along the channels of a pixel and read back along
// the pixels of a channel, beside x; eight neighbouring lanes hold a channel's 64 pixels.
// grid (hw tiles, C tiles, n); partials [n, C, hw tiles, 2]
template <bool F16, bool SILU>
__global__ __launch_bounds__(256) void gn_bwd_reduce_tok_kernel(p2p_group_norm_bwd_args a) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTile * kTileLd];   // [pixel][channel]
  const int p0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile, n = blockIdx.z;
  const int C = a.channels, hw = a.hw;
  const uint16_t* dy = static_cast<const uint16_t*>(a.dy) + (int64_t)n * hw * C;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int p = v >> 3, ch = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw)
      *reinterpret_cast<u16x8_t*>(&tile[p * kTileLd + ch]) =
          *reinterpret_cast<const u16x8_t*>(dy + (int64_t)(p0 + p) * C + c0 + ch);
  }
  __syncthreads();
  const uint16_t* x = static_cast<const uint16_t*>(a.x) + (int64_t)n * C * hw;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int ch = v >> 3, p = (v & 7) * 8;
    float s1 = 0.f, s2 = 0.f;
    if (c0 + ch < C && p0 + p < hw) {
      const ChanCoef kc = chan_coef<F16>(a, n, c0 + ch);
      const u16x8_t vx = *reinterpret_cast<const u16x8_t*>(x + (int64_t)(c0 + ch) * hw + p0 + p);
      u16x8_t vdy;
#pragma unroll
      for (int j = 0; j < 8; ++j) vdy[j] = tile[(p + j) * kTileLd + ch];
      float xh[8], g[8];
      gn_bwd_g8<F16, SILU>(vx, vdy, kc, xh, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s1 += g[j];
        s2 += g[j] * xh[j];
      }
    }
    for (int o = 4; o; o >>= 1) {
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (c0 + ch < C && (v & 7) == 0) {
      float* part = a.workspace + (((int64_t)n * C + c0 + ch) * gridDim.x + blockIdx.x) * 2;
      part[0] = s1;
      part[1] = s2;
    }
  }
}

// one wave per (n, group): the slab's cpg x parts partials are contiguous, channel-major; lane l
// takes items l, l + 64, ..., then the xor tree.  {m1, m2} go behind the partials.
template <bool F16>
__global__ __launch_bounds__(64) void gn_bwd_fold_kernel(p2p_group_norm_bwd_args a, int parts) {
  const int G = a.groups, C = a.channels, cpg = C / G;
  const int n = blockIdx.x / G, g = blockIdx.x - n * G;
  const float* part = a.workspace + ((int64_t)n * C + g * cpg) * parts * 2;
  const uint16_t* gamma = static_cast<const uint16_t*>(a.gamma) + g * cpg;
  const int items = cpg * parts;
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < items; i += 64) {
    const float gm = ld16<F16>(gamma[i / parts]);
    s1 += gm * part[2 * i];
    s2 += gm * part[2 * i + 1];
  }
  for (int o = 32; o; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (threadIdx.x == 0) {
    const float inv_l = 1.f / ((float)cpg * (float)a.hw);
    float* m = a.workspace + (int64_t)a.n * C * parts * 2 + 2 * (int64_t)blockIdx.x;
    m[0] = s1 * inv_l;
    m[1] = s2 * inv_l;
  }
}

template <bool F16, bool SILU>
__global__ __launch_bounds__(256) void gn_bwd_apply_nchw_kernel(p2p_group_norm_bwd_args a, int64_t n_vec,
                                                                const float* means) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int hwv = a.hw >> 3;
  const int64_t row = iv / hwv;
  const int n = (int)(row / a.channels), c = (int)(row - (int64_t)n * a.channels);
  const ChanCoef k = chan_coef<F16>(a, n, c);
  const float* m = means + 2 * (n * a.groups + c / (a.channels / a.groups));
  static_cast<u16x8_t*>(a.dx)[iv] = gn_bwd_dx8<F16, SILU>(static_cast<const u16x8_t*>(a.x)[iv],
                                                           static_cast<const u16x8_t*>(a.dy)[iv], k, m[0], m[1]);
}

template <bool F16, bool SILU>
__global__ __launch_bounds__(256) void gn_bwd_apply_tok_kernel(p2p_group_norm_bwd_args a, const float* means) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTile * kTileLd];   // [pixel][channel]
  const int p0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile, n = blockIdx.z;
  const int C = a.channels, hw = a.hw;
  const uint16_t* dy = static_cast<const uint16_t*>(a.dy) + (int64_t)n * hw * C;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int p = v >> 3, ch = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw)
      *reinterpret_cast<u16x8_t*>(&tile[p * kTileLd + ch]) =
          *reinterpret_cast<const u16x8_t*>(dy + (int64_t)(p0 + p) * C + c0 + ch);
  }
  __syncthreads();
  const int64_t base = (int64_t)n * C * hw;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int ch = v >> 3, p = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw) {
      const int c = c0 + ch;
      const ChanCoef kc = chan_coef<F16>(a, n, c);
      const float* m = means + 2 * (n * a.groups + c / (C / a.groups));
      const int64_t off = base + (int64_t)c * hw + p0 + p;
      const u16x8_t vx = *reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.x) + off);
      u16x8_t vdy;
#pragma unroll
      for (int j = 0; j < 8; ++j) vdy[j] = tile[(p + j) * kTileLd + ch];
      *reinterpret_cast<u16x8_t*>(static_cast<uint16_t*>(a.dx) + off) = gn_bwd_dx8<F16, SILU>(vx, vdy, kc, m[0], m[1]);
    }
  }
}

// din[m, j] = dout[m, j] * gelu(gate), din[m, d + j] = dout[m, j] * h * (Phi(gate) + gate * phi(gate))
template <bool F16>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(p2p_geglu_bwd_args a, int64_t n_vec) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int dv = a.d >> 3;
  const int64_t m = iv / dv;
  const int j = (int)(iv - m * dv) * 8;
  const uint16_t* row = static_cast<const uint16_t*>(a.in) + m * a.in_row_stride;
  const u16x8_t h = *reinterpret_cast<const u16x8_t*>(row + j);
  const u16x8_t g = *reinterpret_cast<const u16x8_t*>(row + a.d + j);
  const u16x8_t dy = *reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.dout) + m * a.d + j);
  u16x8_t oh, og;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float gate = ld16<F16>(g[i]), d = ld16<F16>(dy[i]);
    const float cdf = 0.5f * (1.f + erff(gate * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * __expf(-0.5f * gate * gate);
    oh[i] = st16<F16>(d * (gate * cdf));
    og[i] = st16<F16>(d * ld16<F16>(h[i]) * (cdf + gate * pdf));
  }
  uint16_t* out = static_cast<uint16_t*>(a.din) + m * 2 * a.d;
  *reinterpret_cast<u16x8_t*>(out + j) = oh;
  *reinterpret_cast<u16x8_t*>(out + a.d + j) = og;
}

// dst[n, hw, C] = src[n, C, hw]: gn_apply_tok_kernel's transpose without the arithmetic
__global__ __launch_bounds__(256) void nchw_to_tokens_kernel(p2p_nchw_to_tokens_args a) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTile * kTileLd];   // [pixel][channel]
  const int p0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile, n = blockIdx.z;
  const int C = a.channels, hw = a.hw;
  const uint16_t* src = static_cast<const uint16_t*>(a.src) + (int64_t)n * C * hw;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int ch = v >> 3, p = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw) {
      const u16x8_t in = *reinterpret_cast<const u16x8_t*>(src + (int64_t)(c0 + ch) * hw + p0 + p);
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[(p + j) * kTileLd + ch] = in[j];
    }
  }
  __syncthreads();
  uint16_t* dst = static_cast<uint16_t*>(a.dst) + (int64_t)n * hw * C;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;
    const int p = v >> 3, ch = (v & 7) * 8;
    if (c0 + ch < C && p0 + p < hw)
      *reinterpret_cast<u16x8_t*>(dst + (int64_t)(p0 + p) * C + c0 + ch) =
          *reinterpret_cast<const u16x8_t*>(&tile[p * kTileLd + ch]);
  }
}

// ---- the time path: out[n, c] = W[c, :] . act(in[n, :]) + b[c] for N <= 64 rows, a skinny GEMM
// whose traffic is W.  One wave per kTimeChannelsPerWave rows of W, held in registers (16-bit, as
// loaded: every load of the workgroup is issued before anything else); the activated input rows,
// f32, in LDS, kTimeRows at a time, so W is read once whatever N is.  A dot product is the lane's
// own vectors in order, then the xor tree over the wave: a fixed order.  Three inputs:
//   kTimeSinusoid  in[n, :] = [cos(t_n f_i), sin(t_n f_i)], f_i = exp(-ln(10000) i / half), from the
//                  int64 timesteps (accurate cosf / sinf / expf: the arguments reach 999 rad)
//   kTimeF32Silu   silu of an f32 row (linear_1's unrounded output)
//   kTimeIoSilu    silu of a 16-bit row (emb)
// and the output in f32 (linear_1) or rounded once to the tensor type.
enum { kTimeSinusoid = 0, kTimeF32Silu = 1, kTimeIoSilu = 2 };
constexpr int kTimeVecs = 4;                                  // rows of W of up to 64 * 4 * 8 = 2048 elements
constexpr int kTimeMaxD = 64 * kTimeVecs * 8;
constexpr int kTimeChannelsPerWave = 4;
constexpr int kTimeWaves = 4;
constexpr int kTimeTile = kTimeChannelsPerWave * kTimeWaves;  // output channels per workgroup
constexpr int kTimeRows = 8;                                  // input rows in LDS at a time
static_assert(kTimeTile == P2P_TIME_PROJ_TILE, "p2p_time_proj_args.tiles counts tiles of this many channels");

struct TimeLinearArgs {
  const void* in;            // f32 or 16-bit [n, d]; unused for kTimeSinusoid
  const int64_t* timesteps;  // kTimeSinusoid: n timesteps, timestep_stride apart (0: one for all rows)
  int64_t timestep_stride;
  const void* w;             // one segment: [channels, d], bias [channels], out [n, channels] ...
  const void* b;
  void* out;
  int channels;
  const int64_t* table;      // ... or `segments` rows of {W, b, s_r, C_r}: out_r starts n * s_r elements into `out`
  int segments;
  int n, d;
};

template <bool F16, int IN>
__global__ __launch_bounds__(64 * kTimeWaves) void time_linear_kernel(TimeLinearArgs a) {
  extern __shared__ __attribute__((aligned(16))) float act[];   // [kTimeRows][d]
  constexpr bool OUT_F32 = IN == kTimeSinusoid;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // this workgroup's segment and its first channel there (workgroup-uniform)
  const uint16_t* w = static_cast<const uint16_t*>(a.w);
  const uint16_t* b = static_cast<const uint16_t*>(a.b);
  int64_t out_off = 0;
  int C = a.channels;
  int c0 = blockIdx.x * kTimeTile;
  if (a.table) {
    int tile = blockIdx.x, r = 0;
    for (; r < a.segments; ++r) {
      const int tiles = ((int)a.table[4 * r + 3] + kTimeTile - 1) / kTimeTile;
      if (tile < tiles) break;
      tile -= tiles;
    }
    if (r == a.segments) return;   // a grid larger than the table's tiles
    w = reinterpret_cast<const uint16_t*>(a.table[4 * r]);
    b = reinterpret_cast<const uint16_t*>(a.table[4 * r + 1]);
    out_off = a.table[4 * r + 2] * a.n;
    C = (int)a.table[4 * r + 3];
    c0 = tile * kTimeTile;
  }
  const int D = a.d, nv = D >> 3;
  const int cw = c0 + wave * kTimeChannelsPerWave;   // this wave's first channel
  u16x8_t wv[kTimeChannelsPerWave][kTimeVecs];
#pragma unroll
  for (int k = 0; k < kTimeChannelsPerWave; ++k)
#pragma unroll
    for (int i = 0; i < kTimeVecs; ++i) {
      const int iv = lane + 64 * i;
      wv[k][i] = u16x8_t{};
      if (cw + k < C && iv < nv) wv[k][i] = *reinterpret_cast<const u16x8_t*>(w + (int64_t)(cw + k) * D + 8 * iv);
    }
  float bias[kTimeChannelsPerWave];
#pragma unroll
  for (int k = 0; k < kTimeChannelsPerWave; ++k) bias[k] = cw + k < C ? ld16<F16>(b[cw + k]) : 0.f;

  for (int n0 = 0; n0 < a.n; n0 += kTimeRows) {
    const int rows = min(kTimeRows, a.n - n0);
    __syncthreads();   // the previous rows have been read
    for (int e = threadIdx.x; e < rows * D; e += 64 * kTimeWaves) {
      // (row, column) of element e; rows <= 8, so the row is found by counting, not by a division
      int n = 0;
      while ((n + 1) * D <= e) ++n;
      const int j = e - n * D;
      float v;
      if (IN == kTimeSinusoid) {
        const int half = D >> 1;
        const int i = j < half ? j : j - half;
        const float f = expf(-9.210340371976184f * (float)i / (float)half);
        const float arg = (float)a.timesteps[(n0 + n) * a.timestep_stride] * f;
        v = j < half ? cosf(arg) : sinf(arg);
      } else if (IN == kTimeF32Silu) {
        const float h = static_cast<const float*>(a.in)[(int64_t)(n0 + n) * D + j];
        v = h / (1.f + expf(-h));
      } else {
        const float h = ld16<F16>(static_cast<const uint16_t*>(a.in)[(int64_t)(n0 + n) * D + j]);
        v = h / (1.f + expf(-h));
      }
      act[n * D + j] = v;
    }
    __syncthreads();
    for (int n = 0; n < rows; ++n) {
      float acc[kTimeChannelsPerWave] = {};
#pragma unroll
      for (int i = 0; i < kTimeVecs; ++i) {
        const int iv = lane + 64 * i;
        if (iv < nv) {
          const float4 lo = *reinterpret_cast<const float4*>(act + n * D + 8 * iv);
          const float4 hi = *reinterpret_cast<const float4*>(act + n * D + 8 * iv + 4);
          const float av[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
          for (int k = 0; k < kTimeChannelsPerWave; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[k] += ld16<F16>(wv[k][i][j]) * av[j];
        }
      }
#pragma unroll
      for (int k = 0; k < kTimeChannelsPerWave; ++k) {
        for (int o = 32; o; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
        // lane k stores channel cw + k of row n0 + n
        if (lane == k && cw + k < C) {
          const float y = acc[k] + bias[k];
          const int64_t at = out_off + (int64_t)(n0 + n) * C + cw + k;
          if (OUT_F32) static_cast<float*>(a.out)[at] = y;
          else static_cast<uint16_t*>(a.out)[at] = st16<F16>(y);
        }
      }
    }
  }
}

template <bool F16, int IN>
void launch_time_linear(const TimeLinearArgs& a, int tiles, hipStream_t st) {
  const uint32_t lds = (uint32_t)(min(a.n, kTimeRows) * a.d * sizeof(float));   // <= 64 KB
  launch_kernel((time_linear_kernel<F16, IN>), dim3((unsigned)tiles), dim3(64 * kTimeWaves), lds, st, a);
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

static_assert(kTile == kGnBwdTile, "gn_bwd_workspace_floats counts the token-major partials by this tile");

template <bool F16, bool SILU>
void launch_group_norm_bwd(const p2p_group_norm_bwd_args& a, hipStream_t st) {
  const int64_t rows = (int64_t)a.n * a.channels;
  const dim3 tiles((a.hw + kTile - 1) / kTile, (a.channels + kTile - 1) / kTile, a.n);
  const bool tok = a.dy_layout == P2P_LAYOUT_TOKENS;
  const int parts = tok ? (int)tiles.x : 1;
  if (tok) {
    launch_kernel((gn_bwd_reduce_tok_kernel<F16, SILU>), tiles, dim3(256), 0, st, a);
  } else if (a.hw >= kGnBwdWideRow) {
    launch_kernel((gn_bwd_reduce_nchw_kernel<F16, SILU, 256>), dim3((unsigned)rows), dim3(256), 0, st, a);
  } else {
    launch_kernel((gn_bwd_reduce_nchw_kernel<F16, SILU, 64>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
  }
  launch_kernel(gn_bwd_fold_kernel<F16>, dim3((unsigned)(a.n * a.groups)), dim3(64), 0, st, a, parts);
  const float* means = a.workspace + rows * parts * 2;
  if (tok) {
    launch_kernel((gn_bwd_apply_tok_kernel<F16, SILU>), tiles, dim3(256), 0, st, a, means);
  } else {
    const int64_t n_vec = rows * a.hw / 8;
    launch_kernel((gn_bwd_apply_nchw_kernel<F16, SILU>), dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, st, a,
                  n_vec, means);
  }
}

}  // namespace

int run_group_norm_bwd(const p2p_group_norm_bwd_args& a, hipStream_t st) {
  if (!a.x || !a.gamma || !a.beta || !a.dy || !a.stats || !a.dx || !a.workspace) return P2P_E_ARG;
  if (a.n < 1 || a.channels < 1 || a.hw < 1 || a.groups < 1 || a.channels % a.groups) return P2P_E_ARG;
  if (a.n > 65535 || a.channels > 65535 * kTile || (int64_t)a.n * a.channels > INT32_MAX / 2) return P2P_E_ARG;
  // the split statistics' slabs are not served (nor is anything the 32-bit grids could not index)
  if ((int64_t)(a.channels / a.groups) * a.hw >= kGnStatsSplit) return P2P_E_ARG;
  if ((int64_t)a.n * a.channels * a.hw / 8 / 256 >= INT32_MAX) return P2P_E_ARG;
  if (a.chan_add && a.chan_add_stride != 0 && a.chan_add_stride != a.channels) return P2P_E_ARG;
  if (a.act != P2P_ACT_NONE && a.act != P2P_ACT_SILU) return P2P_E_ARG;
  if (a.dy_layout != P2P_LAYOUT_NCHW && a.dy_layout != P2P_LAYOUT_TOKENS) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.hw % 8 || (a.dy_layout == P2P_LAYOUT_TOKENS && a.channels % 8)) return P2P_E_ALIGN;
  if (!aligned16(a.x) || !aligned16(a.dy) || !aligned16(a.dx)) return P2P_E_ALIGN;
  if (((uintptr_t)a.stats & 3) || ((uintptr_t)a.workspace & 3)) return P2P_E_ALIGN;
  const bool f16 = a.dtype == P2P_DTYPE_F16, act = a.act == P2P_ACT_SILU;
  if (f16 && act) launch_group_norm_bwd<true, true>(a, st);
  else if (f16) launch_group_norm_bwd<true, false>(a, st);
  else if (act) launch_group_norm_bwd<false, true>(a, st);
  else launch_group_norm_bwd<false, false>(a, st);
  return (int)hipGetLastError();
}

int run_geglu_bwd(const p2p_geglu_bwd_args& a, hipStream_t st) {
  if (!a.in || !a.dout || !a.din) return P2P_E_ARG;
  if (a.rows < 1 || a.d < 1 || a.in_row_stride < 2 * (int64_t)a.d) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.d % 8 || a.in_row_stride % 8) return P2P_E_ALIGN;
  if (!aligned16(a.in) || !aligned16(a.dout) || !aligned16(a.din)) return P2P_E_ALIGN;
  const int64_t n_vec = (int64_t)a.rows * (a.d / 8);
  if ((n_vec + 255) / 256 > INT32_MAX) return P2P_E_ARG;
  const dim3 grid((unsigned)((n_vec + 255) / 256));
  if (a.dtype == P2P_DTYPE_F16) launch_kernel(geglu_bwd_kernel<true>, grid, dim3(256), 0, st, a, n_vec);
  else launch_kernel(geglu_bwd_kernel<false>, grid, dim3(256), 0, st, a, n_vec);
  return (int)hipGetLastError();
}

int run_nchw_to_tokens(const p2p_nchw_to_tokens_args& a, hipStream_t st) {
  if (!a.src || !a.dst) return P2P_E_ARG;
  if (a.n < 1 || a.channels < 1 || a.hw < 1 || a.n > 65535) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.hw % 8 || a.channels % 8) return P2P_E_ALIGN;
  if (!aligned16(a.src) || !aligned16(a.dst)) return P2P_E_ALIGN;
  const dim3 grid((a.hw + kTile - 1) / kTile, (a.channels + kTile - 1) / kTile, a.n);
  if (grid.y > 65535) return P2P_E_ARG;
  launch_kernel(nchw_to_tokens_kernel, grid, dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

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

int run_time_embed(const p2p_time_embed_args& a, hipStream_t st) {
  if (!a.timesteps || !a.w1 || !a.b1 || !a.w2 || !a.b2 || !a.workspace || !a.emb) return P2P_E_ARG;
  if (a.n < 1 || a.n > P2P_MAX_BATCH || a.in_channels < 1 || a.d < 1) return P2P_E_ARG;
  if (a.in_channels > kTimeMaxD || a.d > kTimeMaxD) return P2P_E_ARG;
  if (a.timestep_stride != 0 && a.timestep_stride != 1) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.in_channels % 8 || a.d % 8) return P2P_E_ALIGN;
  if (!aligned16(a.w1) || !aligned16(a.w2) || !aligned16(a.workspace) || !aligned16(a.emb)) return P2P_E_ALIGN;
  if (((uintptr_t)a.timesteps & 7) || ((uintptr_t)a.b1 & 1) || ((uintptr_t)a.b2 & 1)) return P2P_E_ALIGN;
  const int tiles = (a.d + kTimeTile - 1) / kTimeTile;
  const bool f16 = a.dtype == P2P_DTYPE_F16;
  TimeLinearArgs l1 = {};
  l1.timesteps = a.timesteps; l1.timestep_stride = a.timestep_stride;
  l1.w = a.w1; l1.b = a.b1; l1.out = a.workspace; l1.channels = a.d;
  l1.n = a.n; l1.d = a.in_channels;
  if (f16) launch_time_linear<true, kTimeSinusoid>(l1, tiles, st);
  else launch_time_linear<false, kTimeSinusoid>(l1, tiles, st);
  TimeLinearArgs l2 = {};
  l2.in = a.workspace;
  l2.w = a.w2; l2.b = a.b2; l2.out = a.emb; l2.channels = a.d;
  l2.n = a.n; l2.d = a.d;
  if (f16) launch_time_linear<true, kTimeF32Silu>(l2, tiles, st);
  else launch_time_linear<false, kTimeF32Silu>(l2, tiles, st);
  return (int)hipGetLastError();
}

int run_time_proj(const p2p_time_proj_args& a, hipStream_t st) {
  if (!a.emb || !a.table || !a.out) return P2P_E_ARG;
  if (a.n < 1 || a.n > P2P_MAX_BATCH || a.d < 1 || a.d > kTimeMaxD || a.segments < 1 || a.tiles < 1) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.d % 8) return P2P_E_ALIGN;
  if (!aligned16(a.emb) || ((uintptr_t)a.table & 7) || ((uintptr_t)a.out & 1)) return P2P_E_ALIGN;
  TimeLinearArgs l = {};
  l.in = a.emb; l.out = a.out;
  l.table = a.table; l.segments = a.segments;
  l.n = a.n; l.d = a.d;
  if (a.dtype == P2P_DTYPE_F16) launch_time_linear<true, kTimeIoSilu>(l, a.tiles, st);
  else launch_time_linear<false, kTimeIoSilu>(l, a.tiles, st);
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
