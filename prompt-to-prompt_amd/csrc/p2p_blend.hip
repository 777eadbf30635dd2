// LocalBlend and AttentionStore helpers (bandwidth-bound, no MFMA).
//
// LocalBlend (null_text.py:41-70; main.py:35-52 is the two-prompt case):
//   maps   = cat_l reshape(store_l, [B, H, 1, 16, 16, W])           -> [B, L*H, 1, 16, 16, W]
//   m      = (maps * alpha).sum(-1).mean(1)                           -> [B, 1, 16, 16]
//   m      = max_pool2d(m, 3, 1, 1)          (pooled mask only)
//   m      = interpolate(m, x_t.shape[2:])   (nearest)
//   mask   = (m / max_{y,x} m) > th;  mask = mask[:1] | mask
//   mask  &= ~(substruct mask)               (optional, unpooled, th[1])
//   x_t    = x_t[:1] + mask * (x_t - x_t[:1])
// Kernel 1 reduces the word axis for every (prompt, layer x head) map; kernel 2 does the rest,
// one workgroup per prompt (each rebuilds prompt 0's mask, which gates every other prompt).
// The latent step that builds the same mask in its own launch is p2p_latent.hip's.
#include "p2p_blend_mask.h"
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

constexpr int kBlendMaxPrompts = 16;

// grid (n_prompts, n_maps * heads, pixel chunks of kWsPix), 256 threads.  A chunk's rows
// [kWsPix, W] are one contiguous span of the store: the workgroup copies it to LDS with
// coalesced 16-byte loads, then every thread sums one pixel's words in index order.
constexpr int kWsPix = 64;

__global__ __launch_bounds__(256) void blend_wordsum_kernel(p2p_blend_args a) {
  const int b = blockIdx.x;
  const int j = blockIdx.y;                 // l * heads + hd
  const int l = j / a.heads_per_map;
  const int hd = j - l * a.heads_per_map;
  const int R2 = a.map_res * a.map_res;
  const int W = a.n_words;
  const int p0 = blockIdx.z * kWsPix;
  const int npix = min(kWsPix, R2 - p0);
  __shared__ float sa[128], ss[128];
  __shared__ __attribute__((aligned(16))) float rows[kWsPix * 128];
  for (int w = threadIdx.x; w < W; w += blockDim.x) {
    sa[w] = a.alpha_layers[b * W + w];
    ss[w] = a.substruct_layers ? a.substruct_layers[b * W + w] : 0.f;
  }
  const float* m = a.maps[l] + ((int64_t)(b * a.heads_per_map + hd) * R2 + p0) * W;
  const int n = npix * W;
  if ((((uintptr_t)m) & 15) == 0) {
    for (int i = threadIdx.x; i < n / 4; i += blockDim.x)
      reinterpret_cast<f32x4_t*>(rows)[i] = reinterpret_cast<const f32x4_t*>(m)[i];
    for (int i = (n & ~3) + threadIdx.x; i < n; i += blockDim.x) rows[i] = m[i];
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) rows[i] = m[i];
  }
  __syncthreads();
  const int pix = threadIdx.x;
  if (pix >= npix) return;
  const float* r = rows + pix * W;          // W odd (77): the 64 rows hit distinct banks
  float acc_a = 0.f, acc_s = 0.f;
  for (int w = 0; w < W; ++w) {
    const float v = r[w];
    acc_a += v * sa[w];
    acc_s += v * ss[w];
  }
  const int LH = a.n_maps * a.heads_per_map;
  a.word_sums[((int64_t)(b * 2 + 0) * LH + j) * R2 + p0 + pix] = acc_a;
  a.word_sums[((int64_t)(b * 2 + 1) * LH + j) * R2 + p0 + pix] = acc_s;
}

// x0 + m * (xb - x0) rounded exactly as the reference's three tensor ops (no fma contraction)
__device__ __forceinline__ float blend1(float x0, float xb, float m) {
#pragma clang fp contract(off)
  const float diff = xb - x0;
  const float t = m * diff;
  return x0 + t;
}

// one workgroup per prompt b: it rebuilds the source prompt's pooled mask next to its own (the
// source mask gates every prompt, mask = mask[:1] | mask), so the prompts run in parallel and no
// workgroup reads another's output (x_t[0] is never written: x_t[0] + mask * 0 == x_t[0])
__global__ __launch_bounds__(256, 1) void blend_finalize_kernel(p2p_blend_args a) {
  const int b = blockIdx.x;
  const int R = a.map_res;
  const int R2 = R * R;
  const int LH = a.n_maps * a.heads_per_map;
  const int HW = a.lat_h * a.lat_w;
  __shared__ BlendLds L;
  build_blend_mask(a.word_sums, a.word_sums + (int64_t)b * 2 * LH * R2, LH, R, a.lat_h, a.lat_w, a.th_pool,
                   a.th_sub, a.substruct_layers != nullptr, L);
  // x_t[b] = x_t[0] + mask * (x_t[b] - x_t[0])
  for (int yx = threadIdx.x; yx < HW; yx += blockDim.x) {
    const float mf = L.msrc[blend_src_of(yx, R, a.lat_h, a.lat_w)];
    if (a.mask_out) a.mask_out[(int64_t)b * HW + yx] = mf != 0.f ? 1 : 0;
    if (b == 0 || !a.x_t) continue;  // x_t[0] + mask * 0 == x_t[0]; mask-only mode
    for (int ch = 0; ch < a.channels; ++ch) {
      const float x0 = a.x_t[(int64_t)(0 * a.channels + ch) * HW + yx];
      float* xb = a.x_t + (int64_t)(b * a.channels + ch) * HW + yx;
      *xb = blend1(x0, *xb, mf);
    }
  }
}

// dst = src * (1 / divisor): what `tensor / scalar` computes on the reference's cuda:0 device
// (the f32 reciprocal, then one multiply per element).
__global__ void store_scale_kernel(const float* __restrict__ src, float* __restrict__ dst, float inv, int64_t n) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    reinterpret_cast<f32x4_t*>(dst)[i] = reinterpret_cast<const f32x4_t*>(src)[i] * inv;
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dst[i] = src[i] * inv;
}

// ---------------------------------------------------------------- shader-clock probe
// Measurement only (bench.py's roofline clock): one wave per workgroup.  Each wave reads the
// shader-cycle counter (s_memtime: one tick per shader clock) and the constant 100 MHz counter
// (s_memrealtime), spins on the 100 MHz counter until `ticks` of it have passed, and reads both
// again -- clock = d(cycles) / d(ticks) x 100 MHz.  Both pairs are read in the same order, so the
// two windows are offset by the same read latency.  Consecutive workgroups land on different XCDs
// (round-robin dispatch), so n workgroups >= 8 sample every XCD.  Lanes 0 / 1 store (vector
// stores): out[2 wg] = cycles, out[2 wg + 1] = ticks.
__global__ void clock_probe_kernel(unsigned long long* __restrict__ out, unsigned ticks) {
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long r1 = r0;
  while (r1 - r0 < ticks) {
    __builtin_amdgcn_s_sleep(2);
    r1 = __builtin_amdgcn_s_memrealtime();
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  r1 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x < 2) out[2 * blockIdx.x + threadIdx.x] = threadIdx.x == 0 ? c1 - c0 : r1 - r0;
}

int run_localblend(const p2p_blend_args& a, hipStream_t st) {
  if (a.n_prompts < 1 || a.n_prompts > kBlendMaxPrompts || a.map_res * a.map_res > 256 || a.n_words > 128 ||
      a.n_maps < 1 || a.n_maps > 8 || !a.alpha_layers || (!a.x_t && !a.mask_out) || !a.word_sums ||
      a.lat_h < 1 || a.lat_w < 1)
    return P2P_E_ARG;
  for (int l = 0; l < a.n_maps; ++l)
    if (!a.maps[l] && !a.word_sums_ready) return P2P_E_ARG;
  dim3 g1(a.n_prompts, a.n_maps * a.heads_per_map, (a.map_res * a.map_res + kWsPix - 1) / kWsPix);
  if (!a.word_sums_ready) launch_kernel(blend_wordsum_kernel, g1, dim3(256), 0, st, a);
  launch_kernel(blend_finalize_kernel, dim3(a.n_prompts), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int run_clock_probe(unsigned long long* out, int n_wg, int ticks, hipStream_t st) {
  launch_kernel(clock_probe_kernel, dim3((unsigned)n_wg), dim3(64), 0, st, out, (unsigned)ticks);
  return (int)hipGetLastError();
}

int run_store_scale(const float* src, float* dst, float divisor, int64_t n, hipStream_t st) {
  if (n <= 0) return 0;
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return P2P_E_ALIGN;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  const float inv = 1.0f / divisor;
  launch_kernel(store_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, dst, inv, n);
  return (int)hipGetLastError();
}

}  // namespace p2p
