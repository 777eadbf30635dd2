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
#include <type_traits>

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
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// LDS of one mask build (256 threads): mean maps, pooled maps, per-wave maxima, the mask per map
// pixel.  [0] = the group's source prompt, [1] = prompt b
struct BlendLds {
  float mean_a[2][256];
  float mean_s[2][256];
  float pooled[2][256];
  float red[4][4];
  float msrc[256];
};

// nearest upsampling (F.interpolate default): latent pixel yx -> map pixel
__device__ __forceinline__ int blend_src_of(int yx, int R, int lat_h, int lat_w) {
  const float sy = (float)R / (float)lat_h, sx = (float)R / (float)lat_w;
  const int Y = yx / lat_w, X = yx - Y * lat_w;
  return min((int)floorf(Y * sy), R - 1) * R + min((int)floorf(X * sx), R - 1);
}

// Prompt b's LocalBlend mask per map pixel (L.msrc, 1.f / 0.f) from the word sums of its group's
// source prompt (ws0) and its own (wsb), each [2, LH, R*R] (index 0: alpha-weighted, 1:
// substruct-weighted): mean over the LH maps, 3x3 max-pool, per-image max of the upsampled map,
// thresholds, mask[:1] | mask, substruct gate (null_text.py:41-67).  Called by all 256 threads of
// the workgroup (it synchronises); blend_finalize_kernel and latent_blend_kernel share it, so
// both build the same mask bit for bit.
__device__ __forceinline__ void build_blend_mask(const float* ws0, const float* wsb, int LH, int R, int lat_h, int lat_w,
                                 float th_pool, float th_sub, bool sub, BlendLds& L) {
  const int R2 = R * R;
  const int tid = threadIdx.x;
  // mean over the L*H maps (sum in index order, then / L*H as Tensor.mean does).  The four
  // (prompt, sum) planes -- source / b x alpha / substruct -- go to the four waves; a lane sums
  // four adjacent map pixels, so every load is one 16-byte row piece and a wave's LH loads of a
  // plane are all in flight at once (one memory round trip for the whole mask)
  {
    // (source | b) x (alpha | substruct); the wave index in a scalar register, so the plane's buffer
    // resource is scalar too (from a VGPR each of the 48 loads became a readfirstlane waterfall loop)
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6), k = g & 1, sidx = g >> 1;
    const int px0 = (tid & 63) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (px0 < R2 && (sidx == 0 || sub)) {
      const float* base = (k ? wsb : ws0) + (int64_t)sidx * LH * R2;
      if ((R2 & 3) == 0) {
        // buffer loads: maps past LH read as 0 (range-checked), so the 48 loads of a batch are
        // issued unconditionally, all before the first add; adding those +0.0 to a sum of
        // non-negative terms leaves it bit for bit (the in-order sum over j < LH)
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (int64_t)LH * R2 * 4);
        for (int j0 = 0; j0 < LH; j0 += 48) {
          f32x4_t v[48];
#pragma unroll
          for (int u = 0; u < 48; ++u)
            v[u] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, ((j0 + u) * R2 + px0) * 4, 0, 0));
#pragma unroll
          for (int u = 0; u < 48; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += v[u][q];
        }
      } else {
        for (int j = 0; j < LH; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (px0 + q < R2) acc[q] += base[(int64_t)j * R2 + px0 + q];
      }
    }
    float* const dst = sidx == 0 ? L.mean_a[k] : L.mean_s[k];
    float pmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (px0 + q < R2) {
        const float mv = acc[q] / (float)LH;
        dst[px0 + q] = mv;
        pmax = fmaxf(pmax, mv);
      }
    // the wave holds its whole plane: its maximum needs no cross-wave reduction
    pmax = wave_max(pmax);
    if ((tid & 63) == 0) L.red[0][g] = pmax;
  }
  __syncthreads();
  if (lat_h >= R && lat_w >= R) {
    // Upsampling samples every map pixel, and a 3x3 max-pool keeps the plane's maximum (every
    // pixel lies in its own window), so the per-image maxima of the pooled / unpooled upsampled
    // maps are the four plane maxima above -- the same floats the generic path below reduces to.
    // Pool on the fly and threshold: one more barrier in all (mask per map pixel, gathered by the
    // nearest upsampling: identical per output pixel, evaluated R*R times instead of H*W)
    const float v0 = L.red[0][0], vb = L.red[0][1], s0m = L.red[0][2], sbm = L.red[0][3];
    for (int pix = tid; pix < R2; pix += 256) {
      const int y = pix / R, x = pix - y * R;
      float p0 = -INFINITY, pb = -INFINITY;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if (yy >= 0 && yy < R && xx >= 0 && xx < R) {
            p0 = fmaxf(p0, L.mean_a[0][yy * R + xx]);
            pb = fmaxf(pb, L.mean_a[1][yy * R + xx]);
          }
        }
      bool mask = p0 / v0 > th_pool || pb / vb > th_pool;
      if (sub) mask = mask && !(L.mean_s[0][pix] / s0m > th_sub || L.mean_s[1][pix] / sbm > th_sub);
      L.msrc[pix] = mask ? 1.f : 0.f;
    }
    __syncthreads();
    return;
  }
  // generic path (latent smaller than the maps: the nearest down-sampling skips map pixels)
  // 3x3 max-pool, stride 1, padding 1 (padding never wins: -inf)
  for (int i = tid; i < 2 * R2; i += 256) {
    const int k = i / R2, pix = i - k * R2;
    const int y = pix / R, x = pix - y * R;
    float m = -INFINITY;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < R && xx >= 0 && xx < R) m = fmaxf(m, L.mean_a[k][yy * R + xx]);
      }
    L.pooled[k][pix] = m;
  }
  __syncthreads();
  // per-image max of the nearest-upsampled maps.  Upsampling (latent >= map resolution) samples
  // every source pixel, so the max over the grid is the max over the R*R sources.
  const bool all_sources = lat_h >= R && lat_w >= R;
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int i = tid; i < (all_sources ? R2 : lat_h * lat_w); i += 256) {
    const int src = all_sources ? i : blend_src_of(i, R, lat_h, lat_w);
    m[0] = fmaxf(m[0], L.pooled[0][src]);
    m[1] = fmaxf(m[1], L.mean_s[0][src]);
    m[2] = fmaxf(m[2], L.pooled[1][src]);
    m[3] = fmaxf(m[3], L.mean_s[1][src]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) m[c] = wave_max(m[c]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) L.red[tid >> 6][c] = m[c];
  __syncthreads();
  float vmax[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    vmax[c] = L.red[0][c];
    for (int w = 1; w < 4; ++w) vmax[c] = fmaxf(vmax[c], L.red[w][c]);
  }
  // mask of prompt b per source pixel (the thresholds of null_text.py:62-67), then gathered by
  // the nearest upsampling: identical per output pixel, evaluated R*R times instead of H*W
  for (int pix = tid; pix < R2; pix += 256) {
    const bool m0 = L.pooled[0][pix] / vmax[0] > th_pool;
    const bool mb = L.pooled[1][pix] / vmax[2] > th_pool;
    bool mask = m0 || mb;
    if (sub) {
      const bool s0 = L.mean_s[0][pix] / vmax[1] > th_sub;
      const bool sb = L.mean_s[1][pix] / vmax[3] > th_sub;
      mask = mask && !(s0 || sb);
    }
    L.msrc[pix] = mask ? 1.f : 0.f;
  }
  __syncthreads();
}

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

// ---------------------------------------------------------------- fused latent update
// One denoising step's latent update (ptp_utils.py:72-75): classifier-free guidance
// (:73), the DDIM step (diffusers DDIMScheduler.step with eta = 0, restated by the reference as
// NullInversion.prev_step, null_text.py:471-479; the same formula with the inversion's
// coefficients is next_step, :481-489) and the LocalBlend latent blend with a precomputed mask
// (null_text.py:68-70 / main.py:50-52).  Every intermediate is rounded where the reference's
// torch ops round it: to bf16 (f16) for the products torch keeps in the U-Net's bf16 (f16) output dtype,
// to f32 elsewhere, with no fma contraction -- so the update is bit-identical to the eager
// sequence on the same inputs.
__device__ __forceinline__ float rnd_bf16(float x) { return bf2f(f2bf(x)); }
__device__ __forceinline__ float rnd_f16(float x) { return h2f(f2h(x)); }

// explicit round-to-nearest ops: no fma contraction whatever the compile flags
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }

// prev_sample from one element's inputs (CFG combine + DDIM step): eu / ec the unconditional and
// conditional eps (ec unused without CFG), x the latent
// the step's scalar coefficients, copied out of the kernel-argument struct by value (a kernel that
// also indexes the struct's blend_sums[] array at run time would otherwise read every field through
// a vector load of the kernarg segment, one dependent round trip each)
struct DdimC {
  int cfg;
  float guidance, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_one_minus_alpha_prev;
  template <typename A>   // p2p_latent_step_args, p2p_direct_step_args or p2p_ddpm_step_args (the same fields)
  __device__ explicit DdimC(const A& a)
      : cfg(a.cfg), guidance(a.guidance), sqrt_beta_t(a.sqrt_beta_t), sqrt_alpha_t(a.sqrt_alpha_t),
        sqrt_alpha_prev(a.sqrt_alpha_prev), sqrt_one_minus_alpha_prev(a.sqrt_one_minus_alpha_prev) {}
  // the step-form interface of latent_blend_kernel: DDIM reads no tensor beside eps and x
  struct Extra {};
  __device__ __forceinline__ void load(Extra&, int64_t) const {}
  __device__ __forceinline__ void store(int64_t, const f32x4_t&) const {}
  template <int DT>
  __device__ __forceinline__ float from(float eu, float ec, float x, const Extra&, int, float&) const;
};

// the CFG combine (ptp_utils.py:73) rounded in the eps dtype as torch rounds it
template <int DT, typename A>
__device__ __forceinline__ float cfg_noise(const A& a, float eu, float ec) {
  auto rd = [](float v) { return DT == P2P_DTYPE_BF16 ? rnd_bf16(v) : DT == P2P_DTYPE_F16 ? rnd_f16(v) : v; };
  if (a.cfg) {
    const float diff = rd(sub_rn(ec, eu));
    const float gd = rd(mul_rn(a.guidance, diff));
    return rd(add_rn(eu, gd));
  }
  return eu;
}

// DT: the eps element type (P2P_DTYPE_*), i.e. the format torch's eager ops round to
template <int DT, typename A>
__device__ __forceinline__ float ddim_from(const A& a, float eu, float ec, float x) {
  auto rd = [](float v) { return DT == P2P_DTYPE_BF16 ? rnd_bf16(v) : DT == P2P_DTYPE_F16 ? rnd_f16(v) : v; };
  const float noise = cfg_noise<DT>(a, eu, ec);
  // a 0-dim f32 factor times a bf16 (f16) tensor: torch casts the factor to bf16 (f16) first
  const float t1 = rd(mul_rn(rd(a.sqrt_beta_t), noise));
  const float x0 = __fdiv_rn(sub_rn(x, t1), a.sqrt_alpha_t);
  const float dir = rd(mul_rn(rd(a.sqrt_one_minus_alpha_prev), noise));
  return add_rn(mul_rn(a.sqrt_alpha_prev, x0), dir);
}

template <int DT>
__device__ __forceinline__ float DdimC::from(float eu, float ec, float x, const Extra&, int, float&) const {
  return ddim_from<DT>(*this, eu, ec, x);
}

// The PLMS step (PNDMScheduler.step, p2p_amd/pndm.py; include/p2p_hip.h p2p_plms_step): the
// CFG-combined eps upcast to f32 (e_new, what the scheduler's history keeps), the linear multistep
// combination m = w[0] e + w[1] h[0] + ... summed left to right, and the transfer
// sample_coeff x - (eps_num m) / eps_den -- f32, every operation rounded on its own
template <typename P>
__device__ __forceinline__ float plms_transfer(const P& p, float e, const float* h, float x) {
  float m = mul_rn(p.w[0], e);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < p.n_hist) m = add_rn(m, mul_rn(p.w[1 + k], h[k]));
  return sub_rn(mul_rn(p.sample_coeff, x), __fdiv_rn(mul_rn(p.eps_num, m), p.eps_den));
}

// the PLMS step's scalars and history pointers by value (see DdimC).  The launcher points the
// hist[] entries past n_hist at x, so all four loads of an element are valid and unconditional
struct PlmsC {
  int cfg, n_hist;
  float guidance, w[5], sample_coeff, eps_num, eps_den;
  const float* hist[4];
  float* hist_out;
  __device__ explicit PlmsC(const p2p_plms_step_args& a)
      : cfg(a.cfg), n_hist(a.n_hist), guidance(a.guidance), w{a.w[0], a.w[1], a.w[2], a.w[3], a.w[4]},
        sample_coeff(a.sample_coeff), eps_num(a.eps_num), eps_den(a.eps_den),
        hist{a.hist[0], a.hist[1], a.hist[2], a.hist[3]}, hist_out(a.hist_out) {}
  struct Extra { f32x4_t h[4]; };
  __device__ __forceinline__ void load(Extra& e, int64_t idx) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) e.h[k] = *reinterpret_cast<const f32x4_t*>(hist[k] + idx);
  }
  __device__ __forceinline__ void store(int64_t idx, const f32x4_t& e_new) const {
    if (hist_out) *reinterpret_cast<f32x4_t*>(hist_out + idx) = e_new;
  }
  template <int DT>
  __device__ __forceinline__ float from(float eu, float ec, float x, const Extra& e, int j, float& e_new) const {
    e_new = cfg_noise<DT>(*this, eu, ec);
    const float h[4] = {e.h[0][j], e.h[1][j], e.h[2][j], e.h[3][j]};
    return plms_transfer(*this, e_new, h, x);
  }
};

// The DPM-Solver++ (2M) step (DPMSolverMultistepScheduler.step, p2p_amd/dpm.py; include/p2p_hip.h
// p2p_dpm_step): the data prediction m0 = (x - sigma_s e) / alpha_s from the CFG-combined eps upcast
// to f32 (m0 is what the scheduler's history keeps), the first-order update x_coeff x - m0_coeff m0
// and, with the previous call's m1, the second-order term - diff_coeff (m0 - m1) -- f32, every
// operation rounded on its own, in dpm.py's order
template <typename P>
__device__ __forceinline__ float dpm_update(const P& p, float e, float m1, float x, float& m0) {
  m0 = __fdiv_rn(sub_rn(x, mul_rn(p.sigma_s, e)), p.alpha_s);
  float o = sub_rn(mul_rn(p.x_coeff, x), mul_rn(p.m0_coeff, m0));
  if (p.n_hist) o = sub_rn(o, mul_rn(p.diff_coeff, sub_rn(m0, m1)));
  return o;
}

// the DPM step's scalars and history pointer by value (see DdimC).  The launcher points hist at x
// when n_hist = 0, so the history load of an element is valid and unconditional
struct DpmC {
  int cfg, n_hist;
  float guidance, sigma_s, alpha_s, x_coeff, m0_coeff, diff_coeff;
  const float* hist;
  float* hist_out;
  __device__ explicit DpmC(const p2p_dpm_step_args& a)
      : cfg(a.cfg), n_hist(a.n_hist), guidance(a.guidance), sigma_s(a.sigma_s), alpha_s(a.alpha_s),
        x_coeff(a.x_coeff), m0_coeff(a.m0_coeff), diff_coeff(a.diff_coeff), hist(a.hist[0]), hist_out(a.hist_out) {}
  struct Extra { f32x4_t h; };
  __device__ __forceinline__ void load(Extra& e, int64_t idx) const {
    e.h = *reinterpret_cast<const f32x4_t*>(hist + idx);
  }
  __device__ __forceinline__ void store(int64_t idx, const f32x4_t& m0) const {
    if (hist_out) *reinterpret_cast<f32x4_t*>(hist_out + idx) = m0;
  }
  // kept: the value the history receives -- this element's data prediction
  template <int DT>
  __device__ __forceinline__ float from(float eu, float ec, float x, const Extra& e, int j, float& kept) const {
    return dpm_update(*this, cfg_noise<DT>(*this, eu, ec), e.h[j], x, kept);
  }
};

// The Direct Inversion edit step (include/p2p_hip.h p2p_direct_step): the DDIM step, and after
// the blend the group's offset row added to the group's source prompt
struct DirectC : DdimC {
  const float* offset;
  __device__ explicit DirectC(const p2p_direct_step_args& a) : DdimC(a), offset(a.offset) {}
};

// The stochastic DDIM step of the DDPM-inversion edit loop (include/p2p_hip.h p2p_ddpm_step): the
// DDIM step with sqrt(1 - a_prev - sigma^2) as its direction factor, then sigma times the group's
// noise row added to every prompt of the group, before the blend
struct DdpmC : DdimC {
  float sigma;
  const float* noise;
  __device__ explicit DdpmC(const p2p_ddpm_step_args& a) : DdimC(a), sigma(a.sigma), noise(a.noise) {}
};

template <typename A> struct StepOf;
template <> struct StepOf<p2p_latent_step_args> { using C = DdimC; };
template <> struct StepOf<p2p_direct_step_args> { using C = DirectC; };
template <> struct StepOf<p2p_ddpm_step_args> { using C = DdpmC; };
template <> struct StepOf<p2p_plms_step_args> { using C = PlmsC; };
template <> struct StepOf<p2p_dpm_step_args> { using C = DpmC; };

template <int DT, typename A>
__device__ __forceinline__ float eps_at(const A& a, int64_t idx) {
  if constexpr (DT == P2P_DTYPE_BF16) return bf2f(static_cast<const uint16_t*>(a.eps)[idx]);
  else if constexpr (DT == P2P_DTYPE_F16) return h2f(static_cast<const uint16_t*>(a.eps)[idx]);
  else return static_cast<const float*>(a.eps)[idx];
}

// prev_sample of prompt b at element i of its [C, H, W] latent
template <int DT>
__device__ __forceinline__ float step_prev(const p2p_latent_step_args& a, int b, int64_t i, int64_t chw) {
  const float eu = eps_at<DT>(a, (int64_t)b * chw + i);
  const float ec = a.cfg ? eps_at<DT>(a, (int64_t)(a.n_prompts + b) * chw + i) : 0.f;
  return ddim_from<DT>(a, eu, ec, a.x[(int64_t)b * chw + i]);
}

// the same for the PLMS step, which also keeps the new eps (hist_out)
template <int DT>
__device__ __forceinline__ float step_prev(const p2p_plms_step_args& a, int b, int64_t i, int64_t chw) {
  const int64_t idx = (int64_t)b * chw + i;
  const float eu = eps_at<DT>(a, idx);
  const float ec = a.cfg ? eps_at<DT>(a, (int64_t)(a.n_prompts + b) * chw + i) : 0.f;
  const float e = cfg_noise<DT>(a, eu, ec);
  float h[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < a.n_hist) h[k] = a.hist[k][idx];
  if (a.hist_out) a.hist_out[idx] = e;
  return plms_transfer(a, e, h, a.x[idx]);
}

// the same for the DPM-Solver++ step, which keeps the new data prediction (hist_out)
template <int DT>
__device__ __forceinline__ float step_prev(const p2p_dpm_step_args& a, int b, int64_t i, int64_t chw) {
  const int64_t idx = (int64_t)b * chw + i;
  const float eu = eps_at<DT>(a, idx);
  const float ec = a.cfg ? eps_at<DT>(a, (int64_t)(a.n_prompts + b) * chw + i) : 0.f;
  const float m1 = a.n_hist ? a.hist[0][idx] : 0.f;
  float m0;
  const float prev = dpm_update(a, cfg_noise<DT>(a, eu, ec), m1, a.x[idx], m0);
  if (a.hist_out) a.hist_out[idx] = m0;
  return prev;
}

// the DDIM step again for the Direct Inversion form (the offset is added by the kernels, after the blend)
template <int DT>
__device__ __forceinline__ float step_prev(const p2p_direct_step_args& a, int b, int64_t i, int64_t chw) {
  const float eu = eps_at<DT>(a, (int64_t)b * chw + i);
  const float ec = a.cfg ? eps_at<DT>(a, (int64_t)(a.n_prompts + b) * chw + i) : 0.f;
  return ddim_from<DT>(a, eu, ec, a.x[(int64_t)b * chw + i]);
}

// mu + sigma z: the product rounded, then the sum (torch's two lines, never an fma)
__device__ __forceinline__ float ddpm_noised(float mu, float sigma, float z) { return add_rn(mu, mul_rn(sigma, z)); }

// the stochastic DDIM step: the noise row is the prompt group's, so prev0 -- what the group's other
// prompts blend towards -- carries it too
template <int DT>
__device__ __forceinline__ float step_prev(const p2p_ddpm_step_args& a, int b, int64_t i, int64_t chw) {
  const float eu = eps_at<DT>(a, (int64_t)b * chw + i);
  const float ec = a.cfg ? eps_at<DT>(a, (int64_t)(a.n_prompts + b) * chw + i) : 0.f;
  const int gs = a.group_size > 0 ? a.group_size : a.n_prompts;
  return ddpm_noised(ddim_from<DT>(a, eu, ec, a.x[(int64_t)b * chw + i]), a.sigma, a.noise[(int64_t)(b / gs) * chw + i]);
}

template <typename A>
constexpr bool kDirectForm = std::is_same<A, p2p_direct_step_args>::value;
template <typename A>
constexpr bool kDdpmForm = std::is_same<A, p2p_ddpm_step_args>::value;

// A: p2p_latent_step_args (DDIM), p2p_plms_step_args, p2p_dpm_step_args, p2p_direct_step_args or
// p2p_ddpm_step_args -- the step form is step_prev's overload.  The Direct Inversion form adds offset[g]
// to group g's source prompt as it is stored: prev0, which the group's other prompts blend towards,
// stays un-offset.  (The DDPM form's noise is part of its step_prev: it is in prev0 as well.)
// (This body and latent_blend_kernel's stay in the kernels: moved into an inlined device function,
// hipcc no longer folds the block size with the launch bounds and schedules the DDIM instantiations
// differently; templated on the argument struct their ISA is the one-form kernels'.)
template <int DT, typename A>
__global__ __launch_bounds__(256) void latent_step_kernel(A a, int64_t chw) {
  const int HW = a.height * a.width;
  const int B = a.n_prompts;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int gs = a.group_size > 0 ? a.group_size : B;   // prompts per prompt group
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chw; i += stride) {
    const int yx = (int)(i % HW);
    float prev0 = 0.f;
    bool blend = false;
    for (int b = 0; b < B; ++b) {
      const int bg = b % gs;                              // position inside its group
      float prev = step_prev<DT>(a, b, i, chw);
      if (bg == 0) {
        prev0 = prev;                                     // the group's source prompt
        blend = a.mask && (!a.group_blend || a.group_blend[b / gs]);
        if constexpr (kDirectForm<A>) prev = add_rn(prev, a.offset[(int64_t)(b / gs) * chw + i]);
      } else if (blend) {
        const float m = a.mask[(int64_t)b * HW + yx] ? 1.f : 0.f;
        prev = add_rn(prev0, mul_rn(m, sub_rn(prev, prev0)));
      }
      a.out[(int64_t)b * chw + i] = prev;
    }
  }
}

// The latent step with LocalBlend's mask built in the same launch (a.blend_sums): grid
// (pixel chunks of 256, prompts).  A workgroup of an edit prompt b whose group blends builds b's
// mask per map pixel from the folded word sums (build_blend_mask: ~160 KB of L2-resident sums, one
// round trip) and updates its chunk of b's latent -- recomputing the group source's prev_sample,
// which it blends towards, from the same inputs (bit-identical to the source workgroup's).  No
// workgroup reads another's output.  The kernel is latency-bound (1 MB per step): every thread
// issues its eps / x loads (4 pixels x 1 channel, for b and the source) before the mask build's,
// so the launch waits about two memory round trips; 64 workgroups keep the per-thread DDIM
// arithmetic (two IEEE divisions per element) short.  The PLMS form (A = p2p_plms_step_args) adds
// its four history loads per prompt to the same batch of loads and one store of the new eps; the
// DPM-Solver++ form (A = p2p_dpm_step_args) adds one history load and one store of the new x0; the
// Direct Inversion form (A = p2p_direct_step_args) one load of the group's offset row, which the
// source prompt's workgroups add to what they store (the edit workgroups recompute the un-offset
// source from the inputs, as before); the DDPM form (A = p2p_ddpm_step_args) one load of the group's
// noise row, which every workgroup of the group adds, times sigma, to its prompt's and to the
// recomputed source's step before it blends.
template <int DT, typename A>
__global__ __launch_bounds__(256, 1) void latent_blend_kernel(A a, int64_t chw, int px_per_wg) {
  // every field this kernel reads, copied to scalars first (see DdimC)
  const int HW = a.height * a.width;
  const int b = blockIdx.y;
  const int NP = a.n_prompts, C = a.channels, H = a.height, W = a.width;
  const int gs = a.group_size > 0 ? a.group_size : NP;
  const int g = b / gs, bg = b - g * gs, b0 = b - bg;
  const float* const ws = a.blend_sums[g];
  const float* const xg = a.x;
  const void* const eg = a.eps;
  float* const og = a.out;
  const int lh = a.blend_lh, res = a.blend_res, use_sub = a.blend_sub;
  const float th_pool = a.blend_th_pool, th_sub = a.blend_th_sub;
  using StepC = typename StepOf<A>::C;
  const StepC dc(a);
  const bool blend = bg != 0 && ws != nullptr;          // workgroup-uniform
  __shared__ BlendLds L;
  // a workgroup covers px_per_wg = 256 pixels x 4 channels per pass: thread t takes channel
  // c0 + t / 64 and 4 adjacent pixels (16-byte pieces; HW % 4 == 0, checked by the launcher)
  const int px = blockIdx.x * px_per_wg + (threadIdx.x & 63) * 4;
  const int pxc = min(px, HW - 4);
  // raw loads first, unconditionally (clamped to valid addresses; the unused ones are discarded),
  // so no load sits in a branch with its own wait: every load of the pass is in flight at once
  constexpr bool k16 = DT != P2P_DTYPE_F32;
  using Raw = typename std::conditional<k16, uint2, f32x4_t>::type;
  auto ld_eps = [eg](int64_t idx) __attribute__((always_inline)) -> Raw {
    if constexpr (k16) return *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(eg) + idx);
    else return *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(eg) + idx);
  };
  auto unpack = [](const Raw& r) __attribute__((always_inline)) -> f32x4_t {
    if constexpr (DT == P2P_DTYPE_BF16)
      return f32x4_t{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                     __uint_as_float(r.y & 0xffff0000u)};
    else if constexpr (DT == P2P_DTYPE_F16)
      return f32x4_t{h2f((uint16_t)(r.x & 0xffffu)), h2f((uint16_t)(r.x >> 16)), h2f((uint16_t)(r.y & 0xffffu)),
                     h2f((uint16_t)(r.y >> 16))};
    else return r;
  };
  for (int c0 = 0; c0 < C; c0 += 4) {
    const int c = c0 + (threadIdx.x >> 6);
    const int64_t i = (int64_t)min(c, C - 1) * HW + pxc;
    Raw reu[2], rec[2];
    f32x4_t xv[2];
    typename StepC::Extra ex[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int bb = s2 ? b0 : b;
      reu[s2] = ld_eps((int64_t)bb * chw + i);
      rec[s2] = ld_eps((int64_t)((dc.cfg ? NP : 0) + bb) * chw + i);
      xv[s2] = *reinterpret_cast<const f32x4_t*>(xg + (int64_t)bb * chw + i);
      dc.load(ex[s2], (int64_t)bb * chw + i);
    }
    f32x4_t offv = {0.f, 0.f, 0.f, 0.f};
    if constexpr (kDirectForm<A>) offv = *reinterpret_cast<const f32x4_t*>(dc.offset + (int64_t)g * chw + i);
    if constexpr (kDdpmForm<A>) offv = *reinterpret_cast<const f32x4_t*>(dc.noise + (int64_t)g * chw + i);
    if (blend && c0 == 0) {
      const int R2 = res * res;
      build_blend_mask(ws, ws + (int64_t)bg * 2 * lh * R2, lh, res, H, W, th_pool, th_sub, use_sub != 0, L);
    }
    if (c >= C || px >= HW) continue;
    const f32x4_t eu = unpack(reu[0]), ec = unpack(rec[0]);
    f32x4_t o;
    float e_new[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float prev = dc.template from<DT>(eu[j], ec[j], xv[0][j], ex[0], j, e_new[j]);
      if constexpr (kDdpmForm<A>) prev = ddpm_noised(prev, dc.sigma, offv[j]);
      if (blend) {
        const f32x4_t eu0 = unpack(reu[1]), ec0 = unpack(rec[1]);
        float e0;
        float prev0 = dc.template from<DT>(eu0[j], ec0[j], xv[1][j], ex[1], j, e0);
        if constexpr (kDdpmForm<A>) prev0 = ddpm_noised(prev0, dc.sigma, offv[j]);
        const float m = L.msrc[blend_src_of(px + j, res, H, W)];
        prev = add_rn(prev0, mul_rn(m, sub_rn(prev, prev0)));
      }
      if constexpr (kDirectForm<A>)
        if (bg == 0) prev = add_rn(prev, offv[j]);
      o[j] = prev;
    }
    *reinterpret_cast<f32x4_t*>(og + (int64_t)b * chw + (int64_t)c * HW + px) = o;
    dc.store((int64_t)b * chw + (int64_t)c * HW + px, f32x4_t{e_new[0], e_new[1], e_new[2], e_new[3]});
  }
}

// The checks and launch geometry the DDIM and PLMS latent steps share.  Returns a P2P_E_* code, or
// 0 with `fused` telling which form launches (the one-launch LocalBlend, or the plain / mask form)
template <typename A>
static int check_latent_args(const A& a, bool& fused) {
  if (!a.eps || !a.x || !a.out || a.n_prompts < 1 || a.channels < 1 || a.height < 1 || a.width < 1 ||
      a.group_size < 0 || (a.group_size > 0 && a.n_prompts % a.group_size))
    return P2P_E_ARG;
  if (a.eps_dtype != P2P_DTYPE_F32 && a.eps_dtype != P2P_DTYPE_BF16 && a.eps_dtype != P2P_DTYPE_F16)
    return P2P_E_DTYPE;
  const int gs = a.group_size > 0 ? a.group_size : a.n_prompts;
  const int n_groups = a.n_prompts / gs;
  fused = false;
  for (int g = 0; g < P2P_MAX_GROUPS; ++g) {
    if (!a.blend_sums[g]) continue;
    if (g >= n_groups) return P2P_E_ARG;
    fused = true;
  }
  if (fused) {
    // the mask comes from the word sums; a precomputed mask as well would be ambiguous.  out must
    // not alias x: a source workgroup's writes would race with the edit workgroups' reads of x[g0]
    if (a.mask || a.group_blend || a.out == a.x || a.blend_lh < 1 || a.blend_res < 1 || (a.height * a.width) % 4 ||
        ((uintptr_t)a.x | (uintptr_t)a.out | (uintptr_t)a.eps) % 16 ||
        a.blend_res * a.blend_res > 256 || a.blend_res > a.height || a.blend_res > a.width)
      return P2P_E_ARG;
  }
  return 0;
}

constexpr int kLatentPx = 256;    // latent pixels per workgroup (x 4 channels: 256 threads x 4 elements)

// the launch both kernels' step forms share: the one-launch LocalBlend (fused) or the plain / mask form
template <typename A>
static int launch_latent_form(const A& a, bool fused, hipStream_t st) {
  const int64_t chw = (int64_t)a.channels * a.height * a.width;
  if (fused) {
    const int hw = a.height * a.width;
    dim3 grid((hw + kLatentPx - 1) / kLatentPx, a.n_prompts);
    if (a.eps_dtype == P2P_DTYPE_BF16)
      launch_kernel(latent_blend_kernel<P2P_DTYPE_BF16, A>, grid, dim3(256), 0, st, a, chw, kLatentPx);
    else if (a.eps_dtype == P2P_DTYPE_F16)
      launch_kernel(latent_blend_kernel<P2P_DTYPE_F16, A>, grid, dim3(256), 0, st, a, chw, kLatentPx);
    else
      launch_kernel(latent_blend_kernel<P2P_DTYPE_F32, A>, grid, dim3(256), 0, st, a, chw, kLatentPx);
    return (int)hipGetLastError();
  }
  int64_t blocks = (chw + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (a.eps_dtype == P2P_DTYPE_BF16)
    launch_kernel(latent_step_kernel<P2P_DTYPE_BF16, A>, dim3((unsigned)blocks), dim3(256), 0, st, a, chw);
  else if (a.eps_dtype == P2P_DTYPE_F16)
    launch_kernel(latent_step_kernel<P2P_DTYPE_F16, A>, dim3((unsigned)blocks), dim3(256), 0, st, a, chw);
  else
    launch_kernel(latent_step_kernel<P2P_DTYPE_F32, A>, dim3((unsigned)blocks), dim3(256), 0, st, a, chw);
  return (int)hipGetLastError();
}

int run_latent_step(const p2p_latent_step_args& a, hipStream_t st) {
  bool fused = false;
  if (const int rc = check_latent_args(a, fused)) return rc;
  return launch_latent_form(a, fused, st);
}

int run_plms_step(const p2p_plms_step_args& in, hipStream_t st) {
  bool fused = false;
  if (const int rc = check_latent_args(in, fused)) return rc;
  if (in.n_hist < 0 || in.n_hist > 4 || in.eps_den == 0.f) return P2P_E_ARG;
  if (in.hist_out && (in.hist_out == in.x || in.hist_out == in.out)) return P2P_E_ARG;
  uintptr_t ptr_bits = (uintptr_t)in.hist_out;
  for (int k = 0; k < in.n_hist; ++k) {
    if (!in.hist[k] || in.hist[k] == in.hist_out) return P2P_E_ARG;
    ptr_bits |= (uintptr_t)in.hist[k];
  }
  if (fused && ptr_bits % 16) return P2P_E_ARG;
  p2p_plms_step_args a = in;
  // the one-launch form loads all four history slots of an element unconditionally: the unused
  // ones read x (a valid f32 tensor of the same shape, 16-byte aligned), and are discarded
  for (int k = a.n_hist; k < 4; ++k) a.hist[k] = a.x;
  return launch_latent_form(a, fused, st);
}

int run_dpm_step(const p2p_dpm_step_args& in, hipStream_t st) {
  bool fused = false;
  if (const int rc = check_latent_args(in, fused)) return rc;
  if (in.n_hist < 0 || in.n_hist > 1 || in.alpha_s == 0.f) return P2P_E_ARG;
  if (in.hist_out && (in.hist_out == in.x || in.hist_out == in.out)) return P2P_E_ARG;
  uintptr_t ptr_bits = (uintptr_t)in.hist_out;
  if (in.n_hist) {
    if (!in.hist[0] || in.hist[0] == in.hist_out) return P2P_E_ARG;
    ptr_bits |= (uintptr_t)in.hist[0];
  }
  if (fused && ptr_bits % 16) return P2P_E_ARG;
  p2p_dpm_step_args a = in;
  // the one-launch form loads the history slot unconditionally (see run_plms_step)
  if (!a.n_hist) a.hist[0] = a.x;
  return launch_latent_form(a, fused, st);
}

int run_direct_step(const p2p_direct_step_args& a, hipStream_t st) {
  bool fused = false;
  if (!a.offset) return P2P_E_ARG;
  if (const int rc = check_latent_args(a, fused)) return rc;
  const int gs = a.group_size > 0 ? a.group_size : a.n_prompts;
  const int64_t chw = (int64_t)a.channels * a.height * a.width;
  const uintptr_t off0 = (uintptr_t)a.offset, off1 = off0 + (uintptr_t)(a.n_prompts / gs) * chw * 4;
  const uintptr_t lat_bytes = (uintptr_t)a.n_prompts * chw * 4;
  for (const uintptr_t p : {(uintptr_t)a.x, (uintptr_t)a.out})
    if (off0 < p + lat_bytes && p < off1) return P2P_E_ARG;
  if (fused && off0 % 16) return P2P_E_ARG;
  return launch_latent_form(a, fused, st);
}

int run_ddpm_step(const p2p_ddpm_step_args& a, hipStream_t st) {
  bool fused = false;
  if (!a.noise || !(a.sigma >= 0.f) || __builtin_isinf(a.sigma)) return P2P_E_ARG;   // (NaN fails the comparison)
  if (const int rc = check_latent_args(a, fused)) return rc;
  const int gs = a.group_size > 0 ? a.group_size : a.n_prompts;
  const int64_t chw = (int64_t)a.channels * a.height * a.width;
  const uintptr_t nz0 = (uintptr_t)a.noise, nz1 = nz0 + (uintptr_t)(a.n_prompts / gs) * chw * 4;
  const uintptr_t lat_bytes = (uintptr_t)a.n_prompts * chw * 4;
  for (const uintptr_t p : {(uintptr_t)a.x, (uintptr_t)a.out})
    if (nz0 < p + lat_bytes && p < nz1) return P2P_E_ARG;
  if (fused && nz0 % 16) return P2P_E_ARG;
  return launch_latent_form(a, fused, st);
}

// ---------------------------------------------------------------- Direct Inversion offsets
// offset[r] = target[r] - prev_step(cfg(eps_u[r], eps_c[r]), x[r]) for R rows, each with its own
// DDIM coefficients read from device memory (include/p2p_hip.h p2p_direct_offset): grid (chunks of
// 256 threads x 4 elements, R).  ddim_from is the latent step's, so a row's prev_step is that
// kernel's bit for bit.
struct OffsetC {
  int cfg;
  float guidance, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_one_minus_alpha_prev;
};

template <int DT>
__global__ __launch_bounds__(256) void direct_offset_kernel(p2p_direct_offset_args a) {
  const int r = blockIdx.y;
  const int iv = blockIdx.x * 256 + threadIdx.x;      // 4-element piece of row r
  if (iv >= a.n / 4) return;
  const f32x4_t cv = reinterpret_cast<const f32x4_t*>(a.coef)[r];
  const OffsetC c{1, a.guidance, cv[0], cv[1], cv[2], cv[3]};
  const int64_t i = (int64_t)r * a.n + (int64_t)iv * 4;
  const int64_t ic = (int64_t)(a.R + r) * a.n + (int64_t)iv * 4;
  f32x4_t eu, ec;
  if constexpr (DT == P2P_DTYPE_F32) {
    eu = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(a.eps) + i);
    ec = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(a.eps) + ic);
  } else {
    const uint2 ru = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(a.eps) + i);
    const uint2 rc = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(a.eps) + ic);
    auto widen = [](uint32_t v) { return DT == P2P_DTYPE_BF16 ? bf2f((uint16_t)v) : h2f((uint16_t)v); };
    eu = f32x4_t{widen(ru.x & 0xffffu), widen(ru.x >> 16), widen(ru.y & 0xffffu), widen(ru.y >> 16)};
    ec = f32x4_t{widen(rc.x & 0xffffu), widen(rc.x >> 16), widen(rc.y & 0xffffu), widen(rc.y >> 16)};
  }
  const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(a.x + i);
  const f32x4_t tv = *reinterpret_cast<const f32x4_t*>(a.target + i);
  f32x4_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = sub_rn(tv[j], ddim_from<DT>(c, eu[j], ec[j], xv[j]));
  *reinterpret_cast<f32x4_t*>(a.offset + i) = o;
}

constexpr int kOffsetMaxRows = 65535;   // grid.y

int run_direct_offset(const p2p_direct_offset_args& a, hipStream_t st) {
  if (!a.eps || !a.x || !a.target || !a.coef || !a.offset) return P2P_E_ARG;
  if (a.R <= 0 || a.n <= 0) return P2P_E_ARG;
  if (a.eps_dtype != P2P_DTYPE_F32 && a.eps_dtype != P2P_DTYPE_BF16 && a.eps_dtype != P2P_DTYPE_F16)
    return P2P_E_DTYPE;
  if (a.R > kOffsetMaxRows) return P2P_E_BATCH;
  if (a.n % 4) return P2P_E_ALIGN;
  // (four elements per access: 16 bytes of f32, 8 of a 16-bit eps, and every row starts on such a boundary)
  if (((uintptr_t)a.eps | (uintptr_t)a.x | (uintptr_t)a.target | (uintptr_t)a.coef | (uintptr_t)a.offset) & 15)
    return P2P_E_ALIGN;
  const dim3 grid((unsigned)((a.n / 4 + 255) / 256), (unsigned)a.R);
  if (a.eps_dtype == P2P_DTYPE_BF16)
    launch_kernel(direct_offset_kernel<P2P_DTYPE_BF16>, grid, dim3(256), 0, st, a);
  else if (a.eps_dtype == P2P_DTYPE_F16)
    launch_kernel(direct_offset_kernel<P2P_DTYPE_F16>, grid, dim3(256), 0, st, a);
  else
    launch_kernel(direct_offset_kernel<P2P_DTYPE_F32>, grid, dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- DDPM inversion noise maps
// noise[r] = (target[r] - mu[r]) / sigma[r] for R rows, each with its own five coefficients read from
// device memory (include/p2p_hip.h p2p_ddpm_noise); direct_offset_kernel's geometry.  mu is the
// latent step's ddim_from with c3' as its direction factor, so a row's mu is p2p_ddpm_step's at
// sigma = 0 bit for bit; a row with sigma = 0 (the grid's last step) stores zeros.
template <int DT>
__global__ __launch_bounds__(256) void ddpm_noise_kernel(p2p_ddpm_noise_args a) {
  const int r = blockIdx.y;
  const int iv = blockIdx.x * 256 + threadIdx.x;      // 4-element piece of row r
  if (iv >= a.n / 4) return;
  const float* cr = a.coef + (int64_t)r * 5;
  const OffsetC c{1, a.guidance, cr[0], cr[1], cr[2], cr[3]};
  const float sigma = cr[4];
  const int64_t i = (int64_t)r * a.n + (int64_t)iv * 4;
  const int64_t ic = (int64_t)(a.R + r) * a.n + (int64_t)iv * 4;
  f32x4_t eu, ec;
  if constexpr (DT == P2P_DTYPE_F32) {
    eu = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(a.eps) + i);
    ec = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(a.eps) + ic);
  } else {
    const uint2 ru = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(a.eps) + i);
    const uint2 rc = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(a.eps) + ic);
    auto widen = [](uint32_t v) { return DT == P2P_DTYPE_BF16 ? bf2f((uint16_t)v) : h2f((uint16_t)v); };
    eu = f32x4_t{widen(ru.x & 0xffffu), widen(ru.x >> 16), widen(ru.y & 0xffffu), widen(ru.y >> 16)};
    ec = f32x4_t{widen(rc.x & 0xffffu), widen(rc.x >> 16), widen(rc.y & 0xffffu), widen(rc.y >> 16)};
  }
  const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(a.x + i);
  const f32x4_t tv = *reinterpret_cast<const f32x4_t*>(a.target + i);
  f32x4_t o = {0.f, 0.f, 0.f, 0.f};
  if (sigma > 0.f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __fdiv_rn(sub_rn(tv[j], ddim_from<DT>(c, eu[j], ec[j], xv[j])), sigma);
  }
  *reinterpret_cast<f32x4_t*>(a.noise + i) = o;
}

int run_ddpm_noise(const p2p_ddpm_noise_args& a, hipStream_t st) {
  if (!a.eps || !a.x || !a.target || !a.coef || !a.noise) return P2P_E_ARG;
  if (a.R <= 0 || a.n <= 0) return P2P_E_ARG;
  if (a.eps_dtype != P2P_DTYPE_F32 && a.eps_dtype != P2P_DTYPE_BF16 && a.eps_dtype != P2P_DTYPE_F16)
    return P2P_E_DTYPE;
  if (a.R > kOffsetMaxRows) return P2P_E_BATCH;
  if (a.n % 4) return P2P_E_ALIGN;
  if (((uintptr_t)a.eps | (uintptr_t)a.x | (uintptr_t)a.target | (uintptr_t)a.coef | (uintptr_t)a.noise) & 15)
    return P2P_E_ALIGN;
  const dim3 grid((unsigned)((a.n / 4 + 255) / 256), (unsigned)a.R);
  if (a.eps_dtype == P2P_DTYPE_BF16)
    launch_kernel(ddpm_noise_kernel<P2P_DTYPE_BF16>, grid, dim3(256), 0, st, a);
  else if (a.eps_dtype == P2P_DTYPE_F16)
    launch_kernel(ddpm_noise_kernel<P2P_DTYPE_F16>, grid, dim3(256), 0, st, a);
  else
    launch_kernel(ddpm_noise_kernel<P2P_DTYPE_F32>, grid, dim3(256), 0, st, a);
  return (int)hipGetLastError();
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
