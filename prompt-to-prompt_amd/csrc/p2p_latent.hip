// The fused latent update of one denoising step, in five step forms (DDIM, PLMS, DPM-Solver++,
// Direct Inversion, DDPM inversion), and the two inversions' row kernel.
//
// One denoising step's latent update (ptp_utils.py:72-75): classifier-free guidance
// (:73), the DDIM step (diffusers DDIMScheduler.step with eta = 0, restated by the reference as
// NullInversion.prev_step, null_text.py:471-479; the same formula with the inversion's
// coefficients is next_step, :481-489) and the LocalBlend latent blend with a precomputed mask
// (null_text.py:68-70 / main.py:50-52).  Every intermediate is rounded where the reference's
// torch ops round it: to bf16 (f16) for the products torch keeps in the U-Net's bf16 (f16) output dtype,
// to f32 elsewhere, with no fma contraction -- so the update is bit-identical to the eager
// sequence on the same inputs.
//
// A step form is written once, as a policy struct (DdimC, PlmsC, DpmC, DirectC, DdpmC): its
// coefficients, the tensors it reads and writes beside eps / x / out, and its arithmetic.  Both
// kernels -- latent_step_kernel (one element per thread) and latent_blend_kernel (four, with
// LocalBlend's mask built in the launch) -- go through it; a new form is one struct, one StepOf
// line and one run_* function.
#include <type_traits>

#include "p2p_blend_mask.h"
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

__device__ __forceinline__ float rnd_bf16(float x) { return bf2f(f2bf(x)); }
__device__ __forceinline__ float rnd_f16(float x) { return h2f(f2h(x)); }

// explicit round-to-nearest ops: no fma contraction whatever the compile flags
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }

// How a kernel hands a form one element of a tensor operand (V: what a thread holds per tensor).
// latent_blend_kernel (V = f32x4_t, four adjacent elements) loads the 16-byte piece with its batch of
// unconditional loads and hands over the register; latent_step_kernel (V = float), bound by its
// traffic, hands over the element's index, and the form reads or writes memory where it uses the
// operand -- so that kernel touches only what a step uses, in the step's own order.
template <typename V> constexpr bool kReg = !std::is_same<V, float>::value;
template <typename V> using Operand = typename std::conditional<kReg<V>, V, int64_t>::type;
template <typename V>
__device__ __forceinline__ Operand<V> fetch(const float* t, int64_t idx) {
  if constexpr (kReg<V>) return *reinterpret_cast<const V*>(t + idx);
  else return idx;
}
__device__ __forceinline__ float read(const float* t, int64_t idx, int) { return t[idx]; }
__device__ __forceinline__ float read(const float*, const f32x4_t& v, int j) { return v[j]; }
// what a form keeps for a nullable tensor t: written at once, or left in the register `store` writes
__device__ __forceinline__ void keep(float* t, const int64_t& idx, float v) { t[idx] = v; }
__device__ __forceinline__ void keep(float*, float& reg, float v) { reg = v; }
// the latent x is the kernel's: its address, or its register
__device__ __forceinline__ float lane(const float* p, int) { return *p; }
__device__ __forceinline__ float lane(const f32x4_t& v, int j) { return v[j]; }

// the CFG combine (ptp_utils.py:73) rounded in the eps dtype as torch rounds it
// DT: the eps element type (P2P_DTYPE_*), i.e. the format torch's eager ops round to
template <int DT, typename C>
__device__ __forceinline__ float cfg_noise(const C& c, float eu, float ec) {
  auto rd = [](float v) { return DT == P2P_DTYPE_BF16 ? rnd_bf16(v) : DT == P2P_DTYPE_F16 ? rnd_f16(v) : v; };
  if (c.cfg) {
    const float diff = rd(sub_rn(ec, eu));
    const float gd = rd(mul_rn(c.guidance, diff));
    return rd(add_rn(eu, gd));
  }
  return eu;
}

// What a form may add to the DDIM step, with the defaults that add nothing:
//   Extra<V>, load     the per-prompt tensors it reads beside eps and x, at element idx of [B, C, H, W]
//   row                its prompt group g's row at element i of the group's [C, H, W]
//   from<DT>           prev_sample of element j from its inputs -- eu / ec the unconditional and
//                      conditional eps (ec unused without CFG), x the latent, z the row -- before
//                      the blend; `kept` takes what the form keeps per prompt (see keep)
//   source_stored      what the group's source prompt stores for its prev_sample
//   store              the 16-byte piece of the kept tensor (latent_blend_kernel)
// What the two kernels hand over, PLMS as the example (idx = b * chw + i):
//                      latent_step_kernel (V = float)         latent_blend_kernel (V = f32x4_t)
//   Extra<V>::h[k]     idx; `from` reads hist[k][idx],        the 16 bytes at hist[k] + idx, loaded for
//                      and only for k < n_hist                all four k with the batch; `from` takes lane j
//   x                  the address x + idx, read in `from`    the register xv; `from` takes lane j
//   z (Direct, DDPM)   the row index g * chw + i; read by     the row's 16 bytes; lane j
//                      the hook that adds it
//   kept               idx; `from` writes hist_out[idx]       a float of the thread; the kernel packs four
//                      at once if hist_out is set             and `store` writes them if hist_out is set
// so a form writes its arithmetic once on read() / lane() / keep(), and `kReg<V> ||` marks a guard that
// only latent_step_kernel needs (there an unused slot is not read; in a register it already is).
struct StepBase {
  template <typename V> struct Extra {};
  template <typename V> __device__ __forceinline__ void load(Extra<V>&, int64_t) const {}
  template <typename V> __device__ __forceinline__ Operand<V> row(int, int64_t, int64_t) const { return Operand<V>{}; }
  template <typename Z> __device__ __forceinline__ float source_stored(float prev, const Z&, int) const { return prev; }
  template <typename V> __device__ __forceinline__ void store(int64_t, const V&) const {}
};

// the step's scalar coefficients, copied out of the kernel-argument struct by value (a kernel that
// also indexes the struct's blend_sums[] array at run time would otherwise read every field through
// a vector load of the kernarg segment, one dependent round trip each)
struct DdimC : StepBase {
  int cfg;
  float guidance, sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_one_minus_alpha_prev;
  template <typename A>   // p2p_latent_step_args, p2p_direct_step_args or p2p_ddpm_step_args (the same fields)
  __device__ explicit DdimC(const A& a)
      : cfg(a.cfg), guidance(a.guidance), sqrt_beta_t(a.sqrt_beta_t), sqrt_alpha_t(a.sqrt_alpha_t),
        sqrt_alpha_prev(a.sqrt_alpha_prev), sqrt_one_minus_alpha_prev(a.sqrt_one_minus_alpha_prev) {}
  // a row kernel's row: always guided, its own four factors
  __device__ DdimC(float guidance, float c0, float c1, float c2, float c3)
      : cfg(1), guidance(guidance), sqrt_beta_t(c0), sqrt_alpha_t(c1), sqrt_alpha_prev(c2),
        sqrt_one_minus_alpha_prev(c3) {}
  // CFG combine + DDIM step
  template <int DT>
  __device__ __forceinline__ float ddim(float eu, float ec, float x) const {
    auto rd = [](float v) { return DT == P2P_DTYPE_BF16 ? rnd_bf16(v) : DT == P2P_DTYPE_F16 ? rnd_f16(v) : v; };
    const float noise = cfg_noise<DT>(*this, eu, ec);
    // a 0-dim f32 factor times a bf16 (f16) tensor: torch casts the factor to bf16 (f16) first
    const float t1 = rd(mul_rn(rd(sqrt_beta_t), noise));
    const float x0 = __fdiv_rn(sub_rn(x, t1), sqrt_alpha_t);
    const float dir = rd(mul_rn(rd(sqrt_one_minus_alpha_prev), noise));
    return add_rn(mul_rn(sqrt_alpha_prev, x0), dir);
  }
  template <int DT, typename X, typename V, typename Z, typename K>
  __device__ __forceinline__ float from(float eu, float ec, const X& x, const Extra<V>&, int j, const Z&, K&) const {
    return ddim<DT>(eu, ec, lane(x, j));
  }
};

// The PLMS step (PNDMScheduler.step, p2p_amd/pndm.py; include/p2p_hip.h p2p_plms_step): the
// CFG-combined eps upcast to f32 (e_new, what the scheduler's history keeps), the linear multistep
// combination m = w[0] e + w[1] h[0] + ... summed left to right, and the transfer
// sample_coeff x - (eps_num m) / eps_den -- f32, every operation rounded on its own.
// The scalars and history pointers by value (see DdimC).  The launcher points the hist[] entries
// past n_hist at x, so all four 16-byte loads of latent_blend_kernel are valid and unconditional
struct PlmsC : StepBase {
  int cfg, n_hist;
  float guidance, w[5], sample_coeff, eps_num, eps_den;
  const float* hist[4];
  float* hist_out;
  __device__ explicit PlmsC(const p2p_plms_step_args& a)
      : cfg(a.cfg), n_hist(a.n_hist), guidance(a.guidance), w{a.w[0], a.w[1], a.w[2], a.w[3], a.w[4]},
        sample_coeff(a.sample_coeff), eps_num(a.eps_num), eps_den(a.eps_den),
        hist{a.hist[0], a.hist[1], a.hist[2], a.hist[3]}, hist_out(a.hist_out) {}
  template <typename V> struct Extra { Operand<V> h[4]; };
  template <typename V>
  __device__ __forceinline__ void load(Extra<V>& e, int64_t idx) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) e.h[k] = fetch<V>(hist[k], idx);
  }
  template <typename V>
  __device__ __forceinline__ void store(int64_t idx, const V& e_new) const {
    if (hist_out) *reinterpret_cast<V*>(hist_out + idx) = e_new;
  }
  template <int DT, typename X, typename V, typename Z, typename K>
  __device__ __forceinline__ float from(float eu, float ec, const X& x, const Extra<V>& e, int j, const Z&,
                                        K& kept) const {
    const float e_new = cfg_noise<DT>(*this, eu, ec);
    float h[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (kReg<V> || k < n_hist) h[k] = read(hist[k], e.h[k], j);
    if (kReg<V> || hist_out) keep(hist_out, kept, e_new);
    const float xj = lane(x, j);
    float m = mul_rn(w[0], e_new);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n_hist) m = add_rn(m, mul_rn(w[1 + k], h[k]));
    return sub_rn(mul_rn(sample_coeff, xj), __fdiv_rn(mul_rn(eps_num, m), eps_den));
  }
};

// The DPM-Solver++ (2M) step (DPMSolverMultistepScheduler.step, p2p_amd/dpm.py; include/p2p_hip.h
// p2p_dpm_step): the data prediction m0 = (x - sigma_s e) / alpha_s from the CFG-combined eps upcast
// to f32 (m0 is what the scheduler's history keeps), the first-order update x_coeff x - m0_coeff m0
// and, with the previous call's m1, the second-order term - diff_coeff (m0 - m1) -- f32, every
// operation rounded on its own, in dpm.py's order.
// The scalars and history pointer by value (see DdimC).  The launcher points hist at x when
// n_hist = 0, so latent_blend_kernel's history load is valid and unconditional (see PlmsC)
struct DpmC : StepBase {
  int cfg, n_hist;
  float guidance, sigma_s, alpha_s, x_coeff, m0_coeff, diff_coeff;
  const float* hist;
  float* hist_out;
  __device__ explicit DpmC(const p2p_dpm_step_args& a)
      : cfg(a.cfg), n_hist(a.n_hist), guidance(a.guidance), sigma_s(a.sigma_s), alpha_s(a.alpha_s),
        x_coeff(a.x_coeff), m0_coeff(a.m0_coeff), diff_coeff(a.diff_coeff), hist(a.hist[0]), hist_out(a.hist_out) {}
  template <typename V> struct Extra { Operand<V> h; };
  template <typename V>
  __device__ __forceinline__ void load(Extra<V>& e, int64_t idx) const { e.h = fetch<V>(hist, idx); }
  template <typename V>
  __device__ __forceinline__ void store(int64_t idx, const V& m0) const {
    if (hist_out) *reinterpret_cast<V*>(hist_out + idx) = m0;
  }
  // kept: the value the history receives -- this element's data prediction
  template <int DT, typename X, typename V, typename Z, typename K>
  __device__ __forceinline__ float from(float eu, float ec, const X& x, const Extra<V>& e, int j, const Z&,
                                        K& kept) const {
    const float m1 = kReg<V> || n_hist ? read(hist, e.h, j) : 0.f;
    const float e_new = cfg_noise<DT>(*this, eu, ec), xj = lane(x, j);
    const float m0 = __fdiv_rn(sub_rn(xj, mul_rn(sigma_s, e_new)), alpha_s);
    float o = sub_rn(mul_rn(x_coeff, xj), mul_rn(m0_coeff, m0));
    if (n_hist) o = sub_rn(o, mul_rn(diff_coeff, sub_rn(m0, m1)));
    if (kReg<V> || hist_out) keep(hist_out, kept, m0);
    return o;
  }
};

// The Direct Inversion edit step (include/p2p_hip.h p2p_direct_step): the DDIM step, and after
// the blend the group's offset row added to the group's source prompt as it is stored -- the
// source's prev_sample, which the group's other prompts blend towards, stays un-offset.
struct DirectC : DdimC {
  const float* offset;
  __device__ explicit DirectC(const p2p_direct_step_args& a) : DdimC(a), offset(a.offset) {}
  template <typename V> __device__ __forceinline__ Operand<V> row(int g, int64_t chw, int64_t i) const {
    return fetch<V>(offset, (int64_t)g * chw + i);
  }
  template <typename Z>
  __device__ __forceinline__ float source_stored(float prev, const Z& z, int j) const {
    return add_rn(prev, read(offset, z, j));
  }
};

// The stochastic DDIM step of the DDPM-inversion edit loop (include/p2p_hip.h p2p_ddpm_step): the
// DDIM step with sqrt(1 - a_prev - sigma^2) as its direction factor, then sigma times the group's
// noise row added to every prompt of the group, before the blend -- so the source's prev_sample,
// which the group's other prompts blend towards, carries it too
struct DdpmC : DdimC {
  float sigma;
  const float* noise;
  __device__ explicit DdpmC(const p2p_ddpm_step_args& a) : DdimC(a), sigma(a.sigma), noise(a.noise) {}
  template <typename V> __device__ __forceinline__ Operand<V> row(int g, int64_t chw, int64_t i) const {
    return fetch<V>(noise, (int64_t)g * chw + i);
  }
  // mu + sigma z: the product rounded, then the sum (torch's two lines, never an fma)
  template <int DT, typename X, typename V, typename Z, typename K>
  __device__ __forceinline__ float from(float eu, float ec, const X& x, const Extra<V>&, int j, const Z& z, K&) const {
    return add_rn(ddim<DT>(eu, ec, lane(x, j)), mul_rn(sigma, read(noise, z, j)));
  }
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

// prev_sample of prompt b at element i of its [C, H, W] latent, before the blend (the loads of one
// element; a device function as the per-form overloads it replaces were, and the loop stays in the kernel)
template <int DT, typename A, typename StepC>
__device__ __forceinline__ float step_prev(const A& a, const StepC& dc, int b, int64_t i, int64_t chw, int64_t z) {
  const int64_t idx = (int64_t)b * chw + i;
  const float eu = eps_at<DT>(a, idx);
  const float ec = dc.cfg ? eps_at<DT>(a, (int64_t)(a.n_prompts + b) * chw + i) : 0.f;
  typename StepC::template Extra<float> ex;
  dc.load(ex, idx);
  return dc.template from<DT>(eu, ec, a.x + idx, ex, 0, z, idx);
}

// A: p2p_latent_step_args (DDIM), p2p_plms_step_args, p2p_dpm_step_args, p2p_direct_step_args or
// p2p_ddpm_step_args -- the step form is StepOf<A>.
// (This body and latent_blend_kernel's stay in the kernels: moved into an inlined device function,
// hipcc no longer folds the block size with the launch bounds and schedules the DDIM instantiations
// differently; templated on the argument struct their ISA is the one-form kernels'.)
template <int DT, typename A>
__global__ __launch_bounds__(256) void latent_step_kernel(A a, int64_t chw) {
  using StepC = typename StepOf<A>::C;
  const StepC dc(a);
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
      const int64_t z = dc.template row<float>(b / gs, chw, i);
      float prev = step_prev<DT>(a, dc, b, i, chw, z);
      if (bg == 0) {
        prev0 = prev;                                     // the group's source prompt
        blend = a.mask && (!a.group_blend || a.group_blend[b / gs]);
        prev = dc.source_stored(prev, z, 0);
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
// arithmetic (two IEEE divisions per element) short.  A form's own loads (PLMS: four history loads
// per prompt, DPM-Solver++: one, Direct Inversion and DDPM: one of the group's row) join the same
// batch of loads; the edit workgroups recompute the source with the same `from`, so a row that
// `from` adds (DDPM's noise) is in what they blend towards, and one that `source_stored` adds (Direct's
// offset, on the source prompt's workgroups) is not.
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
    typename StepC::template Extra<f32x4_t> ex[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int bb = s2 ? b0 : b;
      reu[s2] = ld_eps((int64_t)bb * chw + i);
      rec[s2] = ld_eps((int64_t)((dc.cfg ? NP : 0) + bb) * chw + i);
      xv[s2] = *reinterpret_cast<const f32x4_t*>(xg + (int64_t)bb * chw + i);
      dc.load(ex[s2], (int64_t)bb * chw + i);
    }
    const f32x4_t zv = dc.template row<f32x4_t>(g, chw, i);
    if (blend && c0 == 0) {
      const int R2 = res * res;
      build_blend_mask(ws, ws + (int64_t)bg * 2 * lh * R2, lh, res, H, W, th_pool, th_sub, use_sub != 0, L);
    }
    if (c >= C || px >= HW) continue;
    const f32x4_t eu = unpack(reu[0]), ec = unpack(rec[0]);
    f32x4_t o;
    float kept[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float prev = dc.template from<DT>(eu[j], ec[j], xv[0], ex[0], j, zv, kept[j]);
      if (blend) {
        const f32x4_t eu0 = unpack(reu[1]), ec0 = unpack(rec[1]);
        float k0;
        const float prev0 = dc.template from<DT>(eu0[j], ec0[j], xv[1], ex[1], j, zv, k0);
        const float m = L.msrc[blend_src_of(px + j, res, H, W)];
        prev = add_rn(prev0, mul_rn(m, sub_rn(prev, prev0)));
      }
      if (bg == 0) prev = dc.source_stored(prev, zv, j);
      o[j] = prev;
    }
    *reinterpret_cast<f32x4_t*>(og + (int64_t)b * chw + (int64_t)c * HW + px) = o;
    dc.store((int64_t)b * chw + (int64_t)c * HW + px, f32x4_t{kept[0], kept[1], kept[2], kept[3]});
  }
}

static bool known_eps_dtype(int dt) { return dt == P2P_DTYPE_F32 || dt == P2P_DTYPE_BF16 || dt == P2P_DTYPE_F16; }

// f(the eps dtype as a compile-time constant), for a dtype known_eps_dtype accepted
template <typename F>
static void with_eps_dtype(int dt, F&& f) {
  if (dt == P2P_DTYPE_BF16) f(std::integral_constant<int, P2P_DTYPE_BF16>{});
  else if (dt == P2P_DTYPE_F16) f(std::integral_constant<int, P2P_DTYPE_F16>{});
  else f(std::integral_constant<int, P2P_DTYPE_F32>{});
}

// The checks and launch geometry the step forms share.  Returns a P2P_E_* code, or
// 0 with `fused` telling which form launches (the one-launch LocalBlend, or the plain / mask form)
template <typename A>
static int check_latent_args(const A& a, bool& fused) {
  if (!a.eps || !a.x || !a.out || a.n_prompts < 1 || a.channels < 1 || a.height < 1 || a.width < 1 ||
      a.group_size < 0 || (a.group_size > 0 && a.n_prompts % a.group_size))
    return P2P_E_ARG;
  if (!known_eps_dtype(a.eps_dtype)) return P2P_E_DTYPE;
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

// The multistep forms' history (PLMS: up to four stored tensors, DPM-Solver++: one), checked after
// check_latent_args; then the hist[] entries past n_hist are pointed at x: the one-launch form
// loads every slot of an element unconditionally, and the unused ones read x (a valid f32 tensor of
// the same shape, 16-byte aligned) and are discarded
template <typename A>
static int bind_history(A& a, bool fused) {
  constexpr int kSlots = sizeof(a.hist) / sizeof(a.hist[0]);
  if (a.n_hist < 0 || a.n_hist > kSlots) return P2P_E_ARG;
  if (a.hist_out && (a.hist_out == a.x || a.hist_out == a.out)) return P2P_E_ARG;
  uintptr_t ptr_bits = (uintptr_t)a.hist_out;
  for (int k = 0; k < a.n_hist; ++k) {
    if (!a.hist[k] || a.hist[k] == a.hist_out) return P2P_E_ARG;
    ptr_bits |= (uintptr_t)a.hist[k];
  }
  if (fused && ptr_bits % 16) return P2P_E_ARG;
  for (int k = a.n_hist; k < kSlots; ++k) a.hist[k] = a.x;
  return 0;
}

// A prompt group's row tensor (Direct Inversion's offset, DDPM's noise: f32 [groups, C, H, W]),
// checked after check_latent_args: it must not overlap x or out
template <typename A>
static int check_group_rows(const A& a, const float* rows, bool fused) {
  const int gs = a.group_size > 0 ? a.group_size : a.n_prompts;
  const int64_t chw = (int64_t)a.channels * a.height * a.width;
  const uintptr_t r0 = (uintptr_t)rows, r1 = r0 + (uintptr_t)(a.n_prompts / gs) * chw * 4;
  const uintptr_t lat_bytes = (uintptr_t)a.n_prompts * chw * 4;
  for (const uintptr_t p : {(uintptr_t)a.x, (uintptr_t)a.out})
    if (r0 < p + lat_bytes && p < r1) return P2P_E_ARG;
  if (fused && r0 % 16) return P2P_E_ARG;
  return 0;
}

constexpr int kLatentPx = 256;    // latent pixels per workgroup (x 4 channels: 256 threads x 4 elements)

// the launch every step form shares: the one-launch LocalBlend (fused) or the plain / mask form
template <typename A>
static int launch_latent_form(const A& a, bool fused, hipStream_t st) {
  const int64_t chw = (int64_t)a.channels * a.height * a.width;
  const int hw = a.height * a.width;
  const dim3 blend_grid((hw + kLatentPx - 1) / kLatentPx, a.n_prompts);
  int64_t blocks = (chw + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  with_eps_dtype(a.eps_dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (fused) launch_kernel(latent_blend_kernel<DT, A>, blend_grid, dim3(256), 0, st, a, chw, kLatentPx);
    else launch_kernel(latent_step_kernel<DT, A>, dim3((unsigned)blocks), dim3(256), 0, st, a, chw);
  });
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
  if (in.eps_den == 0.f) return P2P_E_ARG;
  p2p_plms_step_args a = in;
  if (const int rc = bind_history(a, fused)) return rc;
  return launch_latent_form(a, fused, st);
}

int run_dpm_step(const p2p_dpm_step_args& in, hipStream_t st) {
  bool fused = false;
  if (const int rc = check_latent_args(in, fused)) return rc;
  if (in.alpha_s == 0.f) return P2P_E_ARG;
  p2p_dpm_step_args a = in;
  if (const int rc = bind_history(a, fused)) return rc;
  return launch_latent_form(a, fused, st);
}

int run_direct_step(const p2p_direct_step_args& a, hipStream_t st) {
  bool fused = false;
  if (!a.offset) return P2P_E_ARG;
  if (const int rc = check_latent_args(a, fused)) return rc;
  if (const int rc = check_group_rows(a, a.offset, fused)) return rc;
  return launch_latent_form(a, fused, st);
}

int run_ddpm_step(const p2p_ddpm_step_args& a, hipStream_t st) {
  bool fused = false;
  if (!a.noise || !(a.sigma >= 0.f) || __builtin_isinf(a.sigma)) return P2P_E_ARG;   // (NaN fails the comparison)
  if (const int rc = check_latent_args(a, fused)) return rc;
  if (const int rc = check_group_rows(a, a.noise, fused)) return rc;
  return launch_latent_form(a, fused, st);
}

// ---------------------------------------------------------------- the inversions' row kernels
// R rows, each with its own DDIM coefficients read from device memory, grid (chunks of 256 threads
// x 4 elements, R); DdimC::ddim is the latent step's, so a row's prev_step is that kernel's bit
// for bit.
//   A = p2p_direct_offset_args (include/p2p_hip.h p2p_direct_offset), coef [R, 4]:
//     offset[r] = target[r] - prev_step(cfg(eps_u[r], eps_c[r]), x[r])
//   A = p2p_ddpm_noise_args (p2p_ddpm_noise), coef [R, 5]:
//     noise[r] = (target[r] - mu[r]) / sigma[r], mu the same step with c3' as its direction factor
//     (p2p_ddpm_step's at sigma = 0 bit for bit); a row with sigma = 0 (the grid's last step)
//     stores zeros.
__host__ __device__ inline float* row_out(const p2p_direct_offset_args& a) { return a.offset; }
__host__ __device__ inline float* row_out(const p2p_ddpm_noise_args& a) { return a.noise; }

template <int DT, typename A>
__global__ __launch_bounds__(256) void row_kernel(A a) {
  constexpr bool kNoise = std::is_same<A, p2p_ddpm_noise_args>::value;
  const int r = blockIdx.y;
  const int iv = blockIdx.x * 256 + threadIdx.x;      // 4-element piece of row r
  if (iv >= a.n / 4) return;
  f32x4_t cv;
  float sigma = 0.f;
  if constexpr (kNoise) {
    const float* cr = a.coef + (int64_t)r * 5;
    cv = f32x4_t{cr[0], cr[1], cr[2], cr[3]};
    sigma = cr[4];
  } else {
    cv = reinterpret_cast<const f32x4_t*>(a.coef)[r];
  }
  const DdimC c(a.guidance, cv[0], cv[1], cv[2], cv[3]);
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
  if (!kNoise || sigma > 0.f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = sub_rn(tv[j], c.template ddim<DT>(eu[j], ec[j], xv[j]));
      o[j] = kNoise ? __fdiv_rn(d, sigma) : d;
    }
  }
  *reinterpret_cast<f32x4_t*>(row_out(a) + i) = o;
}

constexpr int kRowMaxRows = 65535;   // grid.y

template <typename A>
static int run_rows(const A& a, hipStream_t st) {
  if (!a.eps || !a.x || !a.target || !a.coef || !row_out(a)) return P2P_E_ARG;
  if (a.R <= 0 || a.n <= 0) return P2P_E_ARG;
  if (!known_eps_dtype(a.eps_dtype)) return P2P_E_DTYPE;
  if (a.R > kRowMaxRows) return P2P_E_BATCH;
  if (a.n % 4) return P2P_E_ALIGN;
  // (four elements per access: 16 bytes of f32, 8 of a 16-bit eps, and every row starts on such a
  // boundary; the noise form's coef rows of five are read as scalars, only its base is checked)
  if (((uintptr_t)a.eps | (uintptr_t)a.x | (uintptr_t)a.target | (uintptr_t)a.coef | (uintptr_t)row_out(a)) & 15)
    return P2P_E_ALIGN;
  const dim3 grid((unsigned)((a.n / 4 + 255) / 256), (unsigned)a.R);
  with_eps_dtype(a.eps_dtype, [&](auto dt) {
    launch_kernel(row_kernel<decltype(dt)::value, A>, grid, dim3(256), 0, st, a);
  });
  return (int)hipGetLastError();
}

int run_direct_offset(const p2p_direct_offset_args& a, hipStream_t st) { return run_rows(a, st); }
int run_ddpm_noise(const p2p_ddpm_noise_args& a, hipStream_t st) { return run_rows(a, st); }

}  // namespace p2p
