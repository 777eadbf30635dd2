// The general self-attention kernels for MI355X (gfx950): every precision and head dim.
//
// self_attn_fused_kernel : flash-style self-attention (ptp_utils.py:183-208, context=None) with
//                     the source-map injection of AttentionControlEdit.replace_self_attention
//                     (main.py:169-174 / null_text.py:224-230) as a batch index remap.
// self_pv_kernel    : the second half of the materialise protocol (probabilities from HBM, P V).
//
// The kernels follow the transposed-fragment convention of p2p_device.h: S^T = K Q^T and
// O^T = V^T P^T, query on the lane.  Which launch takes which form: p2p_select.h.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

// The materialise protocol's second half (ptp_utils.py:206-207 after a controller rewrote attn):
// O[n] = probs[n*H + h] V[n] with the probabilities read from HBM.  Same Oᵀ = Vᵀ Pᵀ form as the
// fused kernel: the lane (query) reads its row's keys in the Sᵀ accumulator order, 4 consecutive
// keys per 16-byte load (keys (r&3) + 8(r>>2) + 4h), so a half-wave covers 32 bytes of each of its
// 32 rows per instruction and four instructions a 128-byte segment; V tiles are staged in LDS.
template <typename IO, typename MP, int D, int BK, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void self_pv_kernel(SelfArgs a) {
  using EV = typename MP::elem;
  constexpr int DV = (D + 31) / 32 * 32;
  constexpr int NDT = DV / 32;
  constexpr int NSB = BK / 32;
  constexpr int VS = (MP::kElemBytes == 2) ? VStrideBf16<DV>::value : DV;
  constexpr int NT = 64 * WAVES;
  constexpr int CPR = D / 8;
  constexpr int NCH = (BK * CPR + NT - 1) / NT;
  constexpr int VBUF = BK * VS;
  constexpr int VBYTES = 2 * VBUF * (int)sizeof(EV);
  __shared__ __attribute__((aligned(16))) char smem[VBYTES + 16];
  EV* const Vs = reinterpret_cast<EV*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int hh = lane >> 5;
  const int qi = lane & 31;

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = logical % a.n_qtiles;
  const int nh = logical / a.n_qtiles;
  const int h = nh % a.H;
  const int n = nh / a.H;
  const int p = qt * 32 * WAVES + wave * 32 + qi;
  const bool prow = p < a.P;
  const int K = a.K;
  const IO* const vp = static_cast<const IO*>(a.v) + (int64_t)n * a.bsv + h * D;
  IO* const op = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D;
  const float* const pp = a.probs + ((int64_t)(n * a.H + h) * a.P + (prow ? p : 0)) * (int64_t)K;
  const bool vec4 = (K & 3) == 0;

  // zero the LDS image once: pad columns [D, DV) and rows >= K stay zero
  for (int i = tid; i < VBYTES / 4; i += NT) reinterpret_cast<float*>(smem)[i] = 0.f;

  Chunk8<IO> vreg[NCH];
  auto stage_load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      const int row = cidx / CPR;
      const int ch = cidx - row * CPR;
      const int key = kt * BK + row;
      if (cidx < BK * CPR && key < K) vreg[i].load(vp + (int64_t)key * a.ldv + ch * 8); else vreg[i].clear();
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      if (cidx < BK * CPR) {
        const int row = cidx / CPR;
        const int ch = cidx - row * CPR;
        vreg[i].store(Vs + buf * VBUF + row * VS + ch * 8);
      }
    }
  };

  const int ntiles = (K + BK - 1) / BK;
  f32x16_t O[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
  __syncthreads();
  stage_load(0);
  stage_write(0);
  __syncthreads();
  for (int kt = 0; kt < ntiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ntiles) stage_load(kt + 1);
    float sv[NSB][16];
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int key = kt * BK + sb * 32 + 8 * g + 4 * hh;
        if (vec4 && prow && key < K) {  // K % 4 == 0: the 4 keys are all in range together
          const f32x4_t x = *reinterpret_cast<const f32x4_t*>(pp + key);
          sv[sb][4 * g] = x[0];
          sv[sb][4 * g + 1] = x[1];
          sv[sb][4 * g + 2] = x[2];
          sv[sb][4 * g + 3] = x[3];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) sv[sb][4 * g + e] = (prow && key + e < K) ? pp[key + e] : 0.f;
        }
      }
    const EV* Vb = Vs + buf * VBUF;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) pv_block<VS, NDT>(MP{}, O, Vb, sb * 32, sv[sb], lane);
    if (kt + 1 < ntiles) stage_write(buf ^ 1);
    __syncthreads();
  }
  if (prow) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = dt * 32 + 8 * g + 4 * hh;
        if (dd < D)
          store4(op + (int64_t)p * a.ldo + dd, O[dt][4 * g], O[dt][4 * g + 1], O[dt][4 * g + 2],
                 O[dt][4 * g + 3]);
      }
  }
}

// ====================================================================== fused self attention
// The hot kernel (G1/G7: P = K = 4096, d = 40).  Beyond a plain online-softmax (flash) loop:
//  * row sums come out of the PV MFMA: V's first padding column (d..DV) is set to 1 in LDS, so
//    O^T row d accumulates sum_k bf16(p_k) -- the same weights the PV uses -- with no VALU adds
//    (only when DV > D; otherwise the sum is a per-lane VALU sum as before);
//  * lazy rescale (defer-max): the running max only moves -- and O is only rescaled -- when a
//    tile's max exceeds it by more than kRescaleThr (log2 units), so p stays <= 2^kRescaleThr;
//    the decision precedes the tile's exponentiation (the safe order), wave-uniform;
//  * no key-mask support (materialise mode only) and masking code only for a partial last tile.
//  * EXACT (launches that keep maps): the row sum is the f32 sum of the exponentials (VALU adds),
//    not the MFMA sum of their bf16 roundings, so the lse that self_maps_kernel normalises the
//    stored maps with is f32-exact (a peaky row's bf16 rounding would otherwise be ~2e-3).
//  * NOMAX (launches that want O only): no per-tile row max at all.  The first tile sets the
//    reference point from its exact max; later tiles exponentiate against it directly and the
//    row sum that the PV MFMA leaves in the ones column is checked once per tile: a row whose sum
//    passes 2^64 is rescaled by 2^-64 (its reference moves up by 64).  bf16 P has the f32
//    exponent range, so p may grow far past 1 without any loss of relative precision; only a
//    logit jumping more than ~115 (log2 units) above the running reference within one tile could
//    overflow -- that shows as a non-finite row sum, and then the whole workgroup recomputes
//    its tiles with the max-tracking loop.  Saves the 8 v_max3 + reduction + decision of every
//    32 x 32 block (the kernel is VALU-issue-bound at d = 40).
template <typename IO, typename MQ, typename MP, int D, int BK, int WAVES, bool EXACT = false, bool NOMAX = false>
__global__ __launch_bounds__(64 * WAVES) void self_attn_fused_kernel(SelfArgs a) {
  using EK = typename MQ::elem;
  using EV = typename MP::elem;
  constexpr int DK = (D + 15) / 16 * 16;
  constexpr int DV = (D + 31) / 32 * 32;
  constexpr int NKT = DK / 16;
  constexpr int NDT = DV / 32;
  constexpr int NSB = BK / 32;
  constexpr int KS = KStride<DK, MQ::kElemBytes>::value;
  constexpr int VS = (MP::kElemBytes == 2) ? VStrideBf16<DV>::value : DV;
  constexpr int NT = 64 * WAVES;
  constexpr int CPR = D / 8;
  constexpr int NCH = (BK * CPR + NT - 1) / NT;
  constexpr int KPLANE = BK * KS;
  constexpr int KBUF = KPLANE * MQ::planes;
  constexpr int VBUF = BK * VS;
  constexpr int KBYTES = 2 * KBUF * (int)sizeof(EK);
  constexpr int VBYTES = 2 * VBUF * (int)sizeof(EV);
  constexpr bool kOnes = DV > D && !EXACT;       // row sum through the PV MFMA
  // O^T tile / lane-half / register holding row D
  constexpr int kLdt = OnesCol<D>::dt, kLh = OnesCol<D>::h, kLr = OnesCol<D>::r;
  constexpr float kRescaleThr = 8.0f;
  __shared__ __attribute__((aligned(16))) char smem[KBYTES + VBYTES + 16];
  EK* const Ks = reinterpret_cast<EK*>(smem);
  EV* const Vs = reinterpret_cast<EV*>(smem + KBYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int hh = lane >> 5;
  const int qi = lane & 31;

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = logical % a.n_qtiles;
  const int nh = logical / a.n_qtiles;
  const int h = nh % a.H;
  const int n = nh / a.H;
  const int src = a.qk_src[n];
  const int p = qt * 32 * WAVES + wave * 32 + qi;
  const bool prow = p < a.P;
  const int K = a.K;
  const float c = a.scale_log2;

  const IO* const qp = static_cast<const IO*>(a.q) + (int64_t)src * a.bsq + h * D;
  const IO* const kp = static_cast<const IO*>(a.k) + (int64_t)src * a.bsk + h * D;
  const IO* const vp = static_cast<const IO*>(a.v) + (int64_t)n * a.bsv + h * D;

  // LDS image: zero pads; V column D = 1 in every row of both buffers (the row-sum column)
  for (int i = tid; i < (KBYTES + VBYTES) / 4; i += NT) reinterpret_cast<float*>(smem)[i] = 0.f;
  __syncthreads();
  if constexpr (kOnes) {
    for (int r = tid; r < 2 * BK; r += NT) Vs[r * VS + D] = one_elem<EV>();
  }

  typename MQ::frag qf[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int col = 16 * t + 8 * hh;
    qf[t] = (prow && col < D) ? MQ::load_q(qp + (int64_t)p * a.ldq + col) : MQ::zero();
  }

  Chunk8<IO> kreg[NCH], vreg[NCH];
  // Per-lane element offsets inside a tile are loop-invariant (the tile base advances by a
  // wave-uniform stride), so no address VGPR is rewritten inside the loop.  Rows past K load
  // row K-1 instead of a divergent clear path: those keys are masked to -inf, p = 0, and the
  // duplicated K/V rows never contribute.  Chunk slots past the tile are wave-uniform when
  // BK*CPR % 64 == 0.
  // K/V tiles are fetched with range-checked buffer loads: the descriptor spans this (entry,
  // head)'s rows [tile start, K), so chunks of rows past K read as zeros with no tail logic,
  // and the per-lane byte offsets stay loop-invariant (a VMEM address VGPR rewritten inside
  // the loop makes the compiler drain the prefetch with vmcnt(0)).  Chunk slots past the tile
  // are wave-uniform when BK*CPR % 64 == 0.
  uint32_t koff[NCH], voff[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cidx = tid + i * NT;
    const int row = min(cidx / CPR, BK - 1);
    const int ch = cidx - (cidx / CPR) * CPR;
    koff[i] = (uint32_t)((row * (int)a.ldk + ch * 8) * (int)sizeof(IO));
    voff[i] = (uint32_t)((row * (int)a.ldv + ch * 8) * (int)sizeof(IO));
  }
  const int64_t kbytes = ((int64_t)(K - 1) * a.ldk + D) * (int64_t)sizeof(IO);
  const int64_t vbytes = ((int64_t)(K - 1) * a.ldv + D) * (int64_t)sizeof(IO);
  const int64_t kstep = (int64_t)BK * a.ldk * (int64_t)sizeof(IO);
  const int64_t vstep = (int64_t)BK * a.ldv * (int64_t)sizeof(IO);
  auto stage_load = [&](int kt) {
    const __amdgpu_buffer_rsrc_t rk =
        make_rsrc(reinterpret_cast<const char*>(kp) + kt * kstep, kbytes - kt * kstep);
    const __amdgpu_buffer_rsrc_t rv =
        make_rsrc(reinterpret_cast<const char*>(vp) + kt * vstep, vbytes - kt * vstep);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      if ((BK * CPR) % NT == 0 || cidx < BK * CPR) {
        kreg[i].load_buf(rk, koff[i]);
        vreg[i].load_buf(rv, voff[i]);
      }
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      if ((BK * CPR) % NT == 0 || cidx < BK * CPR) {
        const int row = cidx / CPR;
        const int ch = cidx - row * CPR;
        MQ::stage(kreg[i], Ks + buf * KBUF + row * KS + ch * 8, KPLANE);
        vreg[i].store(Vs + buf * VBUF + row * VS + ch * 8);
      }
    }
  };

  const int ntiles = (K + BK - 1) / BK;
  f32x16_t O[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
  float m_run = -INFINITY;  // log2-domain running max (scaled), lagging by < kRescaleThr
  float l_run = 0.f;        // per-lane partial row sum (only when !kOnes)

  stage_load(0);
  stage_write(0);
  // retire every prologue load (Q fragments included) before the loop: otherwise the loop
  // header merge leaves Q "possibly pending" and the first QK^T waits vmcnt(0), draining the
  // tile prefetch on every iteration
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  // one K/V tile; the key mask exists only in the instantiation for a partial last tile (as a
  // runtime branch the compiler if-converted it: ~100 extra VALU per tile on every tile)
  bool bad = false;  // NOMAX: some row sum of this lane went non-finite
  auto tile = [&](int kt, auto masked, auto fast) {
    const int buf = kt & 1;
    if (kt + 1 < ntiles) stage_load(kt + 1);
    float sv[NSB][16];
    const EK* Kb = Ks + buf * KBUF;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) {
      f32x16_t acc = {};
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const typename MQ::frag fa = MQ::load_k(Kb + (sb * 32 + qi) * KS + 16 * t + 8 * hh, KPLANE);
        MQ::mma(acc, fa, qf[t]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sv[sb][r] = acc[r];
    }
    if constexpr (decltype(masked)::value) {
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * BK + sb * 32 + acc_row(r, hh) >= K) sv[sb][r] = -INFINITY;
    }
    if constexpr (!decltype(fast)::value) {
      float mx = -INFINITY;
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sv[sb][r]);
      mx = fmaxf(mx, other_half(mx)) * c;
      // defer-max: move the reference point only when this tile overshoots it by > thr
      if (__builtin_expect(!__all(mx <= m_run + kRescaleThr), 0)) {
        const float mnew = fmaxf(m_run, mx);
        const float alpha = fast_exp2(m_run - mnew);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) O[dt][r] *= alpha;
        l_run *= alpha;
        m_run = mnew;
      }
    }
    float ls = 0.f;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = fast_exp2(fmaf(sv[sb][r], c, -m_run));
        sv[sb][r] = e;
        if constexpr (!kOnes) ls += e;
      }
    if constexpr (!kOnes) l_run += ls;
    const EV* Vb = Vs + buf * VBUF;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) pv_block<VS, NDT>(MP{}, O, Vb, sb * 32, sv[sb], lane);
    if constexpr (decltype(fast)::value) {
      // the row sum so far (ones column; lanes kLh of the pair hold it, the other half a zero
      // pad column): rescale rows past 2^64, flag non-finite ones
      const float own = O[kLdt][kLr];
      const float lsum = own + other_half(own);
      bad |= !(lsum < INFINITY);
      if (__builtin_expect(__any(lsum > 0x1p64f), 0)) {
        if (lsum > 0x1p64f) {
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dt][r] *= 0x1p-64f;
          m_run += 64.f;
        }
      }
    }
    if (kt + 1 < ntiles) stage_write(buf ^ 1);
    __syncthreads();
  };
  const int nfull = K / BK;
  if constexpr (NOMAX) {
    static_assert(kOnes, "NOMAX reads the row sum from the ones column");
    __shared__ int wg_bad;
    if (tid == 0) wg_bad = 0;
    // tile 0 sets every row's reference point from its exact max
    if (nfull == 0) tile(0, std::true_type{}, std::false_type{});
    else tile(0, std::false_type{}, std::false_type{});
    for (int kt = 1; kt < nfull; ++kt) tile(kt, std::false_type{}, std::true_type{});
    if (nfull < ntiles && nfull > 0) tile(nfull, std::true_type{}, std::true_type{});
    if (__any(bad) && lane == 0) wg_bad = 1;
    __syncthreads();
    if (__builtin_expect(wg_bad != 0, 0)) {
      // some row overflowed: the whole workgroup recomputes with the max-tracking loop
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
      m_run = -INFINITY;
      stage_load(0);
      stage_write(0);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
      for (int kt = 0; kt < nfull; ++kt) tile(kt, std::false_type{}, std::false_type{});
      if (nfull < ntiles) tile(nfull, std::true_type{}, std::false_type{});
    }
  } else {
    for (int kt = 0; kt < nfull; ++kt) tile(kt, std::false_type{}, std::false_type{});
    if (nfull < ntiles) tile(nfull, std::true_type{}, std::false_type{});
  }
  float l;
  if constexpr (kOnes) l = __shfl(O[kLdt][kLr], (lane & 31) + 32 * kLh);
  else l = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.f / l;
  if (prow) {
    IO* const op = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D + (int64_t)p * a.ldo;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dd = dt * 32 + 8 * g + 4 * hh;
        if (dd < D)
          store4(op + dd, O[dt][4 * g] * inv, O[dt][4 * g + 1] * inv, O[dt][4 * g + 2] * inv,
                 O[dt][4 * g + 3] * inv);
      }
    // row log-sum-exp for the backward pass (log2 domain, scale folded: p = exp2(c s - lse))
    if (a.lse && hh == 0) a.lse[(int64_t)(n * a.H + h) * a.P + p] = m_run + __log2f(l);
  }
}

// ====================================================================== launchers
template <typename IO, typename MQ, typename MP, int D, int BK, int W>
static int launch_fused(const SelfArgs& a, SelfForm form, hipStream_t st) {
  SelfArgs b = a;
  b.n_qtiles = (a.P + 32 * W - 1) / (32 * W);
  dim3 grid(b.n_qtiles * a.H * a.N), block(64 * W);
  // NOMAX exists where there is a ones column and P is bf16 (p2p_select.h)
  constexpr bool kNoMax = ((D + 31) / 32 * 32) > D && std::is_same<MP, MmaBf16>::value;
  if (form == FORM_EXACT) {
    launch_kernel((self_attn_fused_kernel<IO, MQ, MP, D, BK, W, true>), grid, block, 0, st, b);
  } else if (form == FORM_NOMAX) {
    if constexpr (kNoMax)
      launch_kernel((self_attn_fused_kernel<IO, MQ, MP, D, BK, W, false, true>), grid, block, 0, st, b);
    else
      return P2P_E_ARG;
  } else {
    launch_kernel((self_attn_fused_kernel<IO, MQ, MP, D, BK, W>), grid, block, 0, st, b);
  }
  return (int)hipGetLastError();
}

int launch_self_fused(const SelfArgs& a, int prec, int d, SelfKernel k, hipStream_t st) {
  return with_precision(prec, [&](auto pr) {
    return with_head_dim(d, [&](auto dd) -> int {
      using IO = typename decltype(pr)::IO;
      using MQ = typename decltype(pr)::MQ;
      using MP = typename decltype(pr)::MP;
      constexpr int D = decltype(dd)::value;
      constexpr int BK = fused_bk(D, MP::kElemBytes == 2);
      const SelfKernelInfo& ki = self_info(k);
      if (ki.bk != BK) return P2P_E_ARG;   // a form of another precision / head dim
      if (ki.family == FAM_FUSED) {
        if constexpr (BK == 64 && (D == 40 || D == 80))
          if (ki.waves == 8) return launch_fused<IO, MQ, MP, D, 64, 8>(a, ki.form, st);
        if (ki.waves == 2) return launch_fused<IO, MQ, MP, D, BK, 2>(a, ki.form, st);
        if (ki.waves == 4) return launch_fused<IO, MQ, MP, D, BK, 4>(a, ki.form, st);
        return P2P_E_ARG;
      }
      if (ki.family != FAM_PV) return P2P_E_ARG;
      // the materialise protocol's P V
      SelfArgs b = a;
      constexpr int W = 4;
      b.n_qtiles = (a.P + 32 * W - 1) / (32 * W);
      dim3 grid(b.n_qtiles * a.H * a.N), block(64 * W);
      launch_kernel((self_pv_kernel<IO, MP, D, BK, W>), grid, block, 0, st, b);
      return (int)hipGetLastError();
    });
  });
}

}  // namespace p2p
