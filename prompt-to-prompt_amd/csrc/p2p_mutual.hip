// Mutual self-attention (MasaCtrl, Cao et al., ICCV 2023, §3.2-3.3) for MI355X (gfx950).
//
// mutual_attn_kernel    : O[n] = softmax(Q[n] K[s]^T * scale + M) V[s], s = kv_src[n] -- an edit row
//                         keeps its own queries and reads the source row's keys and values; M admits,
//                         for a query of class c, the keys of entry s whose class is c (the
//                         mask-guided form), or every key when entry s has no key of class c.
// token_classes_kernel  : the per-token classes from the running word sums of the cross maps.
//
// The attention kernel follows the transposed-fragment convention of p2p_device.h (S^T = K Q^T,
// O^T = V^T P^T, query on the lane) and the loop of self_attn_fused_kernel's DEFAULT form
// (p2p_self.hip): double-buffered K/V tiles through range-checked buffer loads, online softmax
// with the deferred maximum.  Which launch takes which tile shape: select_mutual (p2p_select.h).
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

// The class predicate.  A query is one lane (pair), so its class is one bit per lane; the classes of
// a tile's BK keys are a wave-uniform word: lane j of every wave loads the class byte of key
// kt * BK + j one tile ahead (one range-checked byte load per lane and tile, zeros past K) and a
// ballot turns the 64 bytes into the word.  Per lane, once per tile,
//     mw = (every key admitted ? ~0 : class 1 ? word : ~word) & (keys < K) >> 4 * lane-half
// and accumulator register r of 32-key block sb is admitted iff bit 32 sb + (r & 3) + 8 (r >> 2) of
// mw is set: the partial last tile's range mask rides in the same word.  A key that is not admitted
// scores -inf.  A row may meet whole tiles without an admitted key before its first one: its
// running maximum then stays -inf, the exponentials are taken against 0 instead (exp2(-inf) = 0,
// never exp2(-inf - -inf)), and the rescale factor of a row whose maximum does not move is 1.
template <typename IO, typename MQ, typename MP, int D, int BK, int WAVES, bool MASKED>
__global__ __launch_bounds__(64 * WAVES) void mutual_attn_kernel(MutualArgs a) {
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
  constexpr bool kOnes = DV > D;                 // row sum through the PV MFMA (V column D = 1)
  constexpr int kLdt = OnesCol<D>::dt, kLh = OnesCol<D>::h, kLr = OnesCol<D>::r;
  constexpr float kRescaleThr = 8.0f;
  __shared__ __attribute__((aligned(16))) char smem[KBYTES + VBYTES + 16];
  __shared__ int cls_has[2];                     // entry s holds a key of class 0 / of class 1
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
  const int n = a.ent[nh / a.H];                 // the launch's entries with kv_src >= 0
  const int src = a.kv_src[n];
  const int p = qt * 32 * WAVES + wave * 32 + qi;
  const bool prow = p < a.P;
  const int K = a.K;
  const float c = a.scale_log2;

  const IO* const qp = static_cast<const IO*>(a.q) + (int64_t)n * a.bsq + h * D;
  const IO* const kp = static_cast<const IO*>(a.k) + (int64_t)src * a.bsk + h * D;
  const IO* const vp = static_cast<const IO*>(a.v) + (int64_t)src * a.bsv + h * D;
  const bool restrict_keys = MASKED && src != n;                  // (workgroup-uniform)
  const uint8_t* const kcls = MASKED ? a.token_class + (int64_t)src * K : nullptr;

  // LDS image: zero pads; V column D = 1 in every row of both buffers (the row-sum column)
  for (int i = tid; i < (KBYTES + VBYTES) / 4; i += NT) reinterpret_cast<float*>(smem)[i] = 0.f;
  if (tid < 2) cls_has[tid] = 0;
  __syncthreads();
  if constexpr (kOnes) {
    for (int r = tid; r < 2 * BK; r += NT) Vs[r * VS + D] = one_elem<EV>();
  }
  bool qcls = false;
  if constexpr (MASKED) {
    if (restrict_keys) {
      qcls = prow && a.token_class[(int64_t)n * a.P + p] != 0;
      // which classes entry s holds at all (a query of an absent class admits every key)
      bool h0 = false, h1 = false;
      for (int j = tid; j < K; j += NT) {
        const bool one = kcls[j] != 0;
        h1 |= one;
        h0 |= !one;
      }
      if (__any(h0) && lane == 0) cls_has[0] = 1;
      if (__any(h1) && lane == 0) cls_has[1] = 1;
    }
  }

  typename MQ::frag qf[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int col = 16 * t + 8 * hh;
    qf[t] = (prow && col < D) ? MQ::load_q(qp + (int64_t)p * a.ldq + col) : MQ::zero();
  }

  Chunk8<IO> kreg[NCH], vreg[NCH];
  // K/V tiles are fetched with range-checked buffer loads: the descriptor spans this (entry,
  // head)'s rows [tile start, K), so chunks of rows past K read as zeros with no tail logic, and
  // the per-lane byte offsets stay loop-invariant (self_attn_fused_kernel's staging).
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
  uint8_t cls_next = 0;   // lane j: the class byte of key j of the tile to come
  auto stage_load = [&](int kt) {
    if constexpr (MASKED) {
      // before the K/V loads, so that the ballot's wait leaves those in flight
      if (restrict_keys)
        cls_next = __builtin_amdgcn_raw_buffer_load_b8(make_rsrc(kcls + kt * BK, (int64_t)K - kt * BK), lane, 0, 0);
    }
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
  // retire every prologue load before the loop (self_attn_fused_kernel: the loop header merge
  // would otherwise make the first QK^T of every iteration wait vmcnt(0))
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  // every key admitted: an entry that reads its own keys, no classes, a query past P, or a query
  // whose class entry s does not hold
  const bool admit_all = !restrict_keys || !prow || cls_has[qcls ? 1 : 0] == 0;

  // one K/V tile.  tail: the unmasked kernel's instantiation for a partial last tile (the masked
  // kernel carries the range in its word on every tile)
  auto tile = [&](int kt, auto tail) {
    const int buf = kt & 1;
    uint64_t mw = ~0ull;
    if constexpr (MASKED) {
      const uint64_t word = __ballot(cls_next != 0);
      const int rem = K - kt * BK;
      const uint64_t valid = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
      mw = ((admit_all ? ~0ull : qcls ? word : ~word) & valid) >> (4 * hh);
    }
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
    if constexpr (MASKED) {
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        const uint32_t m32 = (uint32_t)(mw >> (32 * sb));
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!(m32 & (1u << ((r & 3) + 8 * (r >> 2))))) sv[sb][r] = -INFINITY;
      }
    } else if constexpr (decltype(tail)::value) {
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * BK + sb * 32 + acc_row(r, hh) >= K) sv[sb][r] = -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sv[sb][r]);
    mx = fmaxf(mx, other_half(mx)) * c;
    // defer-max: move the reference point only when this tile overshoots it by > thr
    if (__builtin_expect(!__all(mx <= m_run + kRescaleThr), 0)) {
      const float mnew = fmaxf(m_run, mx);
      // (a row still without an admitted key keeps -inf: its factor is 1, not exp2(-inf - -inf))
      const float alpha = mnew == m_run ? 1.f : fast_exp2(m_run - mnew);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] *= alpha;
      l_run *= alpha;
      m_run = mnew;
    }
    const float mref = (MASKED && m_run == -INFINITY) ? 0.f : m_run;
    float ls = 0.f;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = fast_exp2(fmaf(sv[sb][r], c, -mref));
        sv[sb][r] = e;
        if constexpr (!kOnes) ls += e;
      }
    if constexpr (!kOnes) l_run += ls;
    const EV* Vb = Vs + buf * VBUF;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) pv_block<VS, NDT>(MP{}, O, Vb, sb * 32, sv[sb], lane);
    if (kt + 1 < ntiles) stage_write(buf ^ 1);
    __syncthreads();
  };
  if constexpr (MASKED) {
    for (int kt = 0; kt < ntiles; ++kt) tile(kt, std::false_type{});
  } else {
    const int nfull = K / BK;
    for (int kt = 0; kt < nfull; ++kt) tile(kt, std::false_type{});
    if (nfull < ntiles) tile(nfull, std::true_type{});
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
  }
}

// ====================================================================== token classes
// One workgroup per prompt (group g, prompt b): the mean over the lh word-sum maps (plane 0, in
// index order, as build_blend_mask's), min-max normalised over the res^2 pixels, class = (value >=
// threshold); a constant map is class 0 everywhere.  Then the nearest resize to every requested
// side, written to the prompt's cond row and (cfg) its uncond row.
constexpr int kClassThreads = 256;
constexpr int kClassMaxPixels = 1024;

__global__ __launch_bounds__(kClassThreads) void token_classes_kernel(p2p_token_classes_args a) {
  __shared__ float val[kClassMaxPixels];
  __shared__ uint8_t cls[kClassMaxPixels];
  __shared__ float red_mn[kClassThreads / 64], red_mx[kClassThreads / 64];
  const int tid = threadIdx.x;
  const int g = blockIdx.x / a.group_size;
  const int b = blockIdx.x - g * a.group_size;
  const int R2 = a.res * a.res;
  const float* const sums = a.sums[g] + (int64_t)b * 2 * a.lh * R2;   // plane 0 of prompt b
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < R2; i += kClassThreads) {
    float s = 0.f;
    for (int l = 0; l < a.lh; ++l) s += sums[(int64_t)l * R2 + i];
    const float m = s / (float)a.lh;
    val[i] = m;
    mn = fminf(mn, m);
    mx = fmaxf(mx, m);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off));
    mx = fmaxf(mx, __shfl_xor(mx, off));
  }
  if ((tid & 63) == 0) {
    red_mn[tid >> 6] = mn;
    red_mx[tid >> 6] = mx;
  }
  __syncthreads();
  mn = red_mn[0];
  mx = red_mx[0];
#pragma unroll
  for (int w = 1; w < kClassThreads / 64; ++w) {
    mn = fminf(mn, red_mn[w]);
    mx = fmaxf(mx, red_mx[w]);
  }
  const float range = mx - mn;
  for (int i = tid; i < R2; i += kClassThreads)
    cls[i] = (range > 0.f && (val[i] - mn) / range >= a.threshold) ? 1 : 0;
  __syncthreads();
  const int n_prompts = a.n_groups * a.group_size;
  const int row_u = g * a.group_size + b;
  const int row_c = (a.cfg ? n_prompts : 0) + row_u;
  for (int r = 0; r < a.n_res; ++r) {
    const int S = a.side[r];
    uint8_t* const out = a.out[r];
    for (int i = tid; i < S * S; i += kClassThreads) {
      const int y = i / S, x = i - y * S;
      const uint8_t cl = cls[(y * a.res / S) * a.res + x * a.res / S];
      out[(int64_t)row_c * S * S + i] = cl;
      if (a.cfg) out[(int64_t)row_u * S * S + i] = cl;
    }
  }
}

int run_token_classes(const p2p_token_classes_args& a, hipStream_t st) {
  if (a.n_groups < 1 || a.n_groups > P2P_MAX_GROUPS || a.group_size < 1 || a.lh < 1 || a.res < 1) return P2P_E_ARG;
  if ((int64_t)a.res * a.res > kClassMaxPixels) return P2P_E_ARG;
  if ((int64_t)a.n_groups * a.group_size * (a.cfg ? 2 : 1) > P2P_MAX_BATCH) return P2P_E_BATCH;
  if (a.n_res < 1 || a.n_res > 3) return P2P_E_ARG;
  if (!(a.threshold == a.threshold)) return P2P_E_ARG;
  for (int g = 0; g < a.n_groups; ++g) {
    if (!a.sums[g]) return P2P_E_ARG;
    if ((uintptr_t)a.sums[g] & 3) return P2P_E_ALIGN;
  }
  for (int r = 0; r < a.n_res; ++r)
    if (!a.out[r] || a.side[r] < 1 || a.side[r] > 1024) return P2P_E_ARG;
  launch_kernel(token_classes_kernel, dim3(a.n_groups * a.group_size), dim3(kClassThreads), 0, st, a);
  return (int)hipGetLastError();
}

// ====================================================================== launchers
template <typename IO, typename MQ, typename MP, int D, int BK, int W>
static int launch_mutual_t(const MutualArgs& a, bool masked, hipStream_t st) {
  MutualArgs b = a;
  b.n_qtiles = (a.P + 32 * W - 1) / (32 * W);
  dim3 grid(b.n_qtiles * a.H * a.n_active), block(64 * W);
  if (masked) launch_kernel((mutual_attn_kernel<IO, MQ, MP, D, BK, W, true>), grid, block, 0, st, b);
  else launch_kernel((mutual_attn_kernel<IO, MQ, MP, D, BK, W, false>), grid, block, 0, st, b);
  return (int)hipGetLastError();
}

int launch_mutual(const MutualArgs& a, int prec, int d, MutualKernel k, hipStream_t st) {
  return with_precision(prec, [&](auto pr) {
    return with_head_dim(d, [&](auto dd) -> int {
      using IO = typename decltype(pr)::IO;
      using MQ = typename decltype(pr)::MQ;
      using MP = typename decltype(pr)::MP;
      constexpr int D = decltype(dd)::value;
      constexpr int BK = fused_bk(D, MP::kElemBytes == 2);
      const MutualKernelInfo& ki = mutual_info(k);
      if (ki.bk != BK) return P2P_E_ARG;   // a shape of another precision / head dim
      if constexpr (BK == 64 && (D == 40 || D == 80))
        if (ki.waves == 8) return launch_mutual_t<IO, MQ, MP, D, 64, 8>(a, ki.masked, st);
      if (ki.waves == 4) return launch_mutual_t<IO, MQ, MP, D, BK, 4>(a, ki.masked, st);
      return P2P_E_ARG;
    });
  });
}

int run_mutual(const MutualArgs& a, int io_dtype, int compute, int d, hipStream_t st) {
  const int sel = select_mutual(io_dtype, compute, d, a.P, a.token_class != nullptr);
  if (sel < 0) return sel;
  if (a.n_active == 0) return 0;   // every entry skipped: nothing to launch
  return launch_mutual(a, select_precision(io_dtype, compute), d, (MutualKernel)sel, st);
}

}  // namespace p2p
