// self_attn_multi_kernel: d = 40 self-attention, O only, with QB query blocks per wave (gfx950).
// self40_kernel (p2p_self40.hip) has taken over the G1/G7 launches (bf16 / fp16 inputs, K >= 256);
// this kernel serves what that one leaves at P >= 2048: f32 inputs on the bf16 pipe, and bf16
// inputs with K < 256 (p2p_select.h).
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

// ====================================================================== fused self attention, QB rows/wave
// The NOMAX loop of self_attn_fused_kernel (p2p_self.hip) with
// QB 32-row query blocks per wave.  Every K fragment and V fragment read from LDS feeds QB MFMAs
// (half the LDS reads per FLOP at QB = 2), the QB blocks are independent instruction streams in
// the wave, and a tile runs sub-block by sub-block (Q K^T, [max decision], exp, P V) so only one
// 32-key sub-block of scores per block is live; 128-key tiles halve the barriers.  Slow tiles
// (the first one, and the overflow recompute) move the reference point per sub-block with the
// defer-max rule -- the sub-block's P V follows at once, so no P is pending at a rescale.
// Measured at G1 (N = 8, H = 8, bf16; tools/g1_ab.py, profiles/r02): 0.239 ms (64-key tiles with
// the per-tile max, one block per wave) -> 0.233 (NOMAX) -> 0.217 (this, QB = 2, BK = 128).
//
// F16 (bf16 inputs, d = 40): the MFMA itself emits the exponent c*s - m, so a score costs one
// v_exp and half a v_cvt_pk on the VALU instead of v_fma + v_exp + half a cvt:
//   * Q is prescaled by c = scale*log2(e) once, at load, and rounded to f16 (2^-12 relative,
//     8x finer than bf16); K is staged as f16 -- exact, a bf16 value has 8 significant bits --
//     so the QK^T products stay exact in the f32 accumulator;
//   * d = 40 pads to 48 for the MFMA: K column 40 is 1 and Q column 40 holds -m (the row's
//     reference point, an f16 value), so S^T = c s - m comes out of the MFMA;
//   * values outside the f16 range (|k| >= 65520, |c q| >= 65520, |m| >= 65504) set a flag and
//     the workgroup recomputes on the exact bf16 path (K restaged as bf16, fma with c), like the
//     NOMAX overflow recompute.
template <typename IO, typename MQ, int D, int BK, int WAVES, int QB, bool F16 = false, bool PIPE = false>
__global__ __launch_bounds__(64 * WAVES) void self_attn_multi_kernel(SelfArgs a) {
  using EK = typename MQ::elem;
  constexpr int DK = (D + 15) / 16 * 16;
  constexpr int DV = (D + 31) / 32 * 32;
  static_assert(DV > D, "needs the ones column");
  static_assert(!std::is_same<IO, f16_t>::value, "bf16 / f32 inputs only (bf16 V image and P; fp16: p2p_self40.hip)");
  static_assert(!F16 || (DK > D && MQ::planes == 1 && std::is_same<IO, uint16_t>::value),
                "F16: bf16 inputs, a padding column");
  constexpr int NKT = DK / 16;
  constexpr int NDT = DV / 32;
  constexpr int NSB = BK / 32;
  constexpr int KS = KStride<DK, MQ::kElemBytes>::value;
  constexpr int VS = VStrideBf16<DV>::value;
  constexpr int NT = 64 * WAVES;
  constexpr int CPR = D / 8;
  constexpr int NCH = (BK * CPR + NT - 1) / NT;
  constexpr int KPLANE = BK * KS;
  constexpr int KBUF = KPLANE * MQ::planes;
  constexpr int VBUF = BK * VS;
  constexpr int KBYTES = 2 * KBUF * (int)sizeof(EK);
  constexpr int VBYTES = 2 * VBUF * 2;
  constexpr int kLdt = OnesCol<D>::dt, kLh = OnesCol<D>::h, kLr = OnesCol<D>::r;
  // F16: Q column D (the -m slot) = element (D % 16) % 8 of k-step D / 16, lane half (D % 16) / 8
  constexpr int kMt = D / 16;
  constexpr int kMh = (D % 16) / 8;
  constexpr int kMj = D % 8;
  constexpr float kRescaleThr = 8.0f;
  __shared__ __attribute__((aligned(16))) char smem[KBYTES + VBYTES + 16];
  __shared__ int wg_bad;
  EK* const Ks = reinterpret_cast<EK*>(smem);
  uint16_t* const Vs = reinterpret_cast<uint16_t*>(smem + KBYTES);

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
  const int pw = (qt * WAVES + wave) * 32 * QB;   // first query of this wave
  const int K = a.K;
  const float c = a.scale_log2;

  const IO* const qp = static_cast<const IO*>(a.q) + (int64_t)src * a.bsq + h * D;
  const IO* const kp = static_cast<const IO*>(a.k) + (int64_t)src * a.bsk + h * D;
  const IO* const vp = static_cast<const IO*>(a.v) + (int64_t)n * a.bsv + h * D;

  for (int i = tid; i < (KBYTES + VBYTES) / 4; i += NT) reinterpret_cast<float*>(smem)[i] = 0.f;
  if (tid == 0) wg_bad = 0;
  __syncthreads();
  for (int r = tid; r < 2 * BK; r += NT) {
    Vs[r * VS + D] = 0x3F80;
    if constexpr (F16) Ks[r * KS + D] = 0x3C00;   // f16 1.0: the -m column of Q K^T
  }

  // F16 state: the exact bf16 path is taken by the recompute only (ex), after an f16 range miss
  bool ovf = false;
  typename MQ::frag qf[QB][NKT];
  auto load_qf = [&](auto ex) __attribute__((always_inline)) {
#pragma unroll
    for (int b = 0; b < QB; ++b)
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const int col = 16 * t + 8 * hh;
        const int p = pw + 32 * b + qi;
        qf[b][t] = (p < a.P && col < D) ? MQ::load_q(qp + (int64_t)p * a.ldq + col) : MQ::zero();
        if constexpr (F16) if constexpr (!decltype(ex)::value) {
          float mx = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float x = bf2f((uint16_t)qf[b][t].h[j]) * c;
            mx = fmaxf(mx, fabsf(x));
            qf[b][t].h[j] = (short)__builtin_bit_cast(uint16_t, (_Float16)x);
          }
          ovf |= !(mx < 65520.f);
        }
      }
  };
  load_qf(std::false_type{});

  Chunk8<IO> kreg[NCH], vreg[NCH];
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
  auto stage_load = [&](int kt) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t rk =
        make_rsrc(reinterpret_cast<const char*>(kp) + kt * kstep, kbytes - kt * kstep);
    const __amdgpu_buffer_rsrc_t rv =
        make_rsrc(reinterpret_cast<const char*>(vp) + kt * vstep, vbytes - kt * vstep);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if ((BK * CPR) % NT == 0 || tid + i * NT < BK * CPR) {
        kreg[i].load_buf(rk, koff[i]);
        vreg[i].load_buf(rv, voff[i]);
      }
    }
  };
  auto stage_write = [&](int buf, auto ex) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      if ((BK * CPR) % NT == 0 || cidx < BK * CPR) {
        const int row = cidx / CPR;
        const int ch = cidx - row * CPR;
        EK* const kd = Ks + buf * KBUF + row * KS + ch * 8;
        bool staged = false;
        if constexpr (F16) if constexpr (!decltype(ex)::value) {
          staged = true;
          // bf16 -> f16 is exact for magnitudes in [2^-14, 65504] (8 significant bits); below
          // 2^-14 f16 subnormals keep fewer bits (absolute error < 2^-25, flush to 0 under 2^-25),
          // negligible beside the logits.  RTZ packing would clamp past 65504 silently: the range
          // is checked instead
          short8_t hv;
          float mx = 0.f;
#pragma unroll
          for (int j = 0; j < 8; j += 2) {
            const float x0 = bf2f((uint16_t)kreg[i].v[j]), x1 = bf2f((uint16_t)kreg[i].v[j + 1]);
            mx = fmaxf(mx, fmaxf(fabsf(x0), fabsf(x1)));
            const auto pk = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(x0, x1));
            hv[j] = (short)(pk & 0xffff);
            hv[j + 1] = (short)(pk >> 16);
          }
          ovf |= !(mx < 65504.f);
          *reinterpret_cast<short8_t*>(kd) = hv;
        }
        if (!staged) MQ::stage(kreg[i], kd, KPLANE);
        vreg[i].store(Vs + buf * VBUF + row * VS + ch * 8);
      }
    }
  };

  const int ntiles = (K + BK - 1) / BK;
  f32x16_t O[QB][NDT];
  float m_run[QB];
  float m_q[QB];   // F16: the reference point currently held in Q column D (as -m)
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    m_run[b] = -INFINITY;
    m_q[b] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) O[b][dt] = f32x16_t{};
  }
  auto set_mcol = [&](int b, float m) __attribute__((always_inline)) {   // F16: Q column D := -m (lanes of half kMh)
    m_q[b] = m;
    if constexpr (F16)
      if (hh == kMh) qf[b][kMt].h[kMj] = (short)__builtin_bit_cast(uint16_t, (_Float16)(-m));
  };
  auto mma_qk = [&](f32x16_t& acc, const typename MQ::frag& k, const typename MQ::frag& q, auto ex)
      __attribute__((always_inline)) {
    bool done = false;
    if constexpr (F16) if constexpr (!decltype(ex)::value) {
      done = true;
      typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, k.h),
                                                   __builtin_bit_cast(f16x8_t, q.h), acc, 0, 0, 0);
    }
    if (!done) MQ::mma(acc, k, q);
  };

  stage_load(0);
  stage_write(0, std::false_type{});
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  bool bad = false;
  // One tile, sub-block by sub-block (Q K^T, [max decision], exp, P V): only one sub-block's scores
  // per query block are live.  Slow tiles (the first one, and the overflow recompute) move the
  // reference point per 32-key sub-block with the defer-max rule; fast tiles (NOMAX) do not.
  // ex: the exact bf16 path (F16 recompute after a range miss; the only path without F16).
  auto tile = [&](int kt, auto masked, auto fast, auto ex) __attribute__((always_inline)) {
    constexpr bool kF16 = F16 && !decltype(ex)::value;
    const int buf = kt & 1;
    if (kt + 1 < ntiles) stage_load(kt + 1);
    const EK* Kb = Ks + buf * KBUF;
    const uint16_t* Vb = Vs + buf * VBUF;
    auto qk = [&](int sb, f32x16_t (&acc)[QB]) __attribute__((always_inline)) {
#pragma unroll
      for (int b = 0; b < QB; ++b) acc[b] = f32x16_t{};
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const typename MQ::frag fa = MQ::load_k(Kb + (sb * 32 + qi) * KS + 16 * t + 8 * hh, KPLANE);
#pragma unroll
        for (int b = 0; b < QB; ++b) mma_qk(acc[b], fa, qf[b][t], ex);
      }
    };
    // PIPE (fast F16 tiles, where the reference point is fixed for the whole tile): sub-block
    // sb+1's Q K^T is issued before sub-block sb's exponentials, so they can overlap it
    constexpr bool kPipe = PIPE && kF16 && decltype(fast)::value;
    f32x16_t accs[2][QB];
    if constexpr (kPipe) qk(0, accs[0]);
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) {
      f32x16_t acc[QB];
      if constexpr (kPipe) {
#pragma unroll
        for (int b = 0; b < QB; ++b) acc[b] = accs[sb & 1][b];
        if (sb + 1 < NSB) qk(sb + 1, accs[(sb + 1) & 1]);
      } else {
        qk(sb, acc);
      }
      float sv[QB][16];
#pragma unroll
      for (int b = 0; b < QB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sv[b][r] = acc[b][r];
          if constexpr (decltype(masked)::value)
            if (kt * BK + sb * 32 + acc_row(r, hh) >= K) sv[b][r] = -INFINITY;
        }
      if constexpr (!decltype(fast)::value) {
#pragma unroll
        for (int b = 0; b < QB; ++b) {
          float mx = -INFINITY;
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sv[b][r]);
          mx = fmaxf(mx, other_half(mx));
          mx = kF16 ? mx + m_q[b] : mx * c;   // the sub-block's max, log2 units
          if (__builtin_expect(!__all(mx <= m_run[b] + kRescaleThr), 0)) {
            float mnew = fmaxf(m_run[b], mx);
            if constexpr (kF16) {
              mnew = (float)(_Float16)mnew;   // representable in Q's f16 column
              ovf |= !(fabsf(mnew) < 65504.f);
            }
            const float alpha = fast_exp2(m_run[b] - mnew);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
              for (int r = 0; r < 16; ++r) O[b][dt][r] *= alpha;
            m_run[b] = mnew;
          }
        }
      }
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        if constexpr (kF16) {
          if constexpr (decltype(fast)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sv[b][r] = fast_exp2(sv[b][r]);
          } else {
            const float dm = m_run[b] - m_q[b];
#pragma unroll
            for (int r = 0; r < 16; ++r) sv[b][r] = fast_exp2(sv[b][r] - dm);
            set_mcol(b, m_run[b]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) sv[b][r] = fast_exp2(fmaf(sv[b][r], c, -m_run[b]));
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        MmaBf16::frag pb[QB];
#pragma unroll
        for (int b = 0; b < QB; ++b) pb[b] = MmaBf16::pack_p(sv[b] + 8 * s2);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const MmaBf16::frag af = vt_frag<VS>(Vb, sb * 32, s2, dt * 32, lane);
#pragma unroll
          for (int b = 0; b < QB; ++b) MmaBf16::mma(O[b][dt], af, pb[b]);
        }
      }
    }
    if constexpr (decltype(fast)::value) {
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        const float own = O[b][kLdt][kLr];
        const float lsum = own + other_half(own);
        bad |= !(lsum < INFINITY);
        if (__builtin_expect(__any(lsum > 0x1p64f), 0)) {
          if (lsum > 0x1p64f) {
            // the new reference is rounded first (F16: it must be exact in Q's f16 column) and
            // O rescaled by the exact factor between the two, so old and new tiles stay consistent
            const float mnew = kF16 ? (float)(_Float16)(m_run[b] + 64.f) : m_run[b] + 64.f;
            const float f = fast_exp2(m_run[b] - mnew);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
              for (int r = 0; r < 16; ++r) O[b][dt][r] *= f;
            m_run[b] = mnew;
            if constexpr (kF16) {
              ovf |= !(fabsf(mnew) < 65504.f);
              set_mcol(b, mnew);
            }
          }
        }
      }
    }
    if (kt + 1 < ntiles) stage_write(buf ^ 1, ex);
    __syncthreads();
  };
  const int nfull = K / BK;
  constexpr std::false_type kNo{};
  constexpr std::true_type kYes{};
  if (nfull == 0) tile(0, kYes, kNo, kNo);
  else tile(0, kNo, kNo, kNo);
  for (int kt = 1; kt < nfull; ++kt) tile(kt, kNo, kYes, kNo);
  if (nfull < ntiles && nfull > 0) tile(nfull, kYes, kYes, kNo);
  {
    const bool any_bad = __any(bad), any_ovf = __any(ovf);
    if (lane == 0 && (any_bad || any_ovf)) atomicOr(&wg_bad, any_ovf ? 2 : 1);
  }
  __syncthreads();
  if (__builtin_expect(wg_bad != 0, 0)) {
#pragma unroll
    for (int b = 0; b < QB; ++b) {
      m_run[b] = -INFINITY;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) O[b][dt] = f32x16_t{};
    }
    auto redo = [&](auto ex) __attribute__((always_inline)) {
      if constexpr (decltype(ex)::value) {
        load_qf(ex);   // unscaled bf16 Q, column D zero
      } else if constexpr (F16) {
#pragma unroll
        for (int b = 0; b < QB; ++b) set_mcol(b, 0.f);
      }
      stage_load(0);
      stage_write(0, ex);
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
      for (int kt = 0; kt < nfull; ++kt) tile(kt, kNo, kNo, ex);
      if (nfull < ntiles) tile(nfull, kYes, kNo, ex);
    };
    // F16: every recompute (a range miss or a non-finite row sum) takes the exact bf16 path; a
    // row-sum recompute on the F16 slow path could meet |m| >= 65504 on a later tile with nothing
    // left to catch it
    if constexpr (F16) redo(kYes);
    else redo(kNo);
  }
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    const float l = __shfl(O[b][kLdt][kLr], (lane & 31) + 32 * kLh);
    const float inv = 1.f / l;
    const int p = pw + 32 * b + qi;
    if (p < a.P) {
      IO* const op = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D + (int64_t)p * a.ldo;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = dt * 32 + 8 * g + 4 * hh;
          if (dd < D)
            store4(op + dd, O[b][dt][4 * g] * inv, O[b][dt][4 * g + 1] * inv, O[b][dt][4 * g + 2] * inv,
                   O[b][dt][4 * g + 3] * inv);
        }
    }
  }
}

template <typename IO, typename MQ, int D, int BK, int W, int QB, bool F16 = false, bool PIPE = false>
static int launch_multi(const SelfArgs& a, hipStream_t st) {
  SelfArgs b = a;
  b.n_qtiles = (a.P + 32 * W * QB - 1) / (32 * W * QB);
  dim3 grid(b.n_qtiles * a.H * a.N), block(64 * W);
  launch_kernel((self_attn_multi_kernel<IO, MQ, D, BK, W, QB, F16, PIPE>), grid, block, 0, st, b);
  return (int)hipGetLastError();
}

int launch_self_multi(const SelfArgs& a, SelfKernel k, hipStream_t st) {
  switch (k) {
    case SELF_MULTI_F16_256: return launch_multi<uint16_t, QkBf16<uint16_t>, 40, 256, 8, 2, true, true>(a, st);
    case SELF_MULTI_128: return launch_multi<float, QkSplit, 40, 128, 8, 2>(a, st);
    default: return P2P_E_ARG;
  }
}

}  // namespace p2p
