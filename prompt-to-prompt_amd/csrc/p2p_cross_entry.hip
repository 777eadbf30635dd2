// cross_attn_kernel: per-entry cross-attention over the 77 text tokens for MI355X (gfx950), every
// precision and head dim, with the P2P cross edit (AttentionControlEdit.forward, main.py:180-197)
// applied in registers between the exact softmax and PV, the AttentionStore epilogue and
// LocalBlend's word sums.  The group-coupled kernel of p2p_cross.hip takes the G1/G7 launches
// (p2p_select.h); this one takes every other.
//
// The kernel follows the transposed-fragment convention of p2p_device.h: S^T = K Q^T and
// O^T = V^T P^T, query on the lane.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

// ====================================================================== cross attention
// One workgroup = one head x one tile of 32*WAVES queries x one batch entry n.  An edit entry
// (position b > 0 of a prompt group that carries an edit program) first recomputes the
// source prompt's probabilities P0 for the same rows (the K = 77 cross product is cheap) and
// parks them in LDS, one 32-row slab per wave, so the edit can gather from them:
//   R[w]  = post[w] * ( c_rep[w] * P_b[w] + sum_{t < tmax} val[t][w] * P0[row[t][w]] )
//   P_b'  = alpha[w] * R[w] + (1 - alpha[w]) * P_b[w]
// which is AttentionReplace (c_rep 0, mapper column w), AttentionRefine (c_rep 1-a, one term
// mapper[w] with weight a), AttentionReweight (c_rep 0, term (w, eq[w])), and Reweight
// chained on either (post = eq) -- host side: p2p_amd/programs.py.  The term planes make the
// gather a wave-uniform loop whose loads are independent across the lane's 48 columns.
// Stored maps leave through the same slab as whole contiguous rows (one [32, K] block per
// wave).  The slab is dynamic LDS, allocated only by launches with an edit or a store, so a
// plain launch runs at the occupancy of its K/V tiles alone.
#ifdef P2P_EXPERIMENTS
// diagnostic clock stamps of the cross kernel (experiments build, VARIANT_CROSS_STAMPS):
// [logical workgroup < 4096][wave < 4][slot < 24]; read back by p2p_diag_cross_stamps
__device__ unsigned long long g_cross_stamps[4096 * 4 * 24];
#define P2P_CROSS_STAMP(i)                                                                              \
  if (a.variant == VARIANT_CROSS_STAMPS && logical < 4096 && wave < 4 && lane == 0)                     \
    g_cross_stamps[(logical * 4 + wave) * 24 + (i)] = __builtin_amdgcn_s_memtime();
#else
#define P2P_CROSS_STAMP(i) do { } while (0);
#endif

template <typename IO, typename MQ, typename MP, int D, int WAVES, bool DENSE>
__global__ __launch_bounds__(64 * WAVES, (DENSE && D <= 80) ? 2 : 1) void cross_attn_kernel(CrossArgs a) {
  using EK = typename MQ::elem;
  using EV = typename MP::elem;
  constexpr int DK = (D + 15) / 16 * 16;
  constexpr int DV = (D + 31) / 32 * 32;
  constexpr int NKT = DK / 16;
  constexpr int NDT = DV / 32;
  constexpr int KB = P2P_MAX_KEYS_CROSS / 32;
  constexpr int KR = KB * 32;
  constexpr int KS = KStride<DK, MQ::kElemBytes>::value;
  constexpr int VS = (MP::kElemBytes == 2) ? VStrideBf16<DV>::value : DV;
  constexpr int NT = 64 * WAVES;
  constexpr int CPR = D / 8;
  constexpr int NCH = (KR * CPR + NT - 1) / NT;
  constexpr int KPLANE = KR * KS;
  constexpr int KBYTES = KPLANE * MQ::planes * (int)sizeof(EK);
  constexpr int VBYTES = KR * VS * (int)sizeof(EV);
  __shared__ __attribute__((aligned(16))) char smem[KBYTES + VBYTES];
  extern __shared__ __attribute__((aligned(16))) char cross_dyn[];  // slab: WAVES * 32 * P0S f32
  EK* const Ks = reinterpret_cast<EK*>(smem);
  EV* const Vs = reinterpret_cast<EV*>(smem + KBYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int hh = lane >> 5;
  const int qi = lane & 31;

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  P2P_CROSS_STAMP(0)
  // Kernel arguments live in memory: every a.field is a scalar load, and a chain of dependent
  // ones costs a round trip each at the start of every workgroup.  Everything the lean path reads
  // that does not depend on the entry is pinned here, so it all arrives in ONE round trip; the
  // entry's packed info is the one dependent load after it.
  asm volatile("" ::"s"(a.n_qtiles), "s"(a.H), "s"(a.N), "s"(a.P), "s"(a.K), "s"(a.q), "s"(a.k), "s"(a.v),
               "s"(a.o), "s"(a.ldq), "s"(a.ldk), "s"(a.ldv), "s"(a.ldo), "s"(a.bsq), "s"(a.bsk), "s"(a.bsv),
               "s"(a.bso), "s"(a.scale_log2));
  // Entries fastest (rotated, below), then heads -- xcd_remap keeps consecutive ids on one XCD, so the source's Q
  // rows that a tile's three edit workgroups re-read (for P0) and the tile's q / o lines stay in
  // that XCD's L2 (in the pipeline, rocprof: G2/G6 21.4 -> 20.1 us, d = 160 21.7 -> 20.9 us;
  // profiles/r04/cross_order_r04p/)
  // (every launch size: with eight groups per call, N = 64, entries fastest also took G2/G6 134 ->
  // 115 us and d = 160 84 -> 72 us against heads fastest, profiles/r04/cross_order_large_r04am/)
  // The second 32 of every 64 ids rotate the entries by N/2, so the two workgroups a CU holds
  // (ids i and i + 32 of an XCD's chunk, as the group kernel's order measured) pair an edit or
  // source entry with an uncond one instead of two edits: G2/G6 19.8 -> 18.5 us in the pipeline
  // (profiles/r04/cross_pairing_r04ae/).  The rotation is constant over each run of N ids only
  // when N divides 32 -- otherwise (N = 64: eight groups per call) two runs would map onto the
  // same entries -- so only then
  const int rot = (32 % a.N == 0) ? ((logical >> 5) & 1) * (a.N >> 1) : 0;
  const int rest = (logical % a.N + rot) % a.N;
  const int h = (logical / a.N) % a.H;
  const int qt = logical / a.N / a.H;
  const int n = a.N - 1 - rest;  // the edits sit last in the batch: dispatch them first
  // one dependent kernel-argument load decides the path (every a.field read is a scalar memory
  // round trip; chains of them cost ~1 us at the start of every workgroup)
  const int info = a.ent_info[n];
  asm volatile("" ::"s"(info));
  const int gi = info & 0xff;
  const int b = (info >> 8) & 0xff;
  const int first = n - b;
  const bool edit = (info >> 16) & 1;
  const bool stored = (info >> 17) & 1;
  // p2p_group.flags P2P_GROUP_F_R_ONLY (dense edits): this call's alpha makes every blend
  // coefficient A = alpha post c_rep + 1 - alpha zero (a Replace / Reweight step inside
  // cross_replace_steps, main.py:189), so P' = R B: the entry's own Q K^T softmax is not needed and
  // neither are its Q and K -- only its V (checked again from the coefficients below)
  const bool r_only = (info >> 18) & 1;
  // wave-uniform in a scalar register: the buffer resources built from it (Q rows, the running-sum
  // rows) stay scalar -- from a VGPR every such load became a readfirstlane waterfall loop
  const int p0w = __builtin_amdgcn_readfirstlane(qt * 32 * WAVES + wave * 32);
  const int p = p0w + qi;
  const bool prow = p < a.P;
  const int K = a.K;
  const float c = a.scale_log2;
  const int P0S = a.slab_stride;
  float* const slab = reinterpret_cast<float*>(cross_dyn) + wave * 32 * P0S;
  // O out.  The accumulator puts the query on the lane, so a direct store writes 32 rows x 8 bytes
  // per instruction.  bf16 outputs with 16-byte rows instead go through LDS (the self kernels'
  // epilogue): after a workgroup barrier (every wave is done with K / V) each wave writes its 32
  // rows into the dead K / V image and stores them back as whole 16-byte row chunks, consecutive
  // lanes along a row -- half the store instructions, whole lines.
  // Same-box rocprof (profiles/r05/ostore_ab/): d = 80 edit steps 16.43 -> 14.90 us, d = 160 17.44 ->
  // 16.56; the 8x8 layers (P = 64: half of every 128-query workgroup's rows past P) ran 2 % slower
  // and keep the direct store
  const bool o16 = is_io16<IO>::value && a.P >= 256 && (a.ldo & 7) == 0 &&
                   (a.bso & 7) == 0 && ((uintptr_t)a.o & 15) == 0;
  auto store_o = [&](const f32x16_t (&O)[NDT], float inv) __attribute__((always_inline)) {
    if constexpr (is_io16<IO>::value) {
      if (o16) {
        constexpr int OS = D + 8;   // 16-byte aligned rows on distinct banks
        static_assert(WAVES * 32 * OS * 2 <= KBYTES + VBYTES, "the output rows fit the K / V image");
        __syncthreads();
        IO* const orow = reinterpret_cast<IO*>(smem) + wave * 32 * OS;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int dd = dt * 32 + 8 * g + 4 * hh;
            if (dd < D)
              store4(orow + qi * OS + dd, O[dt][4 * g] * inv, O[dt][4 * g + 1] * inv, O[dt][4 * g + 2] * inv,
                     O[dt][4 * g + 3] * inv);
          }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        IO* const ob = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D;
#pragma unroll
        for (int c0 = 0; c0 < 32 * CPR; c0 += 64) {
          const int cidx = c0 + lane;
          const int row = cidx / CPR, ch = cidx - row * CPR;
          if (((32 * CPR) % 64 == 0 || cidx < 32 * CPR) && p0w + row < a.P)
            *reinterpret_cast<short8_t*>(ob + (int64_t)(p0w + row) * a.ldo + ch * 8) =
                *reinterpret_cast<const short8_t*>(orow + row * OS + ch * 8);
        }
        return;
      }
    }
    if (prow) {
      IO* const op = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D + (int64_t)p * a.ldo;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int dd = dt * 32 + 8 * g + 4 * hh;
          if (dd < D)
            store4(op + dd, O[dt][4 * g] * inv, O[dt][4 * g + 1] * inv, O[dt][4 * g + 2] * inv, O[dt][4 * g + 3] * inv);
        }
    }
  };

  // ---- plain entries (no edit program, maps not kept): the lean path.  Every global load is
  // issued first (Q fragments, this thread's K and V chunks) and the padding is written while they
  // fly; V's column D is 1, so the P V MFMA's row D is the row sum of the bf16 weights it used
  // (no per-element sum, no normalised P: O is scaled once); only a key block that runs past K
  // is masked.  (Measured at G1, N = 8, H = 8: tools/cross_bench.py, profiles/r02.)
  if constexpr (MP::kElemBytes == 2 && DV > D) {
    if (!edit && !stored) {
      constexpr int kLdt = OnesCol<D>::dt, kLh = OnesCol<D>::h, kLr = OnesCol<D>::r;
      typename MQ::frag qf[NKT];
      {
        const IO* qp = static_cast<const IO*>(a.q) + (int64_t)n * a.bsq + h * D + (int64_t)p * a.ldq;
#pragma unroll
        for (int t = 0; t < NKT; ++t) {
          const int col = 16 * t + 8 * hh;
          qf[t] = (prow && col < D) ? MQ::load_q(qp + col) : MQ::zero();
        }
      }
      const IO* kp = static_cast<const IO*>(a.k) + (int64_t)n * a.bsk + h * D;
      const IO* vp = static_cast<const IO*>(a.v) + (int64_t)n * a.bsv + h * D;
      Chunk8<IO> kc[NCH], vc[NCH];
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int cidx = tid + i * NT;
        const int row = cidx / CPR;
        const int ch = cidx - row * CPR;
        if (cidx < K * CPR) {
          kc[i].load(kp + (int64_t)row * a.ldk + ch * 8);
          vc[i].load(vp + (int64_t)row * a.ldv + ch * 8);
        }
      }
      P2P_CROSS_STAMP(1)
      if constexpr (DK > D) {   // K columns D..DK of every row: Q's zero columns meet zeros, not stale LDS
        constexpr int PC = (DK - D) / 8;
        for (int i = tid; i < KR * PC * MQ::planes; i += NT) {
          const int pl = i / (KR * PC);
          const int j = i - pl * KR * PC;
          *reinterpret_cast<short8_t*>(Ks + pl * KPLANE + (j / PC) * KS + D + 8 * (j % PC)) = short8_t{};
        }
      }
      for (int i = tid; i < (KR - K) * VS / 8; i += NT)   // V rows K..KR (weighted by p = 0)
        *reinterpret_cast<short8_t*>(Vs + K * VS + 8 * i) = short8_t{};
      for (int r = tid; r < K; r += NT) Vs[r * VS + D] = one_elem<EV>();   // 1.0: the row-sum column
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int cidx = tid + i * NT;
        const int row = cidx / CPR;
        const int ch = cidx - row * CPR;
        if (cidx < K * CPR) {
          MQ::stage(kc[i], Ks + row * KS + ch * 8, KPLANE);
          vc[i].store(Vs + row * VS + ch * 8);
        }
      }
      __syncthreads();
      P2P_CROSS_STAMP(2)
      float sv[KB][16];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        f32x16_t acc = {};
#pragma unroll
        for (int t = 0; t < NKT; ++t) {
          const typename MQ::frag fa = MQ::load_k(Ks + (kb * 32 + qi) * KS + 16 * t + 8 * hh, KPLANE);
          MQ::mma(acc, fa, qf[t]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sv[kb][r] = acc[r];
        if (kb * 32 + 32 > K) {   // wave-uniform: only the block that runs past K
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kb * 32 + acc_row(r, hh) >= K) sv[kb][r] = -INFINITY;
        }
      }
      // K <= (KB-1)*32 + 16 (the 77 text tokens): registers 8..15 of the last block are all masked
      auto soft = [&](auto tail) {
        constexpr bool kShort = decltype(tail)::value;
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (!(kShort && kb == KB - 1 && r >= 8)) mx = fmaxf(mx, sv[kb][r]);
        mx = fmaxf(mx, other_half(mx)) * c;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            sv[kb][r] = (kShort && kb == KB - 1 && r >= 8) ? 0.f : fast_exp2(fmaf(sv[kb][r], c, -mx));
      };
      if (K <= (KB - 1) * 32 + 16) soft(std::true_type{});
      else soft(std::false_type{});
      P2P_CROSS_STAMP(3)
      f32x16_t O[NDT];
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) pv_block<VS, NDT>(MP{}, O, Vs, kb * 32, sv[kb], lane);
      P2P_CROSS_STAMP(4)
      const float inv = 1.f / __shfl(O[kLdt][kLr], (lane & 31) + 32 * kLh);
      store_o(O, inv);
      P2P_CROSS_STAMP(5)
      return;
    }
  }

  const char* const prog = static_cast<const char*>(a.grp_prog[gi]);
  const int slot = a.store_slot[n];
  // maps kept and accumulated: touch this wave's rows of the running sum now (32 x K f32,
  // contiguous), so the read-add-write of the store epilogue finds them in this XCD's L2 instead of
  // paying an HBM round trip at the end of the workgroup
  // (two loads per lane cover 32 rows of up to 96 keys; their values are only consumed at the very
  // end, so nothing waits for them)
  float touch0 = 0.f, touch1 = 0.f;
  // LocalBlend word weights of this entry (lanes 0-31: alpha, 32-63: substruct) for LDS: loaded now
  // (unconditionally, from valid addresses: a load inside a branch gets its own wait), written to
  // LDS once the prologue's loads are in flight; the store epilogue's per-row word sums then read
  // them from LDS, not global memory
  __shared__ __attribute__((aligned(16))) float btab[2][P2P_MAX_KEYS_CROSS];
  const bool blend_on = stored && a.grp_bsum[gi] != nullptr;
  float bw0 = 0.f, bw1 = 0.f;
  if (blend_on) {
    const float* const ta = a.grp_balpha[gi] + (int64_t)b * K;
    const float* const tsub = a.grp_bsub[gi];
    static_assert(2 * P2P_MAX_KEYS_CROSS <= 2 * NT, "two weights per thread");
    const int i1 = tid + NT;
    const float* s0 = tid < K ? ta + tid : (tid < 2 * K && tsub != nullptr) ? tsub + (int64_t)b * K + tid - K : ta;
    const float* s1 = i1 < K ? ta + i1 : (i1 < 2 * K && tsub != nullptr) ? tsub + (int64_t)b * K + i1 - K : ta;
    bw0 = *s0;
    bw1 = *s1;
    if (!(tid < K || (tid < 2 * K && tsub != nullptr))) bw0 = 0.f;
    if (!(i1 < K || (i1 < 2 * K && tsub != nullptr))) bw1 = 0.f;
  }
  // once the prologue's loads are issued: the blend weights into LDS; this wave's rows of the
  // running sum are touched into this XCD's L2 (32 x K f32, contiguous; two loads per lane cover 32
  // rows of up to 96 keys) so the store epilogue's read-add-write finds them there.  The touches
  // go after every other load: they miss to HBM, and a wait for any load issued after them would
  // wait for them too
  // The touches are issued after the workgroup's first barrier, not with the prologue: the whole
  // launch issues its prologue loads at once, and 10 MB of touches (G2/G6) in that burst delayed
  // every workgroup's first round trip (in the pipeline, rocprof: G2/G6 20.0 -> 19.1 us, d = 160
  // 20.7 -> 20.4; no touches at all: 19.8 / 20.6; profiles/r04/cross_touch_r04r/).  Experiments:
  // Mode 3 goes further: after the first barrier the wave reads its rows of the running sum (and
  // its LocalBlend word-sum entries) into registers, so the store epilogue only adds and writes.
  // (bf16 inputs only: the f32-input instantiations have no registers to spare for the rows)
  // 1: touches after the first barrier, 3: the values themselves
  constexpr int touch_when = is_io16<IO>::value ? 3 : 1;
  constexpr int kRmwF4 = 32 * KR / 4;
  f32x4_t rmwbuf[(kRmwF4 + 63) / 64];
  float bsum_old = 0.f;
  const int srows = min(32, a.P - p0w);
  float* const sg = stored ? a.store + ((int64_t)(slot + h) * a.P + p0w) * (int64_t)K : nullptr;
  const bool rmw_vec = stored && srows > 0 && ((uintptr_t)sg & 15) == 0 && ((srows * K) & 3) == 0;
  float* const bdst = blend_on ? a.grp_bsum[gi] + ((int64_t)(b * 2 + hh) * a.grp_blh[gi] + a.grp_bcol[gi] + h) * a.P +
                                     p0w + qi
                               : nullptr;
  auto touch = [&]() __attribute__((always_inline)) {
    if (touch_when == 3) {
      // issued unconditionally (zero-size buffer resources when nothing is kept: no traffic), so
      // every path issues the same number of loads here -- a branch-skipped load makes hipcc's waits
      // for the prologue's loads count on the path without it (the dense prologue below)
      const bool acc = stored && a.store_accumulate;
      rmw_load<kRmwF4>(sg, (acc && rmw_vec) ? srows * K : 0, lane, rmwbuf);
      // the lane's LocalBlend word-sum entry: (b * 2 + hh)'s plane, query p0w + qi (lanes past the
      // rows read a neighbour or zero, and keep 0)
      const bool bl = acc && blend_on;
      const float* const bb = bl ? a.grp_bsum[gi] + ((int64_t)(b * 2) * a.grp_blh[gi] + a.grp_bcol[gi] + h) * a.P + p0w : nullptr;
      const __amdgpu_buffer_rsrc_t rb = make_rsrc(bb, bl ? ((int64_t)a.grp_blh[gi] * a.P + srows) * 4 : 0);
      const float v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, (hh * a.grp_blh[gi] * a.P + qi) * 4, 0, 0));
      bsum_old = qi < srows ? v : 0.f;
    } else if (stored && a.store_accumulate) {
      const int rows = min(32, a.P - p0w);
      const float* g = a.store + ((int64_t)(slot + h) * a.P + p0w) * (int64_t)K;
      const int lines = (rows * K * 4 + 127) / 128;
      static_assert(32 * P2P_MAX_KEYS_CROSS * 4 / 128 <= 128, "two touches per lane");
      if (lane < lines) touch0 = g[lane * 32];
      if (lane + 64 < lines) touch1 = g[(lane + 64) * 32];
    }
  };
  auto finish_prologue = [&]() __attribute__((always_inline)) {
    if (blend_on) {
      const int i1 = tid + NT;
      if (tid < 2 * K) btab[tid < K ? 0 : 1][tid < K ? tid : tid - K] = bw0;
      if (i1 < 2 * K) btab[i1 < K ? 0 : 1][i1 < K ? i1 : i1 - K] = bw1;
      // columns K.. of both tables are zero (the 16-byte weight reads of the register sums)
      static_assert(P2P_MAX_KEYS_CROSS <= NT, "one padding column per thread");
      if (tid < P2P_MAX_KEYS_CROSS - K) btab[0][K + tid] = btab[1][K + tid] = 0.f;
    }
    // (never true; kept because the generated code of every instantiation changes without it)
    if (touch_when == 0) touch();
  };

  // padding the MFMAs read but the staging never writes (disjoint from it: no extra barrier):
  // K columns D..DK (multiplied by Q's zero columns) and V rows K..KR (weighted by p = 0)
  if constexpr (DK > D) {
    for (int i = tid; i < MQ::planes * KR * (DK - D); i += NT) {
      const int pl = i / (KR * (DK - D));
      const int j = i - pl * KR * (DK - D);
      const int row = j / (DK - D);
      Ks[pl * KPLANE + row * KS + D + (j - row * (DK - D))] = EK(0);
    }
  }
  for (int i = tid; i < (KR - K) * VS; i += NT) Vs[K * VS + i] = EV(0);

  // bf16 inputs: Q rows and K / V chunks by range-checked buffer loads issued unconditionally
  // (rows >= P / >= K read as zeros).  Loads inside a branch per fragment or chunk made hipcc
  // re-load kernel arguments and drain the earlier loads with vmcnt(0) between them: the stored
  // source / plain entries' staging ran as a chain of round trips
  constexpr bool kBufIO = (std::is_same<IO, uint16_t>::value && std::is_same<MQ, QkBf16<uint16_t>>::value) ||
                          (std::is_same<IO, f16_t>::value && std::is_same<MQ, QkF16>::value);
  auto load_q = [&](int e, typename MQ::frag (&qf)[NKT]) {
    const IO* qp = static_cast<const IO*>(a.q) + (int64_t)e * a.bsq + h * D;
    if constexpr (kBufIO) {
      const __amdgpu_buffer_rsrc_t rq = make_rsrc(qp + (int64_t)p0w * a.ldq, ((int64_t)(a.P - 1 - p0w) * a.ldq + D) * 2);
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const int col = 16 * t + 8 * hh;
        qf[t].h = __builtin_bit_cast(short8_t, __builtin_amdgcn_raw_buffer_load_b128(rq, (qi * (int)a.ldq + col) * 2, 0, 0));
        if (col >= D) qf[t] = MQ::zero();
      }
    } else {
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const int col = 16 * t + 8 * hh;
        qf[t] = (prow && col < D) ? MQ::load_q(qp + (int64_t)p * a.ldq + col) : MQ::zero();
      }
    }
  };

  // K (and V) of entry e: global -> registers (load_kv), registers -> LDS (store_kv); withK = false:
  // V only (an R_ONLY edit)
  auto load_kv = [&](int e, Chunk8<IO> (&kc)[NCH], Chunk8<IO> (&vc)[NCH], bool withV, bool withK = true) {
    const IO* kp = static_cast<const IO*>(a.k) + (int64_t)e * a.bsk + h * D;
    const IO* vp = static_cast<const IO*>(a.v) + (int64_t)e * a.bsv + h * D;
    if constexpr (kBufIO) {
      const __amdgpu_buffer_rsrc_t rk = make_rsrc(kp, ((int64_t)(K - 1) * a.ldk + D) * 2);
      const __amdgpu_buffer_rsrc_t rv = make_rsrc(vp, ((int64_t)(K - 1) * a.ldv + D) * 2);
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int cidx = tid + i * NT;
        const int row = cidx / CPR;
        const int ch = cidx - row * CPR;
        if (withK) kc[i].load_buf(rk, (uint32_t)((row * (int)a.ldk + ch * 8) * 2));
        if (withV) vc[i].load_buf(rv, (uint32_t)((row * (int)a.ldv + ch * 8) * 2));
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      const int row = cidx / CPR;
      const int ch = cidx - row * CPR;
      if (cidx < K * CPR) {
        if (withK) kc[i].load(kp + (int64_t)row * a.ldk + ch * 8);
        if (withV) vc[i].load(vp + (int64_t)row * a.ldv + ch * 8);
      }
    }
  };
  auto store_kv = [&](const Chunk8<IO> (&kc)[NCH], const Chunk8<IO> (&vc)[NCH], bool withV, bool withK = true) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      const int row = cidx / CPR;
      const int ch = cidx - row * CPR;
      if (cidx < K * CPR) {   // (V rows K..KR are zeroed with the padding; K rows past K are masked)
        if (withK) MQ::stage(kc[i], Ks + row * KS + ch * 8, KPLANE);
        if (withV) vc[i].store(Vs + row * VS + ch * 8);
      }
    }
  };
  // exact softmax of S^T = K_e Q_e^T over the K keys for this lane's query row (K rows past
  // K hold stale LDS: their accumulator rows are replaced by -inf, never used)
  // kShort (K <= (KB-1)*32 + 16, e.g. the 77 text tokens): registers 8..15 of the last key block
  // hold keys >= 80, all masked -- their exponentials, sums and scalings are skipped
  const bool short_tail = K <= (KB - 1) * 32 + 16;
  auto probs_t = [&](const typename MQ::frag (&qf)[NKT], float (&sv)[KB][16], auto tail) {
    constexpr bool kShort = decltype(tail)::value;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      f32x16_t acc = {};
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const typename MQ::frag fa = MQ::load_k(Ks + (kb * 32 + qi) * KS + 16 * t + 8 * hh, KPLANE);
        MQ::mma(acc, fa, qf[t]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sv[kb][r] = acc[r];
      if (kb * 32 + 32 > K) {   // wave-uniform: only the block that runs past K is masked
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kb * 32 + acc_row(r, hh) >= K) sv[kb][r] = -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (!(kShort && kb == KB - 1 && r >= 8)) mx = fmaxf(mx, sv[kb][r]);
    mx = fmaxf(mx, other_half(mx)) * c;
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (kShort && kb == KB - 1 && r >= 8) {
          sv[kb][r] = 0.f;
        } else {
          const float ex = fast_exp2(fmaf(sv[kb][r], c, -mx));
          sv[kb][r] = ex;
          ls += ex;
        }
      }
    const float inv = 1.f / (ls + other_half(ls));
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (!(kShort && kb == KB - 1 && r >= 8)) sv[kb][r] *= inv;
  };
  auto probs = [&](const typename MQ::frag (&qf)[NKT], float (&sv)[KB][16]) {
    if (short_tail) probs_t(qf, sv, std::true_type{});
    else probs_t(qf, sv, std::false_type{});
  };

  typename MQ::frag qf[NKT];
  float sv[KB][16];
  // dense edit (bf16 PV path, program carries the f16 mapper tile): R = P0 . M_e on the MFMA
  constexpr bool kDenseOk = DENSE && MP::kElemBytes == 2;  // separate instantiation: its VGPRs
  // the dense edit's per-column blend coefficients A | B: static LDS, so the store epilogue's
  // per-wave slab (which overlays the dead mapper tile) never overlaps them
  __shared__ __attribute__((aligned(16))) float dcol[kDenseOk ? 2 * KR : 4];
  const bool dense = kDenseOk && edit;   // the launcher picks DENSE only if every edit group is
  f32x16_t Rd[KB];
  int dense_flags = 3;   // dense edits: the blend halves in use (set from the coefficients)
  // dense edits: this entry's own K / V are loaded together with the source's prologue loads, so
  // the workgroup waits one memory round trip instead of two (measured against staging them
  // after the R phase: profiles/r03/cross_store/cross_bench_own_kv_*.log)
  Chunk8<IO> kc1[kDenseOk ? NCH : 1], vc1[kDenseOk ? NCH : 1];
  typename MQ::frag qf1[kDenseOk ? NKT : 1];   // (and its own Q rows)
  bool own_early = false;
  if constexpr (kDenseOk) {
   if (dense) {
    const uint16_t* mg = static_cast<const uint16_t*>(a.grp_dense[gi]) +
                         (int64_t)(b - 1) * P2P_PROGRAM_DENSE * P2P_PROGRAM_DENSE;
    EV* const Ms = reinterpret_cast<EV*>(cross_dyn);  // [96 source words][96 target words]
    // every global load of the prologue is issued at once (one memory round trip), in the order
    // of use: the coefficients and the source's K and Q (P0), then the mapper tile (R) and this
    // entry's own rows.  Each is waited for only where it is used, so the in-order counter lets
    // P0 start once the source's bytes have landed while the tile and the own V land behind it:
    // the launch-wide prologue burst, not the latency, sets the first round trip.
    // d = 160 only: at d <= 80 (two workgroups per CU, 256 VGPRs) the tile and the own V held in
    // registers across P0 spill 56 VGPRs
    constexpr bool late = D > 80;
    constexpr int kMCh = P2P_PROGRAM_DENSE * P2P_PROGRAM_DENSE / 8;   // 16-byte chunks of the tile
    constexpr int kMPer = (kMCh + NT - 1) / NT;
    const float* ce = reinterpret_cast<const float*>(prog + P2P_PROGRAM_HEADER_BYTES +
                                                     (int64_t)(b - 1) * P2P_PROGRAM_REC_BYTES);
    const float* al = a.grp_alpha[gi] + (b - 1) * K;
    static_assert(KR <= NT, "one column per thread");
    const int w = tid;
    float aw = 0.f, cw = 0.f, pw = 0.f;
    if (w < K) {
      aw = al[w];
      cw = ce[w];
      pw = ce[P2P_PROGRAM_COLS + w];
    }
    Chunk8<IO> kc0[NCH], vc0[NCH];
    load_kv(first, kc0, vc0, false);
    load_q(first, qf);
    // (the scheduler would otherwise issue the Q loads last, and every wait for Q would then wait
    // for the tile and the own rows as well)
    __builtin_amdgcn_sched_barrier(0);
    // the tile by range-checked buffer loads (chunks past it read as zeros), the own V on both
    // paths, and only then the path-dependent own K and Q: hipcc's wait for a load counts the
    // loads issued after it on the path that issued the FEWEST, so a branch-skipped load between
    // Q and its use would make the R_ONLY path wait for the tile and the own V before P0
    short8_t mreg[kMPer];
    {
      // rows >= K are zero in the program: past the resource, so they read as zeros without a fetch
      const __amdgpu_buffer_rsrc_t rm = make_rsrc(mg, (int64_t)K * P2P_PROGRAM_DENSE * 2);
#pragma unroll
      for (int j = 0; j < kMPer; ++j)
        mreg[j] = __builtin_bit_cast(short8_t, __builtin_amdgcn_raw_buffer_load_b128(rm, (tid + j * NT) * 16, 0, 0));
    }
    __builtin_amdgcn_sched_barrier(0);
    own_early = !r_only;
    load_kv(n, kc1, vc1, true, false);   // own V
    __builtin_amdgcn_sched_barrier(0);
    if (own_early) {
      load_kv(n, kc1, vc1, false, true);   // own K
      load_q(n, qf1);
    }
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < kMPer; ++j) {
        const int i = tid + j * NT;
        if (i < kMCh) reinterpret_cast<short8_t*>(Ms)[i] = mreg[j];
      }
    };
    finish_prologue();
    P2P_CROSS_STAMP(19)
    if (!late) store_tile();
    P2P_CROSS_STAMP(20)
    {  // per-column coefficients next to the tile, read back after the barriers:
      // P' = alpha*post*(c_rep*P_b + R) + (1-alpha)*P_b = P_b*A + R*B
      float* col = dcol;
      if (w < KR) {
        const float ap = aw * pw;
        col[w] = fmaf(ap, cw, 1.f - aw);
        col[KR + w] = ap;
      }
    }
    P2P_CROSS_STAMP(21)
    store_kv(kc0, vc0, false);
    // R_ONLY: the own V goes to its LDS image in this phase (the P0 / R phase reads only K and the
    // mapper), so no second staging phase follows
    if (r_only && !late) store_kv(kc1, vc1, true, false);
    P2P_CROSS_STAMP(22)
    __syncthreads();
    if (touch_when == 1 || touch_when == 3) touch();
    P2P_CROSS_STAMP(8)
    {
      // which blend halves the row uses (every wave scans the coefficients itself): bit 0 some
      // A != 0 -> this edit's own softmax, bit 1 some B != 0 -> P0 and R.  A Replace step with
      // alpha = 1 on every word (main.py:189) needs only R, one with alpha = 0 only its own P_b;
      // dropping the other half is exact (fma(P, 0, x) = x, fma(P, A, R * 0) = P A)
      const float* col = dcol;
      const int c0 = lane, c1 = lane + 64;
      const bool a0 = c0 < K && col[c0] != 0.f, a1 = c1 < K && col[c1] != 0.f;
      const bool b0 = c0 < K && col[KR + c0] != 0.f, b1 = c1 < K && col[KR + c1] != 0.f;
      dense_flags = (__any(a0 || a1) ? 1 : 0) | (__any(b0 || b1) ? 2 : 0);
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) Rd[kb] = f32x16_t{};
    if (dense_flags & 2) {
    float p0[KB][16];
    probs(qf, p0);
    if (late) {
      store_tile();      // (workgroup-uniform branch: every wave reads the same coefficients)
      __syncthreads();
    }
    P2P_CROSS_STAMP(9)
    // R = M^T P0 on the f16 MFMA: the mapper weights (1, 1/2, 1/4, ...) are exact in f16 and P0 in
    // [0, 1] rounds to 11 significant bits (|dR| <= 2^-12 R, inside the 2e-3 bar); every mapper
    // fragment read once; one 32-key block at a time (the scheduler would otherwise hoist all 18
    // fragment reads)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        short8_t ph;
#pragma unroll
        for (int r = 0; r < 8; ++r) ph[r] = (short)__builtin_bit_cast(uint16_t, (_Float16)p0[kb][8 * s2 + r]);
#pragma unroll
        for (int dt = 0; dt < KB; ++dt) {
          const MmaBf16::frag af =
              vt_frag<P2P_PROGRAM_DENSE>(reinterpret_cast<const uint16_t*>(Ms), kb * 32, s2, dt * 32, lane);
          typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
          Rd[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, af.v),
                                                          __builtin_bit_cast(f16x8_t, ph), Rd[dt], 0, 0, 0);
        }
      }
    }
    }
    if (own_early) {
#pragma unroll
      for (int t = 0; t < NKT; ++t) qf[t] = qf1[t];
    } else if (!r_only || (dense_flags & 1)) {
      load_q(n, qf);
    }
    if (r_only && late) store_kv(kc1, vc1, true, false);   // (V is read only after the barrier below)
    __syncthreads();  // every wave is done with the source K tile and the mapper tile
    P2P_CROSS_STAMP(10)
   }
  }
  if (edit && !dense) {
    // ---- source probabilities P0 for these rows -> this wave's LDS slab
    load_q(first, qf);
    {
      Chunk8<IO> kc[NCH], vc[NCH];
      load_kv(first, kc, vc, false);
      finish_prologue();
      store_kv(kc, vc, false);
    }
    __syncthreads();
    if (touch_when == 1 || touch_when == 3) touch();
    probs(qf, sv);
    load_q(n, qf);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int w = kb * 32 + acc_row(r, hh);
        if (w < K) slab[qi * P0S + w] = sv[kb][r];
      }
    __syncthreads();  // slab written; every wave is done reading the source K tile
  } else if (!edit) {
    load_q(n, qf);
  }
  auto stage_own = [&]() __attribute__((always_inline)) {
    Chunk8<IO> kc[NCH], vc[NCH];
    load_kv(n, kc, vc, true);
    if (!edit) finish_prologue();   // (the edit paths called it with their first loads)
    store_kv(kc, vc, true);
  };
  bool own_staged = true;
  if constexpr (kDenseOk) {
    if (own_early) {
      store_kv(kc1, vc1, true);
    } else if (r_only) {
      // own V is in LDS already; own K only if the coefficients contradict the host's flag
      own_staged = (dense_flags & 1) != 0;
      if (own_staged) {
        Chunk8<IO> kc[NCH], vc[NCH];
        load_kv(n, kc, vc, false);
        store_kv(kc, vc, false);
      }
    } else {
      stage_own();
    }
  } else {
    stage_own();
  }
  if (own_staged) __syncthreads();   // (workgroup-uniform: every wave reads the same coefficients)
  if (!edit && (touch_when == 1 || touch_when == 3)) touch();
  P2P_CROSS_STAMP(11)
  if (!dense || (dense_flags & 1)) {
    probs(qf, sv);
  } else {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sv[kb][r] = 0.f;   // A = 0 on every column: P' = R B
  }
  P2P_CROSS_STAMP(12)

  if (dense) {
    // a lane's columns come in runs of 4 (r & 3): one 16-byte LDS read per run and table;
    // one 32-column block at a time (hoisting every read costs ~150 VGPRs)
    const float* const col = dcol;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int w0 = kb * 32 + 8 * g + 4 * hh;
        const f32x4_t A4 = *reinterpret_cast<const f32x4_t*>(col + w0);
        const f32x4_t B4 = *reinterpret_cast<const f32x4_t*>(col + KR + w0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g + j;
          sv[kb][r] = fmaf(sv[kb][r], A4[j], Rd[kb][r] * B4[j]);   // columns >= K: A = 1, B = 0
        }
      }
    }
  } else if (edit) {
#pragma clang fp contract(off)
    const int tmax = reinterpret_cast<const int*>(prog)[2];
    const char* const rec = prog + P2P_PROGRAM_HEADER_BYTES + (int64_t)(b - 1) * P2P_PROGRAM_REC_BYTES;
    const float* const ce = reinterpret_cast<const float*>(rec);
    const float* const pe = ce + P2P_PROGRAM_COLS;
    const int2* const terms = reinterpret_cast<const int2*>(pe + P2P_PROGRAM_COLS);
    const float* const al = a.grp_alpha[gi] + (b - 1) * K;
    const float* const P0 = slab + qi * P0S;
    float acc[KB][16];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kb][r] = ce[kb * 32 + acc_row(r, hh)] * sv[kb][r];
    for (int t = 0; t < tmax; ++t) {  // wave-uniform; padding terms add +0
      const int2* const plane = terms + t * P2P_PROGRAM_COLS;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int2 tm = plane[kb * 32 + acc_row(r, hh)];
          acc[kb][r] = acc[kb][r] + __int_as_float(tm.y) * P0[tm.x];
        }
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int w = kb * 32 + acc_row(r, hh);
        if (w < K) {
          const float pb = sv[kb][r];
          const float R = pe[w] * acc[kb][r];
          const float aw = al[w];
          sv[kb][r] = aw * R + (1.f - aw) * pb;
        }
      }
  }

  P2P_CROSS_STAMP(13)
  // ---- AttentionStore epilogue: post-edit maps, whole rows through the wave's slab
  if (stored) {
    // the slab is this wave's own region: wave-level ordering suffices (the dense tile under it
    // died at the post-R barrier; the term-plane path's P0 gather reads only this wave's slab)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // key blocks wholly below K write every register (one branch per block, wave-uniform); only
    // the block that crosses K checks its keys (a per-element check costs a compare and two exec
    // updates around every LDS write)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      if (kb * 32 + 32 <= K) {
#pragma unroll
        for (int r = 0; r < 16; ++r) slab[qi * K + kb * 32 + acc_row(r, hh)] = sv[kb][r];
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int w = kb * 32 + acc_row(r, hh);
          if (w < K) slab[qi * K + w] = sv[kb][r];
        }
      }
    }
    P2P_CROSS_STAMP(16)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    P2P_CROSS_STAMP(17)
    const int rows = min(32, a.P - p0w);
    // LocalBlend's word sums of these rows (alpha- and substruct-weighted), folded here so the
    // blend never re-reads the maps: each lane sums the words it holds in registers (runs of four
    // consecutive words, weights read 16 bytes at a time), the two lane halves of a row add, and
    // lanes 0-31 write the alpha sum, 32-63 the substruct sum.  (A pairwise order instead of
    // blend_wordsum_kernel's sequential one: the fold is already a measured summation-order
    // deviation from the map path; the sequential chain cost ~3k cycles per workgroup.)
    if (blend_on) {
      const bool has_sub = a.grp_bsub[gi] != nullptr;
      // (no key checks: past K both the probabilities -- masked to exact zeros by every path --
      // and the weights are 0, so those terms add +0; runs past the short tail are skipped)
      float sa = 0.f, ss = 0.f;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          if (kb == KB - 1 && g4 >= 2 && short_tail) continue;   // registers 8..15: keys >= 80
          const int w0 = kb * 32 + 8 * g4 + 4 * hh;
          const f32x4_t ta = *reinterpret_cast<const f32x4_t*>(&btab[0][w0]);
          const f32x4_t ts = *reinterpret_cast<const f32x4_t*>(&btab[1][w0]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            sa = fmaf(sv[kb][4 * g4 + j], ta[j], sa);
            ss = fmaf(sv[kb][4 * g4 + j], ts[j], ss);
          }
        }
      sa += other_half(sa);
      ss += other_half(ss);
      if (qi < rows) {
        const float acc = hh == 0 ? sa : (has_sub ? ss : 0.f);
        *bdst = a.store_accumulate ? (touch_when == 3 ? bsum_old : *bdst) + acc : acc;
      }
    }
    P2P_CROSS_STAMP(18)
    if (rows > 0) {
      float* g = a.store + ((int64_t)(slot + h) * a.P + p0w) * (int64_t)K;
      const int count = rows * K;
      if (touch_when == 3 && rmw_vec && a.store_accumulate) {
        rmw_add_store<kRmwF4>(g, slab, count, lane, rmwbuf);
      } else if (((uintptr_t)g & 15) == 0 && (count & 3) == 0) {
        store_rows_rmw<32 * KR / 4>(g, slab, count, a.store_accumulate != 0, lane);
        // keeps the prefetch touches alive (never true: a running sum of probabilities is finite)
        if (__builtin_expect(touch0 == -INFINITY || touch1 == -INFINITY, 0)) g[0] = touch0 + touch1;
      } else {
        for (int i = lane; i < count; i += 64) g[i] = a.store_accumulate ? g[i] + slab[i] : slab[i];
      }
    }
  }

  P2P_CROSS_STAMP(14)
  // ---- O = P' V
  f32x16_t O[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) pv_block<VS, NDT>(MP{}, O, Vs, kb * 32, sv[kb], lane);
  P2P_CROSS_STAMP(15)
  store_o(O, 1.f);
}

// ====================================================================== launcher
template <typename IO, typename MQ, typename MP, int D, int W>
static int launch_cross_w(const CrossArgs& a, bool dense, hipStream_t st) {
  CrossArgs b = a;
  b.n_qtiles = (a.P + 32 * W - 1) / (32 * W);
  // the slab holds a [32, K] f32 block per wave: stride K | 1 (odd, so the 32 rows of one
  // column hit distinct banks) for the edit gather, K for the store rows
  b.slab_stride = a.K | 1;
  // the dense path (16-bit PV only) stages the mapper tile in the same dynamic region the slab
  // uses later (the tile is dead before any store)
  constexpr bool kDense = MP::kElemBytes == 2;
  if (dense && !kDense) return P2P_E_ARG;
  b.slab = (a.any_store || ((a.edit_terms || a.edit_dense) && !dense)) ? 1 : 0;
  size_t dyn = b.slab ? (size_t)W * 32 * b.slab_stride * sizeof(float) : 0;
  const size_t tile = (size_t)P2P_PROGRAM_DENSE * P2P_PROGRAM_DENSE * sizeof(uint16_t);
  if (dense && dyn < tile) dyn = tile;
  dim3 grid(b.n_qtiles * a.H * a.N), block(64 * W);
  if (dense)
    launch_kernel((cross_attn_kernel<IO, MQ, MP, D, W, kDense>), grid, block, dyn, st, b);
  else
    launch_kernel((cross_attn_kernel<IO, MQ, MP, D, W, false>), grid, block, dyn, st, b);
  return (int)hipGetLastError();
}

int launch_cross_entry(const CrossArgs& a, int prec, int d, CrossKernel k, hipStream_t st) {
  if (is_group(k)) return P2P_E_ARG;
  return with_precision(prec, [&](auto pr) {
    return with_head_dim(d, [&](auto dd) -> int {
      using IO = typename decltype(pr)::IO;
      using MQ = typename decltype(pr)::MQ;
      using MP = typename decltype(pr)::MP;
      constexpr int D = decltype(dd)::value;
      // the one wave count compiled for this precision and head dim (p2p_select.h picks the same)
      constexpr int W = cross_waves(D, MP::kElemBytes == 2);
      if ((k == CROSS_ENTRY_W2) != (W == 2)) return P2P_E_ARG;
      return launch_cross_w<IO, MQ, MP, D, W>(a, k == CROSS_ENTRY_W4_DENSE, st);
    });
  });
}

}  // namespace p2p

#ifdef P2P_EXPERIMENTS
// dst == nullptr: clear the stamps
extern "C" int p2p_diag_cross_stamps(void* dst, int64_t bytes) {
  const int64_t n = (int64_t)sizeof(p2p::g_cross_stamps);
  if (dst == nullptr) {
    void* p = nullptr;
    hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(p2p::g_cross_stamps));
    return e != hipSuccess ? (int)e : (int)hipMemset(p, 0, n);
  }
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(p2p::g_cross_stamps), bytes < n ? bytes : n, 0, hipMemcpyDeviceToHost);
}
#endif
