// The self-attention kernels that write probabilities to HBM (gfx950), every precision and head dim:
//
// self_maps_kernel  : the AttentionStore epilogue (main.py:129-142) for self layers whose maps
//                     are kept, from the fused kernel's row log-sum-exp.
// self_probs_kernel : the first half of the materialise protocol (probabilities to HBM; the P V
//                     half is self_pv_kernel, p2p_self.hip).
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

// ====================================================================== stored self maps
// AttentionStore epilogue of the self layers whose maps are kept (main.py:129-142, P <= 32^2;
// the stored tensor is the post-injection map, main.py:181-195).  self_attn_fused_kernel<…,EXACT>
// (p2p_self.hip) has produced O and every row's log-sum-exp (log2 domain, scale folded); this kernel recomputes
// S = Q K^T in the NON-transposed orientation -- key on the lane, query on the accumulator
// row -- so p = exp2(c s - lse) leaves as 128-byte row segments per half-wave: the read-add-
// write of the running sum is the whole cost of the layer and is HBM-bound.  With the softmax
// statistics known, keys split freely: one wave = 32 queries x kw keys, one workgroup = four
// consecutive key chunks, so the grid is as wide as the map.  K fragments come straight from
// global memory (a [K, d] head slice is L2-resident); no LDS, no barrier.
template <typename IO, typename MQ, int D>
__global__ __launch_bounds__(256) void self_maps_kernel(SelfArgs a, int kw, int n_kgroups) {
  constexpr int DK = (D + 15) / 16 * 16;
  constexpr int NKT = DK / 16;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hh = lane >> 5;
  const int li = lane & 31;

  int rest = xcd_remap(blockIdx.x, gridDim.x);
  const int kg = rest % n_kgroups;
  rest /= n_kgroups;
  const int qb = rest % a.n_qtiles;
  rest /= a.n_qtiles;
  const int h = rest % a.H;
  const int n = a.map_entry[rest / a.H];
  const int src = a.qk_src[n];
  const int P = a.P;
  const int K = a.K;
  const int k0 = (kg * 4 + wave) * kw;
  if (k0 >= K) return;  // wave-uniform: no barrier in this kernel
  const int k1 = min(K, k0 + kw);
  const int p0 = qb * 32;
  const float c = a.scale_log2;

  const IO* const qp = static_cast<const IO*>(a.q) + (int64_t)src * a.bsq + h * D;
  const IO* const kp = static_cast<const IO*>(a.k) + (int64_t)src * a.bsk + h * D;
  typename MQ::frag qf[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int col = 16 * t + 8 * hh;
    qf[t] = (p0 + li < P && col < D) ? MQ::load_q(qp + (int64_t)(p0 + li) * a.ldq + col) : MQ::zero();
  }
  // per accumulator register r: query row p0 + acc_row(r, hh), its lse and map row
  const float* const lse = a.lse + (int64_t)(n * a.H + h) * P;
  float* const mp = a.store + (int64_t)(a.store_slot[n] + h) * P * (int64_t)K;
  float lr[16];
  bool rok[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = p0 + acc_row(r, hh);
    rok[r] = row < P;
    lr[r] = rok[r] ? lse[row] : 0.f;
  }
  const bool acc_on = a.store_accumulate != 0;
  // one 32-key block per step, its running-sum reads issued before its first write; non-temporal
  // accesses (the map streams through once per step: -7.5 % at G2 with the maps HBM-resident; two
  // key blocks per step measured +2 %).  The loops over the NB = 1 blocks stay written out: without
  // them hipcc generates other code for the d = 8 instantiations.
  constexpr int NB = 1;
  for (int kb = k0; kb < k1; kb += 32 * NB) {
    float old[NB][16];
    if (acc_on) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int key = kb + 32 * j + li;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          old[j][r] = (key < k1 && rok[r])
                          ? __builtin_nontemporal_load(mp + (int64_t)(p0 + acc_row(r, hh)) * K + key)
                          : 0.f;
      }
    }
    f32x16_t acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const IO* const krow = kp + (int64_t)min(kb + 32 * j + li, K - 1) * a.ldk;
      acc[j] = f32x16_t{};
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        const int col = 16 * t + 8 * hh;
        const typename MQ::frag kf = col < D ? MQ::load_q(krow + col) : MQ::zero();
        MQ::mma(acc[j], qf[t], kf);  // A = Q rows, B = K rows: S (query x key), key on the lane
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int key = kb + 32 * j + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (key < k1 && rok[r]) {
          float v = fast_exp2(fmaf(acc[j][r], c, -lr[r]));
          if (acc_on) v += old[j][r];
          __builtin_nontemporal_store(v, mp + (int64_t)(p0 + acc_row(r, hh)) * K + key);
        }
      }
    }
  }
}

// ====================================================================== materialised probabilities
// The materialise protocol's first half (controllers that override forward(attn, ...),
// main.py:85-98): probs[n*H + h] = softmax(Q K^T * scale), f32 [N*H, P, K] (ptp_utils.py:195-204,
// with the optional key mask of :197-201 and its head-major repeat of the mask rows).  HBM-bound
// (G1: 4.3 GB written per layer), so the store side follows self_maps_kernel: one workgroup = 32
// queries x all keys, the four waves split the keys.  Pass 1 (S^T, query on the lane: reductions
// stay in the lane) gives each wave's partial row max / sum, combined across the waves in LDS;
// pass 2 recomputes S with the key on the lane and writes p = exp2(t - M) / L as 128-byte row
// segments per half-wave.  A masked key scores -FLT_MAX after the scale (the reference fills the
// scaled logits with -finfo.max): p = 0 beside any unmasked key, 1/K on a fully masked row.
template <typename IO, typename MQ, int D>
__global__ __launch_bounds__(256) void self_probs_kernel(SelfArgs a, int kw) {
  constexpr int DK = (D + 15) / 16 * 16;
  constexpr int NKT = DK / 16;
  constexpr float kNeg = -3.402823466e38f;
  __shared__ float sm[4][32], sl[4][32];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hh = lane >> 5;
  const int li = lane & 31;

  int rest = xcd_remap(blockIdx.x, gridDim.x);
  const int qb = rest % a.n_qtiles;
  rest /= a.n_qtiles;
  const int h = rest % a.H;
  const int n = rest / a.H;
  const int P = a.P;
  const int K = a.K;
  const int k0 = wave * kw;
  const int k1 = min(K, k0 + kw);  // empty for trailing waves when K < 4 kw: they still sync
  const int p0 = qb * 32;
  const float c = a.scale_log2;
  const uint8_t* const km = a.key_mask ? a.key_mask + (int64_t)((n * a.H + h) % a.N) * K : nullptr;

  const IO* const qp = static_cast<const IO*>(a.q) + (int64_t)n * a.bsq + h * D;
  const IO* const kp = static_cast<const IO*>(a.k) + (int64_t)n * a.bsk + h * D;
  typename MQ::frag qf[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int col = 16 * t + 8 * hh;
    qf[t] = (p0 + li < P && col < D) ? MQ::load_q(qp + (int64_t)(p0 + li) * a.ldq + col) : MQ::zero();
  }
  auto scores = [&](int kb, bool transposed, f32x16_t& acc) {
    const IO* const krow = kp + (int64_t)min(kb + li, K - 1) * a.ldk;
    acc = f32x16_t{};
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const int col = 16 * t + 8 * hh;
      const typename MQ::frag kf = col < D ? MQ::load_q(krow + col) : MQ::zero();
      if (transposed) MQ::mma(acc, kf, qf[t]);  // S^T: key on the accumulator row, query on the lane
      else MQ::mma(acc, qf[t], kf);             // S:   query on the accumulator row, key on the lane
    }
  };

  // ---- pass 1: this wave's row max / sum over its keys (t = s * c, or kNeg when masked)
  float m = -INFINITY, l = 0.f;
  for (int kb = k0; kb < k1; kb += 32) {
    f32x16_t acc;
    scores(kb, true, acc);
    float tv[16];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb + acc_row(r, hh);
      tv[r] = key >= k1 ? -INFINITY : (km && !km[key]) ? kNeg : acc[r] * c;
      mx = fmaxf(mx, tv[r]);
    }
    const float mnew = fmaxf(m, mx);
    if (mnew != -INFINITY) {
      float ls = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ls += fast_exp2(tv[r] - mnew);
      l = fmaf(l, fast_exp2(m - mnew), ls);
      m = mnew;
    }
  }
  {  // the other half-wave holds the other keys of the same query
    const float m2 = __shfl_xor(m, 32), l2 = __shfl_xor(l, 32);
    const float M = fmaxf(m, m2);
    if (M != -INFINITY) {
      l = (m == -INFINITY ? 0.f : l * fast_exp2(m - M)) + (m2 == -INFINITY ? 0.f : l2 * fast_exp2(m2 - M));
      m = M;
    }
  }
  if (hh == 0) {
    sm[wave][li] = m;
    sl[wave][li] = l;
  }
  __syncthreads();
  // per accumulator register r of the S orientation: query row p0 + acc_row(r, hh)
  float Mr[16], Ir[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, hh);
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, sm[w][row]);
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) L += sm[w][row] == -INFINITY ? 0.f : sl[w][row] * fast_exp2(sm[w][row] - M);
    Mr[r] = M;
    Ir[r] = 1.f / L;
  }

  // ---- pass 2: exact probabilities, key on the lane
  float* const pp = a.store + (int64_t)(n * a.H + h) * P * (int64_t)K;
  for (int kb = k0; kb < k1; kb += 32) {
    f32x16_t acc;
    scores(kb, false, acc);
    const int key = kb + li;
    if (key < k1) {
      const bool masked = km && !km[key];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = p0 + acc_row(r, hh);
        if (row < P) {
          const float x = masked ? kNeg - Mr[r] : fmaf(acc[r], c, -Mr[r]);
          // non-temporal: a write-once stream (G1 1.33 -> 1.04 ms, G2 118 -> 104 us)
          __builtin_nontemporal_store(fast_exp2(x) * Ir[r], pp + (int64_t)row * K + key);
        }
      }
    }
  }
}

// ====================================================================== launchers
int run_self_maps(const SelfArgs& a, int io_dtype, int compute, int d, hipStream_t st) {
  if (a.n_maps < 1) return 0;
  return with_precision(select_precision(io_dtype, compute), [&](auto pr) {
    return with_head_dim(d, [&](auto dd) {
      SelfArgs b = a;
      // keys per wave: a quarter of the row (whole 32-key blocks), at most 256 -> a workgroup
      // spans up to 1024 keys; wider rows take more key groups
      const int kw = min(256, ((a.K + 3) / 4 + 31) / 32 * 32);
      const int n_kgroups = (a.K + 4 * kw - 1) / (4 * kw);
      b.n_qtiles = (a.P + 31) / 32;
      dim3 grid(n_kgroups * b.n_qtiles * a.H * a.n_maps), block(256);
      launch_kernel((self_maps_kernel<typename decltype(pr)::IO, typename decltype(pr)::MQ, decltype(dd)::value>),
                    grid, block, 0, st, b, kw, n_kgroups);
      return (int)hipGetLastError();
    });
  });
}

int run_self_probs(const SelfArgs& a, int io_dtype, int compute, int d, hipStream_t st) {
  return with_precision(select_precision(io_dtype, compute), [&](auto pr) {
    return with_head_dim(d, [&](auto dd) {
      SelfArgs b = a;
      const int kw = ((a.K + 3) / 4 + 31) / 32 * 32;  // keys per wave: a quarter of the row
      b.n_qtiles = (a.P + 31) / 32;
      dim3 grid(b.n_qtiles * a.H * a.N), block(256);
      launch_kernel((self_probs_kernel<typename decltype(pr)::IO, typename decltype(pr)::MQ, decltype(dd)::value>),
                    grid, block, 0, st, b, kw);
      return (int)hipGetLastError();
    });
  });
}

}  // namespace p2p
