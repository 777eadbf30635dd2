// The text encoders' own kernels (p2p_amd/text_encoder.py: CLIP; p2p_amd/ldm_bert.py: LDMBert):
// self-attention over the <= 96 prompt tokens at head dim 64 -- causal for CLIP, bidirectional with
// an optional per-entry key count for LDMBert -- LayerNorm with the residual add and a GEMM's bias
// in front of it, and bias + quick-GELU (CLIP) or bias + erf-GELU (LDMBert) behind fc1.  16-bit I/O
// (bf16 or f16), f32 arithmetic, one rounding at the store; every reduction runs in a fixed order
// (no atomics), so two launches on the same input are bit-identical.
//
// text_attn_kernel follows the transposed-fragment convention of p2p_device.h (S^T = K Q^T and
// O^T = V^T P^T, query on the lane) and the staging of cross_attn_kernel's lean path: one
// workgroup per (batch entry, head) stages K and V once -- K row-major with KStride rows for the
// ds_read_b128 fragment loads, V row-major with VStrideBf16 rows for ds_read_b64_tr_b16 -- and wave
// w owns queries 32 w .. 32 w + 31.  CAUSAL: causality is the loop bound: wave w visits key blocks
// 0 .. w (six of the nine 32 x 32 blocks of a 96 x 96 tile), and only its diagonal block is masked.
// The waves' work is 1 : 2 : 3 blocks; pairing blocks to even it out was not tried (DESIGN.md
// §4.13).  Keys T .. 95 are zero rows of the LDS tile, which causality hides from every stored row.
// !CAUSAL: an entry attends to its first L keys (L = T, or its key count clamped into [1, T]);
// every wave visits every key block below L, an even split, and nothing hides the zero rows L .. 95
// -- they would score 0, not -inf -- so the block that holds key L masks them by index.  Either
// way the T x T matrix lives in registers only.
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

// a probability as the P V MFMA will see it: rounded to the operand format
__device__ __forceinline__ float round_p(MmaBf16, float p) { return bf2f(f2bf(p)); }
__device__ __forceinline__ float round_p(MmaF16, float p) { return h2f(f2h(p)); }

constexpr int kCausalD = 64;
constexpr int kCausalWaves = P2P_MAX_KEYS_CROSS / 32;

template <bool CAUSAL, typename IO, typename MQ, typename MP>
__global__ __launch_bounds__(64 * kCausalWaves) void text_attn_kernel(TextAttnArgs a) {
  using EK = typename MQ::elem;
  using EV = typename MP::elem;
  constexpr int D = kCausalD;
  constexpr int NKT = D / 16;
  constexpr int NDT = D / 32;
  constexpr int KB = kCausalWaves;
  constexpr int KR = KB * 32;
  constexpr int KS = KStride<D, 2>::value;
  constexpr int VS = VStrideBf16<D>::value;
  constexpr int NT = 64 * KB;
  constexpr int CPR = D / 8;
  constexpr int NCH = KR * CPR / NT;
  static_assert(KR * CPR % NT == 0, "every thread stages the same number of chunks");
  static_assert(MQ::planes == 1 && sizeof(EK) == 2 && sizeof(EV) == 2, "16-bit operands");
  constexpr int KBYTES = KR * KS * 2;
  constexpr int VBYTES = KR * VS * 2;
  __shared__ __attribute__((aligned(16))) char smem[KBYTES + VBYTES];
  EK* const Ks = reinterpret_cast<EK*>(smem);
  EV* const Vs = reinterpret_cast<EV*>(smem + KBYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;
  const int qi = lane & 31;
  const int n = blockIdx.x / a.H;
  const int h = blockIdx.x - n * a.H;
  const int T = a.T;
  const int p = wave * 32 + qi;
  const bool prow = p < T;
  // the keys this entry attends to (workgroup-uniform).  L >= 1: key 0 is always visible
  int L = T;
  if (!CAUSAL && a.key_counts) L = min(max(a.key_counts[n], 1), T);

  // every global load first: this lane's Q fragments, this thread's K and V chunks
  typename MQ::frag qf[NKT];
  {
    const IO* qp = static_cast<const IO*>(a.q) + (int64_t)n * a.bsq + h * D + (int64_t)p * a.ldq;
#pragma unroll
    for (int t = 0; t < NKT; ++t) qf[t] = prow ? MQ::load_q(qp + 16 * t + 8 * hh) : MQ::zero();
  }
  const IO* kp = static_cast<const IO*>(a.k) + (int64_t)n * a.bsk + h * D;
  const IO* vp = static_cast<const IO*>(a.v) + (int64_t)n * a.bsv + h * D;
  Chunk8<IO> kc[NCH], vc[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cidx = tid + i * NT;
    const int row = cidx / CPR;
    const int ch = cidx - row * CPR;
    if (row < L) {   // rows L .. 95 are never read from memory: their LDS rows are zero
      kc[i].load(kp + (int64_t)row * a.ldk + ch * 8);
      vc[i].load(vp + (int64_t)row * a.ldv + ch * 8);
    } else {
      kc[i].clear();
      vc[i].clear();
    }
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cidx = tid + i * NT;
    const int row = cidx / CPR;
    const int ch = cidx - row * CPR;
    MQ::stage(kc[i], Ks + row * KS + ch * 8, 0);
    vc[i].store(Vs + row * VS + ch * 8);
  }
  __syncthreads();
  if (wave * 32 >= T) return;   // a wave without rows (T <= 64): done after the only barrier

  float sv[KB][16];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    // wave-uniform: the blocks above the diagonal, or past the last key, are never computed
    if (CAUSAL ? kb > wave : kb * 32 >= L) continue;
    f32x16_t acc = {};
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const typename MQ::frag fa = MQ::load_k(Ks + (kb * 32 + qi) * KS + 16 * t + 8 * hh, 0);
      MQ::mma(acc, fa, qf[t]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sv[kb][r] = acc[r];
    if (CAUSAL) {
      if (kb == wave) {   // the diagonal block: key 32 kb + j against query 32 kb + qi
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (acc_row(r, hh) > qi) sv[kb][r] = -INFINITY;
      }
    } else if (kb * 32 + 32 > L) {   // the block that holds key L: the zero rows L .. are masked by index
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kb * 32 + acc_row(r, hh) >= L) sv[kb][r] = -INFINITY;
    }
  }
  const float c = a.scale_log2;
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    if (CAUSAL ? kb > wave : kb * 32 >= L) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sv[kb][r]);
  }
  // key 0 is unmasked for every query, so mx is finite in both halves' maximum
  mx = fmaxf(mx, other_half(mx)) * c;
  float l = 0.f;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    if (CAUSAL ? kb > wave : kb * 32 >= L) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sv[kb][r] = round_p(MP{}, fast_exp2(fmaf(sv[kb][r], c, -mx)));   // a masked key: exp2(-inf) = 0
      l += sv[kb][r];
    }
  }
  l += other_half(l);
  f32x16_t O[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    if (CAUSAL ? kb > wave : kb * 32 >= L) continue;
    pv_block<VS, NDT>(MP{}, O, Vs, kb * 32, sv[kb], lane);
  }
  // every row attends to key 0 at least, and the row's largest weight is exp2(0) = 1: l >= 1, no
  // row is empty and no guard against 0 / 0 is needed
  const float inv = 1.f / l;
  if (prow) {   // rows >= T are never stored
    IO* const op = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D + (int64_t)p * a.ldo;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store4(op + dt * 32 + 8 * g + 4 * hh, O[dt][4 * g] * inv, O[dt][4 * g + 1] * inv, O[dt][4 * g + 2] * inv,
               O[dt][4 * g + 3] * inv);
  }
}

// sum over the wave, the same bits in every lane (each step adds the same two values in both lanes
// of a pair)
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 8-element vectors a lane keeps in registers: rows of up to 64 * 4 * 8 = 2048 channels
constexpr int kLnVecs = 4;
constexpr int kLnMaxChannels = 64 * kLnVecs * 8;
constexpr int kLnRowsPerBlock = 4;

// one wave per row, the row in registers between the three sweeps: s = x + add + add_bias rounded
// to the tensor type (and stored to sum_out), mean, centred variance, y
template <bool F16>
__global__ __launch_bounds__(64 * kLnRowsPerBlock) void layer_norm_kernel(p2p_layer_norm_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kLnRowsPerBlock + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const int nv = a.channels >> 3;
  const int64_t base = row * a.channels;
  const uint16_t* const x = static_cast<const uint16_t*>(a.x) + base;
  const uint16_t* const add = a.add ? static_cast<const uint16_t*>(a.add) + base : nullptr;
  const uint16_t* const bias = static_cast<const uint16_t*>(a.add_bias);
  uint16_t* const sum_out = a.sum_out ? static_cast<uint16_t*>(a.sum_out) + base : nullptr;
  float s[kLnVecs][8];
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < kLnVecs; ++i) {
    const int iv = lane + 64 * i;
    if (iv < nv) {
      const u16x8_t vx = *reinterpret_cast<const u16x8_t*>(x + 8 * iv);
      u16x8_t va = {}, vb = {}, vs;
      if (add) va = *reinterpret_cast<const u16x8_t*>(add + 8 * iv);
      if (bias) vb = *reinterpret_cast<const u16x8_t*>(bias + 8 * iv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = ld16<F16>(vx[j]);
        if (add) t += ld16<F16>(va[j]);
        if (bias) t += ld16<F16>(vb[j]);
        vs[j] = st16<F16>(t);
        // the statistics and y come from the rounded sum: what the next reader of sum_out sees
        s[i][j] = ld16<F16>(vs[j]);
        tot += s[i][j];
      }
      if (sum_out) *reinterpret_cast<u16x8_t*>(sum_out + 8 * iv) = vs;
    }
  }
  const float inv_c = 1.f / (float)a.channels;
  const float mean = wave_sum(tot) * inv_c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kLnVecs; ++i)
    if (lane + 64 * i < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = s[i][j] - mean;
        q += d * d;
      }
    }
  const float rstd = 1.f / sqrtf(wave_sum(q) * inv_c + a.eps);
  const uint16_t* const gamma = static_cast<const uint16_t*>(a.gamma);
  const uint16_t* const beta = static_cast<const uint16_t*>(a.beta);
  uint16_t* const y = static_cast<uint16_t*>(a.y) + base;
#pragma unroll
  for (int i = 0; i < kLnVecs; ++i) {
    const int iv = lane + 64 * i;
    if (iv < nv) {
      const u16x8_t vg = *reinterpret_cast<const u16x8_t*>(gamma + 8 * iv);
      const u16x8_t vb = *reinterpret_cast<const u16x8_t*>(beta + 8 * iv);
      u16x8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = st16<F16>((s[i][j] - mean) * rstd * ld16<F16>(vg[j]) + ld16<F16>(vb[j]));
      *reinterpret_cast<u16x8_t*>(y + 8 * iv) = o;
    }
  }
}

// The many-row form, for the U-Net's transformer blocks (thousands of rows of 320 or 640 channels):
// LPR lanes per row, 64 / LPR rows per wave, so that no lane idles at C = 40 LPR and a wave has
// 64 / LPR times the bytes in flight.  Lane l of a row's group holds vectors l, l + LPR, ..; the
// sums run over the lane's vectors in that order, then over the group by xor-shuffles: a fixed
// order, but not layer_norm_kernel's, so the host gives this form only the plain norms (no add) of
// channels <= kLnGroupedMaxChannels, below the text encoders' widths: where it measured faster.
constexpr int kLnGroupVecs = 5;
constexpr int kLnGroupedMaxChannels = 16 * kLnGroupVecs * 8;   // 640
constexpr int kLnGroupedThreads = 256;

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool F16, int LPR>
__global__ __launch_bounds__(kLnGroupedThreads) void layer_norm_grouped_kernel(p2p_layer_norm_args a) {
  constexpr int kRows = kLnGroupedThreads / LPR;   // rows per workgroup
  const int sub = threadIdx.x % LPR;
  const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / LPR;
  // a group past the last row loads and stores nothing, but stays for the shuffles of its wave
  const bool live = row < a.rows;
  const int nv = a.channels >> 3;
  const int64_t base = live ? row * a.channels : 0;
  const uint16_t* const x = static_cast<const uint16_t*>(a.x) + base;
  const uint16_t* const add = a.add ? static_cast<const uint16_t*>(a.add) + base : nullptr;
  const uint16_t* const bias = static_cast<const uint16_t*>(a.add_bias);
  uint16_t* const sum_out = a.sum_out ? static_cast<uint16_t*>(a.sum_out) + base : nullptr;
  u16x8_t vx[kLnGroupVecs], va[kLnGroupVecs];
  // every load of the row first
#pragma unroll
  for (int i = 0; i < kLnGroupVecs; ++i) {
    const int iv = sub + LPR * i;
    vx[i] = u16x8_t{};
    va[i] = u16x8_t{};
    if (live && iv < nv) {
      vx[i] = *reinterpret_cast<const u16x8_t*>(x + 8 * iv);
      if (add) va[i] = *reinterpret_cast<const u16x8_t*>(add + 8 * iv);
    }
  }
  float s[kLnGroupVecs][8];
  float tot = 0.f;
#pragma unroll
  for (int i = 0; i < kLnGroupVecs; ++i) {
    const int iv = sub + LPR * i;
    if (live && iv < nv) {
      u16x8_t vb = {}, vs;
      if (bias) vb = *reinterpret_cast<const u16x8_t*>(bias + 8 * iv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = ld16<F16>(vx[i][j]);
        if (add) t += ld16<F16>(va[i][j]);
        if (bias) t += ld16<F16>(vb[j]);
        vs[j] = st16<F16>(t);
        // the statistics and y come from the rounded sum, as in layer_norm_kernel
        s[i][j] = ld16<F16>(vs[j]);
        tot += s[i][j];
      }
      if (sum_out) *reinterpret_cast<u16x8_t*>(sum_out + 8 * iv) = vs;
    }
  }
  const float inv_c = 1.f / (float)a.channels;
  const float mean = group_sum<LPR>(tot) * inv_c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kLnGroupVecs; ++i)
    if (live && sub + LPR * i < nv) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = s[i][j] - mean;
        q += d * d;
      }
    }
  const float rstd = 1.f / sqrtf(group_sum<LPR>(q) * inv_c + a.eps);
  const uint16_t* const gamma = static_cast<const uint16_t*>(a.gamma);
  const uint16_t* const beta = static_cast<const uint16_t*>(a.beta);
  uint16_t* const y = static_cast<uint16_t*>(a.y) + base;
#pragma unroll
  for (int i = 0; i < kLnGroupVecs; ++i) {
    const int iv = sub + LPR * i;
    if (live && iv < nv) {
      const u16x8_t vg = *reinterpret_cast<const u16x8_t*>(gamma + 8 * iv);
      const u16x8_t vb = *reinterpret_cast<const u16x8_t*>(beta + 8 * iv);
      u16x8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = st16<F16>((s[i][j] - mean) * rstd * ld16<F16>(vg[j]) + ld16<F16>(vb[j]));
      *reinterpret_cast<u16x8_t*>(y + 8 * iv) = o;
    }
  }
}

template <bool F16, int LPR>
void launch_layer_norm_grouped(const p2p_layer_norm_args& a, hipStream_t st) {
  constexpr int kRows = kLnGroupedThreads / LPR;
  const dim3 grid((unsigned)((a.rows + kRows - 1) / kRows)), block(kLnGroupedThreads);
  launch_kernel((layer_norm_grouped_kernel<F16, LPR>), grid, block, 0, st, a);
}

// out[m, j] = act(h), h = in[m, j] + bias[j]; act: h * sigmoid(1.702 h), or (ERF) the exact GELU
// 0.5 h (1 + erf(h / sqrt 2)) as geglu_kernel (p2p_unet.hip) writes it
template <bool F16, bool ERF>
__global__ __launch_bounds__(256) void bias_act_kernel(p2p_bias_act_args a, int64_t n_vec) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int dv = a.d >> 3;
  const int64_t m = iv / dv;
  const int j = (int)(iv - m * dv) * 8;
  const u16x8_t vi = *reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.in) + m * a.in_row_stride + j);
  const u16x8_t vb = *reinterpret_cast<const u16x8_t*>(static_cast<const uint16_t*>(a.bias) + j);
  u16x8_t o;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float h = ld16<F16>(vi[i]) + ld16<F16>(vb[i]);
    if (ERF) o[i] = st16<F16>(0.5f * h * (1.f + erff(h * 0.70710678118654752f)));
    else o[i] = st16<F16>(h / (1.f + __expf(-1.702f * h)));
  }
  *reinterpret_cast<u16x8_t*>(static_cast<uint16_t*>(a.out) + m * a.out_row_stride + j) = o;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool io16(int dtype) { return dtype == P2P_DTYPE_BF16 || dtype == P2P_DTYPE_F16; }

}  // namespace

int run_text_attn(const TextAttnArgs& a, bool causal, int io_dtype, hipStream_t st) {
  const dim3 grid((unsigned)(a.N * a.H)), block(64 * kCausalWaves);
  if (io_dtype != P2P_DTYPE_F16 && io_dtype != P2P_DTYPE_BF16) return P2P_E_DTYPE;
  const bool f16 = io_dtype == P2P_DTYPE_F16;
  if (causal && f16) launch_kernel((text_attn_kernel<true, f16_t, QkF16, MmaF16>), grid, block, 0, st, a);
  else if (causal) launch_kernel((text_attn_kernel<true, uint16_t, QkBf16<uint16_t>, MmaBf16>), grid, block, 0, st, a);
  else if (f16) launch_kernel((text_attn_kernel<false, f16_t, QkF16, MmaF16>), grid, block, 0, st, a);
  else launch_kernel((text_attn_kernel<false, uint16_t, QkBf16<uint16_t>, MmaBf16>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

int run_layer_norm(const p2p_layer_norm_args& a, hipStream_t st) {
  if (!a.x || !a.gamma || !a.beta || !a.y) return P2P_E_ARG;
  if (a.rows < 1 || a.channels < 1) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.channels % 8) return P2P_E_ALIGN;
  if (a.channels > kLnMaxChannels) return P2P_E_ARG;
  if (!aligned16(a.x) || !aligned16(a.add) || !aligned16(a.add_bias) || !aligned16(a.gamma) || !aligned16(a.beta) ||
      !aligned16(a.sum_out) || !aligned16(a.y))
    return P2P_E_ALIGN;
  const bool f16 = a.dtype == P2P_DTYPE_F16;
  // the row mapping is a function of the width and of whether there is an `add` (so are a row's
  // bits): the plain norm takes 8 lanes per row up to 320 channels and 16 up to 640 -- measured 11 %
  // and 3 % faster there than a wave per row; with an add a wave already has two operands in flight
  // and the grouped form measured 1.5-5 % slower, so every add, and every width above 640 (all the
  // text encoders'), keeps a wave per row
  const bool grouped = !a.add && a.channels <= kLnGroupedMaxChannels;
  if (grouped && a.channels <= kLnGroupedMaxChannels / 2) {
    if (f16) launch_layer_norm_grouped<true, 8>(a, st);
    else launch_layer_norm_grouped<false, 8>(a, st);
  } else if (grouped) {
    if (f16) launch_layer_norm_grouped<true, 16>(a, st);
    else launch_layer_norm_grouped<false, 16>(a, st);
  } else {
    const dim3 grid((unsigned)((a.rows + kLnRowsPerBlock - 1) / kLnRowsPerBlock)), block(64 * kLnRowsPerBlock);
    if (f16) launch_kernel(layer_norm_kernel<true>, grid, block, 0, st, a);
    else launch_kernel(layer_norm_kernel<false>, grid, block, 0, st, a);
  }
  return (int)hipGetLastError();
}

int run_bias_act(const p2p_bias_act_args& a, bool erf, hipStream_t st) {
  if (!a.in || !a.bias || !a.out) return P2P_E_ARG;
  if (a.rows < 1 || a.d < 1 || a.in_row_stride < a.d || a.out_row_stride < a.d) return P2P_E_ARG;
  if (!io16(a.dtype)) return P2P_E_DTYPE;
  if (a.d % 8 || a.in_row_stride % 8 || a.out_row_stride % 8) return P2P_E_ALIGN;
  if (!aligned16(a.in) || !aligned16(a.bias) || !aligned16(a.out)) return P2P_E_ALIGN;
  const int64_t n_vec = (int64_t)a.rows * (a.d / 8);
  if ((n_vec + 255) / 256 > INT32_MAX) return P2P_E_ARG;
  const dim3 grid((unsigned)((n_vec + 255) / 256));
  if (erf && a.dtype == P2P_DTYPE_F16) launch_kernel((bias_act_kernel<true, true>), grid, dim3(256), 0, st, a, n_vec);
  else if (erf) launch_kernel((bias_act_kernel<false, true>), grid, dim3(256), 0, st, a, n_vec);
  else if (a.dtype == P2P_DTYPE_F16) launch_kernel((bias_act_kernel<true, false>), grid, dim3(256), 0, st, a, n_vec);
  else launch_kernel((bias_act_kernel<false, false>), grid, dim3(256), 0, st, a, n_vec);
  return (int)hipGetLastError();
}

}  // namespace p2p
