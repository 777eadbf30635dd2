// Self-attention for one wide head (d = 512): the mid-block attention of the SD VAE, one head of
// 512 channels over up to 4096 tokens.  O = softmax(scale Q K^T) V, bf16 or fp16 tensors with the
// MFMA of that type, f32 softmax statistics, O in the input type; no kept maps, no lse.
//
// A 32-query x 512 f32 accumulator does not fit one wave beside its operands, so the four waves of
// a workgroup (32 queries) split the work twice, in the transposed-fragment convention of
// p2p_device.h (S^T = K Q^T, O^T = V^T P^T, query on the lane):
//   * Q K^T of a 64-key tile: wave w takes key block w & 1 (32 keys) and the half w >> 1 of d
//     (256 columns, 16 MFMAs).  Its Q half stays in registers (64); its K fragments come from a
//     row-major LDS image of the tile.
//   * the four partial 32 x 32 f32 blocks are exchanged through LDS (16 KB); every wave then adds
//     the two d-halves of both key blocks in the same order and runs the same online softmax on all
//     64 keys, so all four hold identical row statistics and the same P in the S^T register layout,
//     which is the B operand of the P V MFMA as it stands (no second exchange of P);
//   * P V: wave w owns O columns [128 w, 128 w + 128) (64 accumulator registers, 16 MFMAs per
//     tile) and reads V^T from a row-major LDS image of the tile with transposing reads.
// LDS: one K tile of 64 x 520 16-bit elements (row stride 16 x 65 bytes for the 16-byte fragment
// reads: 66,560 B), one V tile of 64 x 544 (row stride 272 dwords = 16 mod 64 for the transposing
// reads: 69,632 B) and the 16 KB exchange = 152,576 B of the CU's 160 KiB: a 64-key tile of K and V
// at d = 512 is 64 KB each, so there is no room for a second buffer of either.  The next tile is
// instead held in registers (128 per lane, loaded at the top of a tile with 1 KB-contiguous rows
// per wave instruction) and written into the images as soon as the tile's readers are through: K
// behind the barrier that follows Q K^T, V behind the one that follows P V -- two barriers per tile.
// Its bound (profiles/r09/vae/wide_probe.txt): every workgroup streams all of K and V
// through its CU, 128 KB per tile, and one CU fills at about 38 GB/s whatever the others do -- 3.4 us
// per 64-key tile against 0.43 us of MFMA, with 1 workgroup or 256 in flight.  (A first form that
// read each wave's K fragments straight from global memory, 32 rows x 32 bytes per instruction,
// took the same 216-218 us at 4096 x 4096 x 512.)  Shortening the chain needs the keys split over
// workgroups and a combine pass with a workspace, which p2p_self_attn_fwd does not have.
// Every reduction runs in a fixed order: two launches on one input give the same bits.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {

namespace {

constexpr int kWideD = 512;
constexpr int kWideBK = 64;                      // keys per tile
constexpr int kWideVS = kWideD + 32;             // V image row stride (elements): 272 dwords
constexpr int kWideKS = KStride<kWideD, 2>::value;   // K image row stride (elements): 16 x odd bytes
constexpr int kWideKBytes = kWideBK * kWideKS * 2;
constexpr int kWideVBytes = kWideBK * kWideVS * 2;
constexpr int kWideXchg = 4 * 16 * 64;           // exchange floats: [wave][4 reg groups][64 lanes][4]
constexpr int kWideLds = kWideKBytes + kWideVBytes + kWideXchg * 4;
static_assert(kWideLds <= 160 * 1024, "the K and V images and the exchange must fit the CU's LDS");
static_assert(kWideKBytes % 16 == 0 && kWideVBytes % 16 == 0, "16-byte aligned LDS regions");
static_assert((kWideVS / 2) % 64 == 16, "bank rule of the transposing V reads (VStrideBf16)");

template <typename IO, typename MQ, typename MP>
__global__ __launch_bounds__(256) void self_wide_kernel(SelfArgs a) {
  using EK = typename MQ::elem;
  using EV = typename MP::elem;
  constexpr int D = kWideD, BK = kWideBK, VS = kWideVS, KS = kWideKS;
  constexpr int NT = 256;
  constexpr int NKT = D / 2 / 16;                // k steps of one wave's d half
  constexpr int NDT = D / 4 / 32;                // O^T tiles of one wave's 128 columns
  constexpr int CPR = D / 8;                     // 16-byte chunks per K / V row
  constexpr int NCH = BK * CPR / NT;             // K (and V) chunks per thread and tile
  static_assert(BK * CPR % NT == 0, "whole chunk slots");
  __shared__ __attribute__((aligned(16))) char smem[kWideLds];
  EK* const Ks = reinterpret_cast<EK*>(smem);
  EV* const Vs = reinterpret_cast<EV*>(smem + kWideKBytes);
  float* const xch = reinterpret_cast<float*>(smem + kWideKBytes + kWideVBytes);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int hh = lane >> 5;
  const int qi = lane & 31;
  const int kb = wave & 1;                       // key block of the Q K^T share
  const int dh = wave >> 1;                      // d half of the Q K^T share

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = logical % a.n_qtiles;
  const int nh = logical / a.n_qtiles;
  const int h = nh % a.H;
  const int n = nh / a.H;
  const int src = a.qk_src[n];
  const int p = qt * 32 + qi;
  const bool prow = p < a.P;
  const int K = a.K;
  const float c = a.scale_log2;

  const IO* const qp = static_cast<const IO*>(a.q) + (int64_t)src * a.bsq + h * D;
  const IO* const kp = static_cast<const IO*>(a.k) + (int64_t)src * a.bsk + h * D;
  const IO* const vp = static_cast<const IO*>(a.v) + (int64_t)n * a.bsv + h * D;

  typename MQ::frag qf[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t)
    qf[t] = prow ? MQ::load_q(qp + (int64_t)p * a.ldq + dh * (D / 2) + 16 * t + 8 * hh) : MQ::zero();

  // K and V tiles through range-checked buffer loads: the descriptor spans the rows [tile start,
  // K) of this (entry, head), so rows past K read as zeros (their logits are masked below, and a
  // zero V row keeps 0 * V finite) and the per-lane byte offsets are loop-invariant.  Chunk c of a
  // tile is row c / 64, columns 8 (c % 64) ..: a wave instruction reads one whole 1 KB row.
  uint32_t koff[NCH], voff[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int cidx = tid + i * NT;
    koff[i] = (uint32_t)(((cidx / CPR) * (int)a.ldk + (cidx % CPR) * 8) * (int)sizeof(IO));
    voff[i] = (uint32_t)(((cidx / CPR) * (int)a.ldv + (cidx % CPR) * 8) * (int)sizeof(IO));
  }
  const int64_t kbytes = ((int64_t)(K - 1) * a.ldk + D) * (int64_t)sizeof(IO);
  const int64_t vbytes = ((int64_t)(K - 1) * a.ldv + D) * (int64_t)sizeof(IO);
  const int64_t kstep = (int64_t)BK * a.ldk * (int64_t)sizeof(IO);
  const int64_t vstep = (int64_t)BK * a.ldv * (int64_t)sizeof(IO);

  Chunk8<IO> kreg[NCH], vreg[NCH];
  auto load_kv = [&](int kt) {
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(reinterpret_cast<const char*>(kp) + kt * kstep, kbytes - kt * kstep);
    const __amdgpu_buffer_rsrc_t rv = make_rsrc(reinterpret_cast<const char*>(vp) + kt * vstep, vbytes - kt * vstep);
#pragma unroll
    for (int i = 0; i < NCH; ++i) kreg[i].load_buf(rk, koff[i]);
#pragma unroll
    for (int i = 0; i < NCH; ++i) vreg[i].load_buf(rv, voff[i]);
  };
  auto write_k = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      MQ::stage(kreg[i], Ks + (cidx / CPR) * KS + (cidx % CPR) * 8, 0);
    }
  };
  auto write_v = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + i * NT;
      vreg[i].store(Vs + (cidx / CPR) * VS + (cidx % CPR) * 8);
    }
  };

  const int ntiles = (K + BK - 1) / BK;
  f32x16_t O[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) O[dt] = f32x16_t{};
  float m_run = -INFINITY;   // running row max, log2 domain, scale folded
  float l_run = 0.f;         // this lane's share of the row sum (its half of every 32-key block)

  load_kv(0);
  write_k();
  write_v();
  __syncthreads();
  const EK* const Kw = Ks + (kb * 32 + qi) * KS + dh * (D / 2) + 8 * hh;   // this lane's K fragments
  const EV* const Vw = Vs + wave * (D / 4);                                // this wave's V columns
  for (int kt = 0; kt < ntiles; ++kt) {
    const bool more = kt + 1 < ntiles;
    if (more) load_kv(kt + 1);
    // this wave's share of S^T: 32 keys x 32 queries over 256 columns of d
    f32x16_t acc = {};
#pragma unroll
    for (int t = 0; t < NKT; ++t) MQ::mma(acc, MQ::load_k(Kw + 16 * t, 0), qf[t]);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4_t*>(xch + ((wave * 4 + g) * 64 + lane) * 4) =
          f32x4_t{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    // every wave is through with the K image; the partial blocks are visible
    __syncthreads();
    // every wave: both key blocks, d halves added low + high
    float sv[2][16];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4_t lo = *reinterpret_cast<const f32x4_t*>(xch + ((sb * 4 + g) * 64 + lane) * 4);
        const f32x4_t hi = *reinterpret_cast<const f32x4_t*>(xch + (((2 + sb) * 4 + g) * 64 + lane) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[sb][4 * g + e] = lo[e] + hi[e];
      }
    if ((kt + 1) * BK > K) {   // the ragged last tile
#pragma unroll
      for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * BK + sb * 32 + acc_row(r, hh) >= K) sv[sb][r] = -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sv[sb][r]);
    mx = fmaxf(mx, other_half(mx)) * c;   // key 0 of tile 0 is always in range: finite from there on
    if (!__all(mx <= m_run)) {
      const float mnew = fmaxf(m_run, mx);
      const float alpha = fast_exp2(m_run - mnew);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dt][r] *= alpha;
      l_run *= alpha;
      m_run = mnew;
    }
    float ls = 0.f;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = fast_exp2(fmaf(sv[sb][r], c, -m_run));
        sv[sb][r] = e;
        ls += e;
      }
    l_run += ls;
    // the next tile's K into the image (read again only behind the next barrier)
    if (more) write_k();
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) pv_block<VS, NDT>(MP{}, O, Vw, sb * 32, sv[sb], lane);
    // every wave is through with the V image and the exchange
    __syncthreads();
    // the next tile's V: its readers wait behind the barrier after the next Q K^T
    if (more) write_v();
  }
  const float l = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.f / l;
  if (prow) {
    IO* const op = static_cast<IO*>(a.o) + (int64_t)n * a.bso + h * D + (int64_t)p * a.ldo + wave * (D / 4);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store4(op + dt * 32 + 8 * g + 4 * hh, O[dt][4 * g] * inv, O[dt][4 * g + 1] * inv, O[dt][4 * g + 2] * inv,
               O[dt][4 * g + 3] * inv);
  }
}

}  // namespace

int launch_self_wide(const SelfArgs& a, int prec, hipStream_t st) {
  SelfArgs b = a;
  b.n_qtiles = (a.P + 31) / 32;
  const int64_t wgs = (int64_t)b.n_qtiles * a.H * a.N;
  // the kernel's per-lane byte offsets inside a tile are 32-bit
  if (wgs > INT32_MAX || a.ldk > (1 << 20) || a.ldv > (1 << 20)) return P2P_E_ARG;
  const dim3 grid((unsigned)wgs), block(256);
  if (prec == PREC_BF16)
    launch_kernel((self_wide_kernel<uint16_t, QkBf16<uint16_t>, MmaBf16>), grid, block, 0, st, b);
  else if (prec == PREC_F16)
    launch_kernel((self_wide_kernel<f16_t, QkF16, MmaF16>), grid, block, 0, st, b);
  else
    return P2P_E_DTYPE;
  return (int)hipGetLastError();
}

}  // namespace p2p
