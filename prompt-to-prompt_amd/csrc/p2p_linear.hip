// linear_kernel: y = epilogue(x[M, K] . W[N, K]^T), the transformer blocks' feed-forward GEMMs on the
// tile loop of conv3x3_kernel (p2p_mma_tile.h).  A linear layer is that loop with one
// tap and no halo: x is token-major (a row's K run is contiguous, rows may be strided) and
// nn.Linear's own [N, K] weight is already the K-major image the loop stages, so nothing is packed.
//
// A workgroup of four waves owns 128 rows x BN staged weight rows (BN = 128 or 160).  Epilogues, all
// from the f32 accumulators with one rounding, all stored token-major in 16-byte pieces through an
// LDS image of the tile:
//   BIAS      acc + bias[n] (bias nullable);
//   GEGLU     W is [2 D, K]: the staged rows of a tile are mapped so that each wave holds, for its 32
//             output columns, the two h fragments and the two matching gate fragments (b_off[] is
//             per staged row anyway), so out[m, j] = (acc_h + b[j]) * gelu(acc_g + b[D + j]) is
//             lane-local; a tile writes 64 output columns.  GEGLU_P also stores the rounded
//             pre-activation acc + b as p_out [M, 2 D] (for the backward); out's bits are the same;
//   RESIDUAL  acc + bias[n] + res[m, n]: the res tile is loaded coalesced into the epilogue's LDS
//             image, each lane adds its elements in f32 and writes the rounded value back in place;
//   PARTIAL   (K split, small M) the f32 partial of this block's K range, column-major
//             [split][N][Mp] (Mp = M rounded up to the tile: the accumulator's four rows are one
//             aligned 16-byte store and no row needs a guard); linear_reduce_kernel sums the
//             partials in split order, adds bias and residual, rounds and writes token-major: no
//             atomics, the same bits on every launch.
#include <type_traits>

#include "p2p_mma_tile.h"

namespace p2p {
namespace {

enum { EPI_BIAS = 0, EPI_GEGLU, EPI_GEGLU_P, EPI_RESIDUAL, EPI_PARTIAL };

struct LinearArgs {
  const uint16_t* x;     // [M, K], row stride x_stride
  const uint16_t* w;     // [N, K] dense; GEGLU: [2 N, K]
  const uint16_t* bias;  // [N] (GEGLU: [2 N]) or null
  const uint16_t* res;   // RESIDUAL: [M, N], row stride res_stride
  void* y;               // [M, N] 16-bit dense, or the f32 partials [split][N][Mp]
  uint16_t* p_out;       // GEGLU_P: [M, 2 N] dense
  int M, K, N;           // N: output columns (GEGLU: D)
  int x_stride, res_stride;
  int m_tiles, n_tiles, split;
};

template <bool F16>
__device__ __forceinline__ uint16_t cvt16(float v) {
  if constexpr (F16) return f2h(v);
  else return f2bf(v);
}
template <bool F16>
__device__ __forceinline__ float ld16f(uint16_t v) {
  if constexpr (F16) return h2f(v);
  else return bf2f(v);
}

template <bool F16, int BK, int NF, int EPI>
__global__ __launch_bounds__(kConvThreads) void linear_kernel(LinearArgs a) {
  constexpr bool GEGLU = EPI == EPI_GEGLU || EPI == EPI_GEGLU_P;
  static_assert(!GEGLU || NF % 2 == 0, "a wave's fragments are half h, half gate");
  constexpr int BM = kConvBM, BN = 32 * NF;
  constexpr int OC = GEGLU ? BN / 2 : BN;     // output columns of a tile
  constexpr int CPR = BK / 8;                 // 16-byte chunks per staged row
  constexpr int RPP = kConvThreads / CPR;     // rows per staging pass
  constexpr int NA = BM / RPP, NB = BN / RPP;
  static_assert(BM % RPP == 0 && BN % RPP == 0, "staging passes cover the tiles exactly");
  constexpr int P = (EPI == EPI_GEGLU ? OC : BN) + 8;   // 16-bit elements per row of the epilogue's tile image
  constexpr int kStage = (BM + BN) * BK * 2;
  constexpr int kEpi = EPI == EPI_PARTIAL ? 0 : BM * P * 2;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kStage > kEpi ? kStage : kEpi];
  unsigned char* const ldsA = lds;
  unsigned char* const ldsB = lds + BM * BK * 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles = a.m_tiles * a.n_tiles;
  int bid = blockIdx.x;
  const int split = bid / tiles;          // slowest: a split's tiles are dispatched together
  bid = xcd_remap(bid - split * tiles, tiles);
  const int m0 = (bid / a.n_tiles) * BM, n0 = (bid % a.n_tiles) * OC;

  const int steps = a.K / BK;
  const int t_begin = (int)((int64_t)steps * split / a.split), t_end = (int)((int64_t)steps * (split + 1) / a.split);

  // staging roles: chunk sc of rows sr + RPP i
  const int sc = tid % CPR, sr = tid / CPR;
  int a_off[NA], a_lds[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int r = sr + RPP * i;
    a_off[i] = min(m0 + r, a.M - 1) * a.x_stride + sc * 8;   // rows past M repeat the last one; never stored
    a_lds[i] = lds_chunk<BK>(r, sc);
  }
  int b_off[NB], b_lds[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int r = sr + RPP * i;
    int row;
    if constexpr (GEGLU) {   // staged row r = (wave column, fragment j, lane row): j < NF / 2 an h row, else its gate row
      const int j = (r >> 4) % NF;
      const int c = (r / (16 * NF)) * (8 * NF) + (j % (NF / 2)) * 16 + (r & 15);
      row = min(n0 + c, a.N - 1) + (j >= NF / 2 ? a.N : 0);
    } else {
      row = min(n0 + r, a.N - 1);              // rows past N repeat the last one; never stored
    }
    b_off[i] = row * a.K + sc * 8;
    b_lds[i] = lds_chunk<BK>(r, sc);
  }

  u32x4_t ra[NA], rb[NB];
  auto load_step = [&](int t) {
    const int c0 = t * BK;
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = *reinterpret_cast<const u32x4_t*>(a.x + (a_off[i] + c0));
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[i] = *reinterpret_cast<const u32x4_t*>(a.w + (b_off[i] + c0));
  };
  auto write_step = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) *reinterpret_cast<u32x4_t*>(ldsA + a_lds[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<u32x4_t*>(ldsB + b_lds[i]) = rb[i];
  };

  P2P_MMA_TILE_LOOP(t_begin, t_end)

  // acc[i][j][e]: row m0 + wm 64 + i 16 + fq 4 + e, staged weight row wn 16 NF + j 16 + fr
  if constexpr (EPI == EPI_PARTIAL) {
    const int64_t Mp = (int64_t)a.m_tiles * BM;
    float* const ws = reinterpret_cast<float*>(a.y) + (int64_t)split * a.N * Mp;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int n = n0 + wn * (16 * NF) + j * 16 + fr;
      if (n >= a.N) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<f32x4_t*>(ws + n * Mp + (m0 + wm * 64 + i * 16 + fq * 4)) = acc[i][j];
    }
  } else {
    // (the loop's last barrier stands behind every fragment read: the staging image may be reused)
    uint16_t* const tile = reinterpret_cast<uint16_t*>(lds);
    // the 16-byte pieces of the tile's first W columns, row by row: f(tile piece, row m, tile column c)
    auto for_pieces = [&](auto W, auto&& f) {
      constexpr int PPR = decltype(W)::value / 8;
      for (int p = tid; p < BM * PPR; p += kConvThreads) {
        const int r = p / PPR, c = (p - r * PPR) * 8;
        if (m0 + r < a.M) f(reinterpret_cast<u32x4_t*>(tile + r * P + c), m0 + r, c);
      }
    };
    auto store_out = [&]() {
      uint16_t* const y = reinterpret_cast<uint16_t*>(a.y);
      for_pieces(std::integral_constant<int, OC>{}, [&](u32x4_t* piece, int m, int c) {
        if (n0 + c < a.N) *reinterpret_cast<u32x4_t*>(y + (int64_t)m * a.N + n0 + c) = *piece;   // (N % 8 == 0)
      });
    };
    const int row0 = wm * 64 + fq * 4;

    if constexpr (GEGLU) {
      float bh[NF / 2], bg[NF / 2];
#pragma unroll
      for (int j = 0; j < NF / 2; ++j) {
        const int n = n0 + wn * (8 * NF) + j * 16 + fr;
        const bool ok = a.bias && n < a.N;
        bh[j] = ok ? ld16f<F16>(a.bias[n]) : 0.f;
        bg[j] = ok ? ld16f<F16>(a.bias[a.N + n]) : 0.f;
      }
      if constexpr (EPI == EPI_GEGLU_P) {   // the rounded pre-activation: h columns in the image's first half, gates in the second
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            const int c = (j >= NF / 2 ? OC : 0) + wn * (8 * NF) + (j % (NF / 2)) * 16 + fr;
            const float b = j >= NF / 2 ? bg[j % (NF / 2)] : bh[j % (NF / 2)];
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(row0 + i * 16 + e) * P + c] = cvt16<F16>(acc[i][j][e] + b);
          }
        __syncthreads();
        for_pieces(std::integral_constant<int, BN>{}, [&](u32x4_t* piece, int m, int c) {
          const int half = c / OC, n = n0 + c - half * OC;
          if (n < a.N) *reinterpret_cast<u32x4_t*>(a.p_out + (int64_t)m * (2 * a.N) + half * a.N + n) = *piece;
        });
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF / 2; ++j) {
          const int c = wn * (8 * NF) + j * 16 + fr;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float h = acc[i][j][e] + bh[j], gate = acc[i][j + NF / 2][e] + bg[j];
            const float gelu = 0.5f * gate * (1.f + erff(gate * 0.70710678118654752f));
            tile[(row0 + i * 16 + e) * P + c] = cvt16<F16>(h * gelu);
          }
        }
    } else {
      if constexpr (EPI == EPI_RESIDUAL) {
        for_pieces(std::integral_constant<int, BN>{}, [&](u32x4_t* piece, int m, int c) {
          if (n0 + c < a.N) *piece = *reinterpret_cast<const u32x4_t*>(a.res + (int64_t)m * a.res_stride + n0 + c);
        });
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int c = wn * (16 * NF) + j * 16 + fr;
        const float b = (a.bias && n0 + c < a.N) ? ld16f<F16>(a.bias[n0 + c]) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            uint16_t* const t = tile + (row0 + i * 16 + e) * P + c;
            float v = acc[i][j][e] + b;
            if constexpr (EPI == EPI_RESIDUAL) v += ld16f<F16>(*t);   // (past M or N: whatever the image held; never stored)
            *t = cvt16<F16>(v);
          }
      }
    }
    __syncthreads();
    store_out();
  }
}

// y[m, n] = round(sum over the splits, in split order, of ws[s][n][m], + bias[n] + res[m, n]): a
// 64 x 64 tile read along m, transposed through LDS and stored in 16-byte pieces along n
template <bool F16>
__global__ __launch_bounds__(256) void linear_reduce_kernel(const float* ws, uint16_t* y, const uint16_t* bias,
                                                            const uint16_t* res, int M, int N, int Mp, int res_stride,
                                                            int split) {
  __shared__ float tile[64][65];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  const int64_t slab = (int64_t)N * Mp;
  const int mi = tid & 63;
#pragma unroll 4
  for (int q = 0; q < 16; ++q) {
    const int n = (tid >> 6) + 4 * q;
    float s = 0.f;
    if (n0 + n < N) {
      const float* p = ws + (int64_t)(n0 + n) * Mp + m0 + mi;   // (m0 + mi < Mp: Mp is a multiple of the 128-row tile)
      s = p[0];
      for (int k = 1; k < split; ++k) s += p[k * slab];
    }
    tile[n][mi] = s;
  }
  __syncthreads();
  const int r = tid >> 2, m = m0 + r;
  if (m >= M) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = ((tid & 3) + 4 * h) * 8, n = n0 + c;
    if (n >= N) continue;   // (N % 8 == 0: a piece stands or falls together)
    u32x4_t rv = {0u, 0u, 0u, 0u};
    if (res) rv = *reinterpret_cast<const u32x4_t*>(res + (int64_t)m * res_stride + n);
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = tile[c + k][r];
      if (bias) v[k] += ld16f<F16>(bias[n + k]);
      if (res) v[k] += ld16f<F16>((uint16_t)(rv[k >> 1] >> (16 * (k & 1))));
    }
    const u32x4_t o = {pack2<F16>(v[0], v[1]), pack2<F16>(v[2], v[3]), pack2<F16>(v[4], v[5]), pack2<F16>(v[6], v[7])};
    *reinterpret_cast<u32x4_t*>(y + (int64_t)m * N + n) = o;
  }
}

template <bool F16, int BK, int NF>
void launch_linear_tile(const LinearArgs& a, int form, hipStream_t st) {
  const dim3 grid((unsigned)(a.m_tiles * a.n_tiles * a.split)), block(kConvThreads);
  if (a.split > 1) launch_kernel((linear_kernel<F16, BK, NF, EPI_PARTIAL>), grid, block, 0, st, a);
  else if (form == P2P_LINEAR_RESIDUAL) launch_kernel((linear_kernel<F16, BK, NF, EPI_RESIDUAL>), grid, block, 0, st, a);
  else launch_kernel((linear_kernel<F16, BK, NF, EPI_BIAS>), grid, block, 0, st, a);
}

template <bool F16, int BK>
void launch_linear_geglu(const LinearArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.m_tiles * a.n_tiles)), block(kConvThreads);
  if (a.p_out) launch_kernel((linear_kernel<F16, BK, 4, EPI_GEGLU_P>), grid, block, 0, st, a);
  else launch_kernel((linear_kernel<F16, BK, 4, EPI_GEGLU>), grid, block, 0, st, a);
}

template <bool F16>
void launch_linear_dtype(const LinearArgs& a, int form, const LinearPlan& plan, void* y, hipStream_t st) {
  if (form == P2P_LINEAR_GEGLU) {
    if (plan.bk == 64) launch_linear_geglu<F16, 64>(a, st);
    else launch_linear_geglu<F16, 32>(a, st);
  } else if (plan.bk == 64 && plan.bn == 160) {
    launch_linear_tile<F16, 64, 5>(a, form, st);
  } else if (plan.bk == 64) {
    launch_linear_tile<F16, 64, 4>(a, form, st);
  } else {
    launch_linear_tile<F16, 32, 4>(a, form, st);
  }
  if (plan.split > 1) {
    const int Mp = a.m_tiles * kConvBM;
    const dim3 grid((unsigned)(Mp / 64), (unsigned)((a.N + 63) / 64));
    launch_kernel(linear_reduce_kernel<F16>, grid, dim3(256), 0, st, (const float*)a.y, (uint16_t*)y, a.bias, a.res,
                  a.M, a.N, Mp, a.res_stride, plan.split);
  }
}

}  // namespace

// the launcher: run_linear (p2p_dispatch.hip) has checked the arguments and chosen the plan
int launch_linear(const p2p_linear_args& a, const LinearPlan& plan, hipStream_t st) {
  LinearArgs k;
  k.x = (const uint16_t*)a.x;
  k.w = (const uint16_t*)a.weight;
  k.bias = (const uint16_t*)a.bias;
  k.res = a.form == P2P_LINEAR_RESIDUAL ? (const uint16_t*)a.res : nullptr;
  k.p_out = a.form == P2P_LINEAR_GEGLU ? (uint16_t*)a.p_out : nullptr;
  k.M = a.m, k.K = a.k, k.N = a.n;
  k.x_stride = (int)a.x_row_stride, k.res_stride = (int)a.res_row_stride;
  k.m_tiles = (a.m + kConvBM - 1) / kConvBM;
  k.n_tiles = (a.n + linear_tile_cols(a.form, plan) - 1) / linear_tile_cols(a.form, plan);
  k.split = plan.split;
  k.y = plan.split > 1 ? (void*)a.workspace : a.y;
  if (a.dtype == P2P_DTYPE_F16) launch_linear_dtype<true>(k, a.form, plan, a.y, st);
  else launch_linear_dtype<false>(k, a.form, plan, a.y, st);
  return (int)hipGetLastError();
}

}  // namespace p2p
