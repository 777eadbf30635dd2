// The 128-row MFMA tile loop that conv3x3_kernel (p2p_conv.hip) and linear_kernel (p2p_linear.hip)
// share: four waves (2 x 2) own a 128 x 32 NF tile of
// v_mfma_f32_16x16x32_{bf16,f16} fragments; both operands are staged through registers into one
// XOR-swizzled LDS image per K step -- the loads of step t + 1 are issued before the MFMAs of step t
// and written after them, two barriers per step.  Where a staged row comes from is the kernel's own
// business: it hands the loop a load_step(t) that fills its staging registers and a write_step()
// that puts them into the image.
#pragma once

#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {
namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

constexpr int kConvThreads = 256;

template <bool F16>
__device__ __forceinline__ float conv_bias(const uint16_t* bias, int co) {
  if constexpr (F16) return h2f(bias[co]);
  else return bf2f(bias[co]);
}

template <bool F16>
__device__ __forceinline__ f32x4_t mma16(const u32x4_t& a, const u32x4_t& b, const f32x4_t& c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0,
                                                   0);
}

template <bool F16>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  if constexpr (F16) return (uint32_t)f2h(lo) | ((uint32_t)f2h(hi) << 16);
  else return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}

// byte offset of 16-byte chunk c of row r in a staged image with BK 16-bit elements per row: the
// chunk index is XORed with the row so that the 16 rows one fragment read touches spread over the
// banks (two rows per bank group instead of eight or sixteen)
template <int BK>
__device__ __forceinline__ int lds_chunk(int r, int c) {
  constexpr int CPR = BK / 8;
  const int s = BK == 64 ? (r & 7) : ((r >> 1) & 3);
  return r * (BK * 2) + ((c ^ s) & (CPR - 1)) * 16;
}

// K steps [t_begin, t_end) of one tile into acc: acc[i][j][e] is row wm 64 + i 16 + (lane >> 4) 4 + e,
// column wn 16 NF + j 16 + (lane & 15) of the tile.  The last barrier stands behind every fragment
// read, so the caller may reuse the staging image at once.
// P2P_MMA_TILE_LOOP: written as a macro, not a function -- with the loop in a function template that takes
// the two steps as callables, hipcc's register allocation of conv3x3_kernel came out different (146
// against 148 VGPRs and other instruction lines); expanded in place the 26 instantiations are the
// code they were.  Expects in scope: F16, BK, NF, ldsA, ldsB, wm, wn, lane, load_step(t), write_step();
// defines acc, fr, fq.
#define P2P_MMA_TILE_LOOP(t_begin, t_end)                                                                              \
  f32x4_t acc[4][NF];                                                                                                  \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                        \
      _Pragma("unroll") for (int j = 0; j < NF; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};                           \
                                                                                                                       \
  const int fr = lane & 15, fq = lane >> 4;                                                                            \
  load_step(t_begin);                                                                                                  \
  write_step();                                                                                                        \
  __syncthreads();                                                                                                     \
  for (int t = t_begin; t < t_end; ++t) {                                                                              \
    const bool more = t + 1 < t_end;                                                                                   \
    if (more) load_step(t + 1);                                                                                        \
    _Pragma("unroll") for (int kk = 0; kk < BK / 32; ++kk) {                                                           \
      u32x4_t fa[4], fb[NF];                                                                                           \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) fa[i] =                                                            \
          *reinterpret_cast<const u32x4_t*>(ldsA + lds_chunk<BK>(wm * 64 + i * 16 + fr, kk * 4 + fq));                 \
      _Pragma("unroll") for (int j = 0; j < NF; ++j) fb[j] =                                                           \
          *reinterpret_cast<const u32x4_t*>(ldsB + lds_chunk<BK>(wn * (16 * NF) + j * 16 + fr, kk * 4 + fq));          \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                    \
          _Pragma("unroll") for (int j = 0; j < NF; ++j) acc[i][j] = mma16<F16>(fa[i], fb[j], acc[i][j]);              \
    }                                                                                                                  \
    __syncthreads();                                                                                                   \
    if (more) {                                                                                                        \
      write_step();                                                                                                    \
      __syncthreads();                                                                                                 \
    }                                                                                                                  \
  }

}  // namespace
}  // namespace p2p
