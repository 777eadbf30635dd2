// The pipelined MFMA tile loop of conv3x3_pipe_kernel (p2p_conv.hip): p2p_mma_tile.h's
// tile at BK = 64, BN = 160 with both operands brought global -> LDS by global_load_lds_dwordx4 into a
// ring of D stage images, no staging registers.  WM x 2 waves own a 64 WM-row x 160-column tile, each
// wave the 64 x 80 fragment block of P2P_MMA_TILE_LOOP, so every accumulator receives the MFMA
// sequence it receives there (t ascending, then kk): the bits are that loop's.
//
// One raw s_barrier per K step:
//   counted vmcnt: this wave's DMAs of stage t landed (up to D - 2 later stages stay in flight);
//   s_barrier:     so did every other wave's, and every wave's fragment reads of stage t - 1 retired
//                  (their MFMAs were issued before the wave arrived);
//   issue stage t + D - 1 into the slot stage t - 1 just left -- at once, or (LATE) between the two
//   halves of the step, where its address arithmetic runs in the shadow of the first half's MFMAs;
//   fragment reads of stage t, MFMAs.
// A stage is read only behind the issuing waves' counted wait and a barrier the reader has passed;
// no __syncthreads() stands where a DMA is in flight (its fence would drain the ring); every wave
// issues the same number of DMA instructions per stage, so one vmcnt constant serves all.
//
// The LDS image of a DMA is lane-linear -- one wave instruction writes 1024 consecutive bytes, 8 rows
// of 128 -- so the XOR swizzle of lds_chunk<64> is applied on the source side: lane l is (row l / 8,
// slot l % 8) of its 8 rows and fetches chunk slot ^ row of that row.  A row that must read as zeros
// (a tap outside the image, a row past M) points at kPipeZeros instead of at its pixel.
#pragma once

#include "p2p_mma_tile.h"

namespace p2p {
namespace {

// what a halo lane's DMA fetches
__device__ __attribute__((aligned(16))) const uint32_t kPipeZeros[4] = {0u, 0u, 0u, 0u};

// 16 bytes per lane from g to LDS byte lds_off + 16 lane (lds_off wave-uniform)
__device__ __forceinline__ void pipe_dma16(const void* g, uint32_t lds_off) {
  __builtin_amdgcn_global_load_lds(g, reinterpret_cast<__attribute__((address_space(3))) void*>((uintptr_t)lds_off), 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void pipe_wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is six bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// vmcnt(min(ahead, K) * P): the stage `ahead` stages behind the newest issued one has landed
template <int P, int K>
__device__ __forceinline__ void pipe_wait_stage(int ahead) {
  if constexpr (K == 0) {
    pipe_wait_vmcnt<0>();
  } else {
    if (ahead >= K) pipe_wait_vmcnt<K * P>();
    else pipe_wait_stage<P, K - 1>(ahead);
  }
}

// K steps [t_begin, t_end) into acc: acc[i][j][e] is row wm 64 + i 16 + (lane >> 4) 4 + e, column
// wn 80 + j 16 + (lane & 15) of the tile.  lds: the ring's byte offset in LDS and its generic pointer;
// a stage is kStage bytes, A's rows first, B's from kBOff.  issue(t, lds_off) starts this wave's P DMA
// instructions of step t into the stage at byte lds_off.  On return every DMA has landed; the
// caller puts a barrier before it reuses the ring.  LATE: the issue stands behind the MFMAs of kk = 0
// (measured per tile height, p2p_select.h).
template <bool F16, int D, int P, int kStage, int kBOff, bool LATE, class Issue>
__device__ __forceinline__ void mma_pipe_loop(f32x4_t (&acc)[4][5], const unsigned char* ring, uint32_t ring_off, int wm,
                                              int wn, int lane, int t_begin, int t_end, Issue&& issue) {
  static_assert(D >= 2 && (D - 2) * P < 64, "the ring's depth against vmcnt's range");
  constexpr int NF = 5;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int s = 0; s < D - 1; ++s)
    if (t_begin + s < t_end) issue(t_begin + s, ring_off + s * kStage);
  int rs = 0, ws = D - 1;     // the slot step t reads, the slot step t + D - 1 is written to
  for (int t = t_begin; t < t_end; ++t) {
    pipe_wait_stage<P, D - 2>(t_end - 1 - t);
    __builtin_amdgcn_s_barrier();
    if (!LATE && t + D - 1 < t_end) issue(t + D - 1, ring_off + ws * kStage);
    const unsigned char* const ldsA = ring + rs * kStage;
    const unsigned char* const ldsB = ldsA + kBOff;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      u32x4_t fa[4], fb[NF];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        fa[i] = *reinterpret_cast<const u32x4_t*>(ldsA + lds_chunk<64>(wm * 64 + i * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int j = 0; j < NF; ++j)
        fb[j] = *reinterpret_cast<const u32x4_t*>(ldsB + lds_chunk<64>(wn * (16 * NF) + j * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = mma16<F16>(fa[i], fb[j], acc[i][j]);
      if (LATE && kk == 0 && t + D - 1 < t_end) issue(t + D - 1, ring_off + ws * kStage);
    }
    rs = rs + 1 == D ? 0 : rs + 1;
    ws = ws + 1 == D ? 0 : ws + 1;
  }
}

}  // namespace
}  // namespace p2p
