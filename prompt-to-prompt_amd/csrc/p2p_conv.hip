// conv3x3_kernel: the U-Net's 3x3 convolutions as an implicit GEMM on v_mfma_f32_16x16x32_{bf16,f16}
// (DESIGN.md §4.16), in three addressing forms that share everything but where a tap reads:
//   Same   stride 1, padding 1 (the resnets);
//   Up2    the padded convolution of the nearest-neighbour 2x upsampling of x, which is never
//          written: tap (dy, dx) of output pixel (oy, ox) reads low-resolution pixel
//          ((oy + dy) >> 1, (ox + dx) >> 1) and is valid inside the 2h x 2w map (Upsample2D);
//   Down2  stride 2, padding 1, even h and w: tap (ky, kx) reads (2 oy + ky - 1, 2 ox + kx - 1) and is
//          valid where both are >= 0 (Downsample2D).
//
//   M = n h w output pixels (x is token-major: one pixel's channels are one contiguous K run),
//   N = c_out, K = 9 c_in walked tap by tap: one K step is one tap and BK channels.
//
// A workgroup of four waves (2 x 2) owns a 128-pixel x BN-channel tile (BN = 128 or 160 = 4 or 5
// 16-wide fragments per wave; every c_out of the U-Net is a multiple of 160).  Both operands are
// staged through registers into one XOR-swizzled LDS image per step: the loads of step t + 1 are
// issued before the MFMAs of step t and written after them, two barriers per step.  The halo is
// made on the way from the staging registers to LDS: a tap that leaves the image (above / below, left / right -- which
// covers the boundary between two images, since a tile's pixel index runs across them) loads the
// pixel's own, always valid, address and is then replaced by zeros, so no load is conditional and
// nothing is ever read out of bounds.
//
// In the Up2 / Down2 forms the source offset of a staged row is no uniform shift of its own: it is
// worked out per (staged row, tap) when the tap changes, never per channel step.
//
// Epilogue: the f32 accumulators, plus the bias where there is one, are rounded once; a lane holds four consecutive pixels of one
// output channel, the tile is transposed through LDS and stored NCHW in 16-byte pieces along the
// pixels.  With a K split (small M) every split stores its f32 partial tile in NCHW order into the
// caller's workspace and conv3x3_reduce_kernel sums the partials in split order and adds the bias: no
// atomics, the same bits on every launch.
//
// The tile loop itself (staging image, swizzle, MFMAs, barriers) is p2p_mma_tile.h's, shared with
// linear_kernel (p2p_linear.hip).  At BK = 64, BN = 160 -- every shape of the U-Net -- the selection
// (select_conv3x3_loop) may instead take conv3x3_pipe_kernel below: the same tile on p2p_mma_pipe.h's
// loop, a global_load_lds ring with the prefetch in flight across the barrier.
#include <atomic>

#include "p2p_mma_pipe.h"

namespace p2p {
namespace {

constexpr int kTilePitch = kConvBM + 8;   // 16-bit elements per channel row of the epilogue's transposed tile

struct ConvArgs {
  const uint16_t* x;   // [n, h w, c_in]
  const uint16_t* wp;  // [9, c_out, c_in]
  void* y;             // [n, c_out, h w] 16-bit, or the f32 partials [split][n, c_out, h w]
  int M, h, w, hw, c_in, c_out;   // h, w: the output map (Same: the input map too)
  int m_tiles, n_tiles, split;
  const uint16_t* bias;   // [c_out] or null (the split form adds it in the reduce)
  int ih, iw;             // the input map of the Up2 / Down2 forms
};

// F16: f16 tensors (else bf16); BK: channels per K step; NF: 16-channel fragments per wave (BN = 32 NF);
// PARTIAL: store the f32 partial of this block's K range instead of the rounded tile; FORM: where a tap
// reads (P2P_CONV_SAME / _UP2 / _DOWN2); BIAS: a.bias is added before the rounding (never with PARTIAL:
// the reduce adds it) -- compiled in, so that the forms without a bias are the code they were
template <bool F16, int BK, int NF, bool PARTIAL, int FORM, bool BIAS>
__global__ __launch_bounds__(kConvThreads) void conv3x3_kernel(ConvArgs a) {
  constexpr int BM = kConvBM, BN = 32 * NF;
  constexpr int CPR = BK / 8;                 // 16-byte chunks per staged row
  constexpr int RPP = kConvThreads / CPR;     // rows per staging pass
  constexpr int NA = BM / RPP, NB = BN / RPP;
  static_assert(BM % RPP == 0 && BN % RPP == 0, "staging passes cover the tiles exactly");
  static_assert(!(PARTIAL && BIAS), "the split form adds the bias in its reduce");
  constexpr int kStage = (BM + BN) * BK * 2;
  constexpr int kEpi = PARTIAL ? 0 : BN * kTilePitch * 2;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kStage > kEpi ? kStage : kEpi];
  unsigned char* const ldsA = lds;
  unsigned char* const ldsB = lds + BM * BK * 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles = a.m_tiles * a.n_tiles;
  int bid = blockIdx.x;
  const int split = bid / tiles;          // slowest: a split's tiles are dispatched together
  bid = xcd_remap(bid - split * tiles, tiles);
  const int m0 = (bid / a.n_tiles) * BM, n0 = (bid % a.n_tiles) * BN;

  const int steps_per_tap = a.c_in / BK;
  const int steps = 9 * steps_per_tap;
  const int t_begin = (int)((int64_t)steps * split / a.split), t_end = (int)((int64_t)steps * (split + 1) / a.split);

  // staging roles: chunk sc of rows sr + RPP i
  const int sc = tid % CPR, sr = tid / CPR;
  int a_off[NA], a_yx[NA];     // element offset of the pixel's chunk; (py << 16 | px), or -1 past M
  int a_lds[NA];
  // Up2 / Down2: a_off is the chunk of the output pixel's own source pixel (the centre tap's, always
  // valid), a_img the chunk in its image's first pixel, a_src what the current tap reads
  [[maybe_unused]] int a_img[NA], a_src[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int r = sr + RPP * i;
    int m = m0 + r;
    const bool in = m < a.M;
    m = in ? m : a.M - 1;
    const int rem = m % a.hw;
    const int py = rem / a.w, px = rem - py * a.w;
    if constexpr (FORM == P2P_CONV_SAME) {
      a_off[i] = m * a.c_in + sc * 8;
    } else {
      a_img[i] = (m / a.hw) * (a.ih * a.iw) * a.c_in + sc * 8;
      const int own = FORM == P2P_CONV_UP2 ? (py >> 1) * a.iw + (px >> 1) : (2 * py) * a.iw + 2 * px;
      a_off[i] = a_img[i] + own * a.c_in;
    }
    a_yx[i] = in ? ((py << 16) | px) : -1;
    a_lds[i] = lds_chunk<BK>(r, sc);
  }
  int b_off[NB], b_lds[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int r = sr + RPP * i;
    const int co = min(n0 + r, a.c_out - 1);   // rows past c_out repeat the last one; never stored
    b_off[i] = co * a.c_in + sc * 8;
    b_lds[i] = lds_chunk<BK>(r, sc);
  }

  u32x4_t ra[NA], rb[NB];
  unsigned ra_ok = 0;          // bit i: ra[i] is inside its image (else write_step stores zeros)
  [[maybe_unused]] int cur_tap = -1;   // Up2 / Down2: the tap a_src and ra_ok stand for
  auto load_step = [&](int t) {
    const int tap = t / steps_per_tap;
    const int c0 = (t - tap * steps_per_tap) * BK;
    const int ky = tap / 3, dy = ky - 1, dx = tap - ky * 3 - 1;
    if constexpr (FORM == P2P_CONV_SAME) {
      const int shift = (dy * a.w + dx) * a.c_in;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int py = a_yx[i] >> 16, px = a_yx[i] & 0xffff;
        const bool ok = (a_yx[i] >= 0) & ((unsigned)(py + dy) < (unsigned)a.h) & ((unsigned)(px + dx) < (unsigned)a.w);
        ra[i] = *reinterpret_cast<const u32x4_t*>(a.x + (a_off[i] + c0 + (ok ? shift : 0)));
        ra_ok = ok ? (ra_ok | (1u << i)) : (ra_ok & ~(1u << i));
      }
    } else {
      if (tap != cur_tap) {   // (uniform) a new tap: where each staged row reads it, and whether it is inside
        cur_tap = tap;
        ra_ok = 0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
          const int py = a_yx[i] >> 16, px = a_yx[i] & 0xffff;
          bool ok;
          int src;
          if constexpr (FORM == P2P_CONV_UP2) {
            const int ty = py + dy, tx = px + dx;   // in the 2 ih x 2 iw map
            ok = (a_yx[i] >= 0) & ((unsigned)ty < (unsigned)a.h) & ((unsigned)tx < (unsigned)a.w);
            src = (ty >> 1) * a.iw + (tx >> 1);
          } else {
            const int ty = 2 * py + dy, tx = 2 * px + dx;   // <= ih - 1, iw - 1 for even ih, iw
            ok = (a_yx[i] >= 0) & (ty >= 0) & (tx >= 0);
            src = ty * a.iw + tx;
          }
          a_src[i] = ok ? a_img[i] + src * a.c_in : a_off[i];
          ra_ok |= ok ? (1u << i) : 0u;
        }
      }
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[i] = *reinterpret_cast<const u32x4_t*>(a.x + (a_src[i] + c0));
    }
    const int wbase = tap * a.c_out * a.c_in + c0;
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[i] = *reinterpret_cast<const u32x4_t*>(a.wp + (wbase + b_off[i]));
  };
  auto write_step = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i)   // the zeros are made here, behind the MFMAs, so that nothing waits for the load early
      *reinterpret_cast<u32x4_t*>(ldsA + a_lds[i]) = ((ra_ok >> i) & 1u) ? ra[i] : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<u32x4_t*>(ldsB + b_lds[i]) = rb[i];
  };

  P2P_MMA_TILE_LOOP(t_begin, t_end)

  // acc[i][j][e]: pixel m0 + wm 64 + i 16 + fq 4 + e, channel n0 + wn 16 NF + j 16 + fr
  if constexpr (PARTIAL) {
    float* const ws = reinterpret_cast<float*>(a.y) + (int64_t)split * a.M * a.c_out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fq * 4;
      if (m >= a.M) continue;               // (M % 8 == 0: the four pixels stand or fall together)
      const int img = m / a.hw, rem = m - img * a.hw;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int co = n0 + wn * (16 * NF) + j * 16 + fr;
        if (co < a.c_out) *reinterpret_cast<f32x4_t*>(ws + ((int64_t)img * a.c_out + co) * a.hw + rem) = acc[i][j];
      }
    }
  } else {
    // (the loop's last barrier stands behind every fragment read: the staging image may be reused)
    uint16_t* const tile = reinterpret_cast<uint16_t*>(lds);
    if constexpr (BIAS) {   // f32 accumulator + bias, then the one rounding
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int co = n0 + wn * (16 * NF) + j * 16 + fr;
        const float b = co < a.c_out ? conv_bias<F16>(a.bias, co) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] += b;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const f32x4_t v = acc[i][j];
        const u32x2_t p = {pack2<F16>(v[0], v[1]), pack2<F16>(v[2], v[3])};
        *reinterpret_cast<u32x2_t*>(tile + (wn * (16 * NF) + j * 16 + fr) * kTilePitch + wm * 64 + i * 16 + fq * 4) = p;
      }
    __syncthreads();
    uint16_t* const y = reinterpret_cast<uint16_t*>(a.y);
    const int ch = tid & 15;                // 8-pixel piece of the tile's 128
    const int m = m0 + ch * 8;
    if (m < a.M) {
      const int img = m / a.hw, rem = m - img * a.hw;   // hw % 8 == 0: a piece stays inside one image
#pragma unroll
      for (int p = 0; p < BN / 16; ++p) {
        const int r = (tid >> 4) + 16 * p;
        if (n0 + r < a.c_out)
          *reinterpret_cast<u32x4_t*>(y + ((int64_t)img * a.c_out + n0 + r) * a.hw + rem) =
              *reinterpret_cast<const u32x4_t*>(tile + r * kTilePitch + ch * 8);
      }
    }
  }
}

// conv3x3_kernel at BK = 64, BN = 160 on p2p_mma_pipe.h's loop: BM = 128 (four waves) or 256 (eight,
// 4 x 2) pixels per workgroup, a ring of D stage images filled by global_load_lds, no staging
// registers.  The tile order, a split's step range, the order K is walked in, each lane's accumulators
// and the epilogue are conv3x3_kernel's, so the output has its bits.
//
// Staging: one DMA instruction is 8 rows; wave v issues A's row groups 4 v .. 4 v + 3 and NBI of B's
// 20 (four waves: 5 each; eight waves: 3 each, groups 20 .. 23 loading 16 .. 19 once more -- the same
// bytes to the same place -- so that every wave's count is the same).  The halo is the choice of
// source: where each of a lane's four pixels reads the current tap, or that it reads kPipeZeros, is
// worked out when the tap changes (a uniform branch), never per channel step, in all three forms.
// The eight-wave form issues a step's DMA between the two halves of the step's MFMAs, the four-wave
// form in front of them: as measured.
template <bool F16, int BM, int D, bool PARTIAL, int FORM, bool BIAS>
__global__ __launch_bounds__(BM * 2) void conv3x3_pipe_kernel(ConvArgs a) {
  constexpr int BK = 64, NF = 5, BN = 32 * NF;
  constexpr int THREADS = BM * 2, WAVES = THREADS / 64;
  constexpr int NA = BM / 8 / WAVES;                     // A DMA instructions per wave and stage
  constexpr int NBI = (BN / 8 + WAVES - 1) / WAVES;      // B's
  static_assert(NA * WAVES * 8 == BM, "A's row groups are shared out exactly");
  static_assert(!(PARTIAL && BIAS), "the split form adds the bias in its reduce");
  constexpr int kStage = (BM + BN) * BK * 2, kBOff = BM * BK * 2;
  constexpr int kPitch = BM + 8;                         // 16-bit elements per channel row of the transposed tile
  constexpr int kEpi = PARTIAL ? 0 : BN * kPitch * 2;
  static_assert(D * kStage <= 160 * 1024 && kEpi <= D * kStage, "the ring fits LDS and holds the epilogue's tile");
  __shared__ __attribute__((aligned(128))) unsigned char lds[D * kStage];
  const uint32_t lds_off = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles = a.m_tiles * a.n_tiles;
  int bid = blockIdx.x;
  const int split = bid / tiles;          // slowest: a split's tiles are dispatched together
  bid = xcd_remap(bid - split * tiles, tiles);
  const int m0 = (bid / a.n_tiles) * BM, n0 = (bid % a.n_tiles) * BN;

  const int steps_per_tap = a.c_in / BK;
  const int steps = 9 * steps_per_tap;
  const int t_begin = (int)((int64_t)steps * split / a.split), t_end = (int)((int64_t)steps * (split + 1) / a.split);

  // staging roles: row lane / 8 of a DMA's 8, 16-byte slot lane % 8, which holds chunk slot ^ row
  const int lrow = lane >> 3, chunk = (lane & 7) ^ lrow;
  int a_base[NA], a_yx[NA];    // Same: element offset of the pixel's chunk, Up2 / Down2: of its image's first
                               // pixel's; (py << 16 | px), or -1 past M
  int a_src[NA];               // what the current tap reads, or -1: zeros
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + (wave * NA + i) * 8 + lrow;
    const bool in = m < a.M;
    const int mc = in ? m : a.M - 1;
    const int rem = mc % a.hw;
    const int py = rem / a.w, px = rem - py * a.w;
    if constexpr (FORM == P2P_CONV_SAME) a_base[i] = mc * a.c_in + chunk * 8;
    else a_base[i] = (mc / a.hw) * (a.ih * a.iw) * a.c_in + chunk * 8;
    a_yx[i] = in ? ((py << 16) | px) : -1;
  }
  int b_off[NBI];
  uint32_t b_lds[NBI];
#pragma unroll
  for (int i = 0; i < NBI; ++i) {
    int g = wave * NBI + i;
    if (g >= BN / 8) g -= NBI * WAVES - BN / 8;   // the surplus loads rows already covered once more
    const int co = min(n0 + g * 8 + lrow, a.c_out - 1);   // rows past c_out repeat the last one; never stored
    b_off[i] = co * a.c_in + chunk * 8;
    b_lds[i] = kBOff + g * 1024;
  }

  int cur_tap = -1;   // the tap a_src stands for
  auto issue = [&](int t, uint32_t stage) __attribute__((always_inline)) {
    const int tap = t / steps_per_tap;
    const int c0 = (t - tap * steps_per_tap) * BK;
    if (tap != cur_tap) {   // (uniform) a new tap: where each staged row reads it, or that it is outside
      cur_tap = tap;
      const int ky = tap / 3, dy = ky - 1, dx = tap - ky * 3 - 1;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int py = a_yx[i] >> 16, px = a_yx[i] & 0xffff;
        bool ok;
        int src;
        if constexpr (FORM == P2P_CONV_SAME) {
          ok = (a_yx[i] >= 0) & ((unsigned)(py + dy) < (unsigned)a.h) & ((unsigned)(px + dx) < (unsigned)a.w);
          src = dy * a.w + dx;
        } else if constexpr (FORM == P2P_CONV_UP2) {
          const int ty = py + dy, tx = px + dx;   // in the 2 ih x 2 iw map
          ok = (a_yx[i] >= 0) & ((unsigned)ty < (unsigned)a.h) & ((unsigned)tx < (unsigned)a.w);
          src = (ty >> 1) * a.iw + (tx >> 1);
        } else {
          const int ty = 2 * py + dy, tx = 2 * px + dx;   // <= ih - 1, iw - 1 for even ih, iw
          ok = (a_yx[i] >= 0) & (ty >= 0) & (tx >= 0);
          src = ty * a.iw + tx;
        }
        a_src[i] = ok ? a_base[i] + src * a.c_in : -1;
      }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const void* const g = a_src[i] >= 0 ? (const void*)(a.x + (a_src[i] + c0)) : (const void*)kPipeZeros;
      pipe_dma16(g, __builtin_amdgcn_readfirstlane(stage + (wave * NA + i) * 1024));
    }
    const int wbase = tap * a.c_out * a.c_in + c0;
#pragma unroll
    for (int i = 0; i < NBI; ++i) pipe_dma16(a.wp + (wbase + b_off[i]), __builtin_amdgcn_readfirstlane(stage + b_lds[i]));
  };

  f32x4_t acc[4][NF];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  mma_pipe_loop<F16, D, NA + NBI, kStage, kBOff, BM == 256>(acc, lds, lds_off, wm, wn, lane, t_begin, t_end, issue);
  const int fr = lane & 15, fq = lane >> 4;

  // acc[i][j][e]: pixel m0 + wm 64 + i 16 + fq 4 + e, channel n0 + wn 16 NF + j 16 + fr
  if constexpr (PARTIAL) {
    float* const ws = reinterpret_cast<float*>(a.y) + (int64_t)split * a.M * a.c_out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + fq * 4;
      if (m >= a.M) continue;               // (M % 8 == 0: the four pixels stand or fall together)
      const int img = m / a.hw, rem = m - img * a.hw;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int co = n0 + wn * (16 * NF) + j * 16 + fr;
        if (co < a.c_out) *reinterpret_cast<f32x4_t*>(ws + ((int64_t)img * a.c_out + co) * a.hw + rem) = acc[i][j];
      }
    }
  } else {
    __syncthreads();   // every DMA has landed (the loop's last wait); behind this, every fragment read too
    uint16_t* const tile = reinterpret_cast<uint16_t*>(lds);
    if constexpr (BIAS) {   // f32 accumulator + bias, then the one rounding
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int co = n0 + wn * (16 * NF) + j * 16 + fr;
        const float b = co < a.c_out ? conv_bias<F16>(a.bias, co) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] += b;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const f32x4_t v = acc[i][j];
        const u32x2_t p = {pack2<F16>(v[0], v[1]), pack2<F16>(v[2], v[3])};
        *reinterpret_cast<u32x2_t*>(tile + (wn * (16 * NF) + j * 16 + fr) * kPitch + wm * 64 + i * 16 + fq * 4) = p;
      }
    __syncthreads();
    uint16_t* const y = reinterpret_cast<uint16_t*>(a.y);
    constexpr int PIECES = BM / 8;          // 8-pixel pieces of a channel row; THREADS / PIECES = 16 rows a pass
    const int ch = tid % PIECES;
    const int m = m0 + ch * 8;
    if (m < a.M) {
      const int img = m / a.hw, rem = m - img * a.hw;   // hw % 8 == 0: a piece stays inside one image
#pragma unroll
      for (int p = 0; p < BN / 16; ++p) {
        const int r = tid / PIECES + 16 * p;
        if (n0 + r < a.c_out)
          *reinterpret_cast<u32x4_t*>(y + ((int64_t)img * a.c_out + n0 + r) * a.hw + rem) =
              *reinterpret_cast<const u32x4_t*>(tile + r * kPitch + ch * 8);
      }
    }
  }
}

// y = round(sum over the splits, in split order, of the f32 partials, + bias[channel] where there is
// one); 8 elements per thread, all of one channel (hw % 8 == 0)
template <bool F16>
__global__ __launch_bounds__(256) void conv3x3_reduce_kernel(const float* ws, uint16_t* y, int64_t total, int split,
                                                             const uint16_t* bias, int hw, int c_out) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= total) return;
  f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(ws + i), s1 = *reinterpret_cast<const f32x4_t*>(ws + i + 4);
  for (int s = 1; s < split; ++s) {
    s0 += *reinterpret_cast<const f32x4_t*>(ws + s * total + i);
    s1 += *reinterpret_cast<const f32x4_t*>(ws + s * total + i + 4);
  }
  if (bias) {
    const float b = conv_bias<F16>(bias, (int)((unsigned)i / (unsigned)hw % (unsigned)c_out));   // (total < 2^31)
    s0 += b;
    s1 += b;
  }
  const u32x4_t o = {pack2<F16>(s0[0], s0[1]), pack2<F16>(s0[2], s0[3]), pack2<F16>(s1[0], s1[1]), pack2<F16>(s1[2], s1[3])};
  *reinterpret_cast<u32x4_t*>(y + i) = o;
}

// packed[tap][co][ci] = w[co][ci][tap]
__global__ __launch_bounds__(256) void conv3x3_pack_kernel(const uint16_t* w, uint16_t* packed, int c_in, int c_out) {
  const int64_t per_tap = (int64_t)c_out * c_in;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_tap * 9) return;
  const int tap = (int)(i / per_tap);
  const int64_t r = i - tap * per_tap;     // co * c_in + ci
  packed[i] = w[r * 9 + tap];
}

template <bool F16, int BK, int NF, int FORM>
void launch_conv_tile(const ConvArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.m_tiles * a.n_tiles * a.split));
  if (a.split > 1) launch_kernel((conv3x3_kernel<F16, BK, NF, true, FORM, false>), grid, dim3(kConvThreads), 0, st, a);
  else if (a.bias) launch_kernel((conv3x3_kernel<F16, BK, NF, false, FORM, true>), grid, dim3(kConvThreads), 0, st, a);
  else launch_kernel((conv3x3_kernel<F16, BK, NF, false, FORM, false>), grid, dim3(kConvThreads), 0, st, a);
}

template <bool F16, int BM, int D, int FORM>
void launch_conv_pipe(const ConvArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(a.m_tiles * a.n_tiles * a.split)), block(BM * 2);
  if (a.split > 1) launch_kernel((conv3x3_pipe_kernel<F16, BM, D, true, FORM, false>), grid, block, 0, st, a);
  else if (a.bias) launch_kernel((conv3x3_pipe_kernel<F16, BM, D, false, FORM, true>), grid, block, 0, st, a);
  else launch_kernel((conv3x3_pipe_kernel<F16, BM, D, false, FORM, false>), grid, block, 0, st, a);
}

template <bool F16, int FORM>
void launch_conv_form(const ConvArgs& a, const ConvPlan& plan, int loop, hipStream_t st) {
  if (loop == CONV_LOOP_PIPE256) launch_conv_pipe<F16, 256, kConvPipeDepth256, FORM>(a, st);
  else if (loop == CONV_LOOP_PIPE128) launch_conv_pipe<F16, 128, kConvPipeDepth128, FORM>(a, st);
  else if (plan.bk == 64 && plan.bn == 160) launch_conv_tile<F16, 64, 5, FORM>(a, st);
  else if (plan.bk == 64) launch_conv_tile<F16, 64, 4, FORM>(a, st);
  else launch_conv_tile<F16, 32, 4, FORM>(a, st);
}

template <bool F16>
void launch_conv(const ConvArgs& a, int form, const ConvPlan& plan, int loop, hipStream_t st) {
  if (form == P2P_CONV_UP2) launch_conv_form<F16, P2P_CONV_UP2>(a, plan, loop, st);
  else if (form == P2P_CONV_DOWN2) launch_conv_form<F16, P2P_CONV_DOWN2>(a, plan, loop, st);
  else launch_conv_form<F16, P2P_CONV_SAME>(a, plan, loop, st);
}

// p2p_conv3x3_set_loop's value: 0 = select_conv3x3_loop's choice, else the loop every BK = 64, BN = 160
// launch takes
std::atomic<int> g_conv_loop{CONV_LOOP_AUTO};

bool conv_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// the launcher: run_conv3x3_ex (p2p_dispatch.hip) has checked the arguments, worked out the output map
// (out_h x out_w) and chosen the plan
int launch_conv3x3(const p2p_conv3x3_ex_args& a, int out_h, int out_w, const ConvPlan& plan, hipStream_t st) {
  ConvArgs k;
  k.x = (const uint16_t*)a.x;
  k.wp = (const uint16_t*)a.weight;
  k.hw = out_h * out_w;
  k.M = a.n * k.hw;
  k.h = out_h, k.w = out_w, k.c_in = a.c_in, k.c_out = a.c_out;
  k.ih = a.in_height, k.iw = a.in_width;
  k.bias = plan.split > 1 ? nullptr : (const uint16_t*)a.bias;
  const int loop = conv3x3_loop(g_conv_loop.load(std::memory_order_relaxed), plan, a.form, a.n, out_h, out_w, a.c_in, a.c_out);
  const int bm = conv3x3_loop_bm(loop);
  k.m_tiles = (k.M + bm - 1) / bm;
  k.n_tiles = (a.c_out + plan.bn - 1) / plan.bn;
  k.split = plan.split;
  k.y = plan.split > 1 ? (void*)a.workspace : a.y;
  if (a.dtype == P2P_DTYPE_F16) launch_conv<true>(k, a.form, plan, loop, st);
  else launch_conv<false>(k, a.form, plan, loop, st);
  if (plan.split > 1) {
    const int64_t total = (int64_t)k.M * a.c_out;   // % 8 == 0 (hw % 8 == 0)
    const dim3 grid((unsigned)((total / 8 + 255) / 256));
    if (a.dtype == P2P_DTYPE_F16)
      launch_kernel(conv3x3_reduce_kernel<true>, grid, dim3(256), 0, st, (const float*)a.workspace, (uint16_t*)a.y, total,
                    plan.split, (const uint16_t*)a.bias, k.hw, a.c_out);
    else
      launch_kernel(conv3x3_reduce_kernel<false>, grid, dim3(256), 0, st, (const float*)a.workspace, (uint16_t*)a.y, total,
                    plan.split, (const uint16_t*)a.bias, k.hw, a.c_out);
  }
  return (int)hipGetLastError();
}

int set_conv3x3_loop(int loop) {
  if (loop != CONV_LOOP_AUTO && loop != CONV_LOOP_TILE && loop != CONV_LOOP_PIPE128 && loop != CONV_LOOP_PIPE256) return P2P_E_ARG;
  g_conv_loop.store(loop, std::memory_order_relaxed);
  return 0;
}

int run_conv3x3_pack(const p2p_conv3x3_pack_args& a, hipStream_t st) {
  if (!a.weight || !a.packed) return P2P_E_ARG;
  if (a.c_in < 1 || a.c_out < 1 || (int64_t)a.c_in * a.c_out * 9 > INT32_MAX) return P2P_E_ARG;
  if (a.dtype != P2P_DTYPE_BF16 && a.dtype != P2P_DTYPE_F16) return P2P_E_DTYPE;
  if (a.c_in % 32 || a.c_out % 32) return P2P_E_ALIGN;
  if (((uintptr_t)a.weight & 1) || !conv_aligned16(a.packed)) return P2P_E_ALIGN;
  const int64_t total = (int64_t)a.c_in * a.c_out * 9;
  launch_kernel(conv3x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint16_t*)a.weight,
                (uint16_t*)a.packed, a.c_in, a.c_out);
  return (int)hipGetLastError();
}

}  // namespace p2p
