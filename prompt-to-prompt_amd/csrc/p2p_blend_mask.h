// LocalBlend's mask build (null_text.py:41-67), shared by p2p_blend.hip's blend_finalize_kernel and
// p2p_latent.hip's latent_blend_kernel: both call build_blend_mask, so both build the same mask bit
// for bit.
#pragma once

#include "p2p_device.h"

namespace p2p {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// LDS of one mask build (256 threads): mean maps, pooled maps, per-wave maxima, the mask per map
// pixel.  [0] = the group's source prompt, [1] = prompt b
struct BlendLds {
  float mean_a[2][256];
  float mean_s[2][256];
  float pooled[2][256];
  float red[4][4];
  float msrc[256];
};

// nearest upsampling (F.interpolate default): latent pixel yx -> map pixel
__device__ __forceinline__ int blend_src_of(int yx, int R, int lat_h, int lat_w) {
  const float sy = (float)R / (float)lat_h, sx = (float)R / (float)lat_w;
  const int Y = yx / lat_w, X = yx - Y * lat_w;
  return min((int)floorf(Y * sy), R - 1) * R + min((int)floorf(X * sx), R - 1);
}

// Prompt b's LocalBlend mask per map pixel (L.msrc, 1.f / 0.f) from the word sums of its group's
// source prompt (ws0) and its own (wsb), each [2, LH, R*R] (index 0: alpha-weighted, 1:
// substruct-weighted): mean over the LH maps, 3x3 max-pool, per-image max of the upsampled map,
// thresholds, mask[:1] | mask, substruct gate (null_text.py:41-67).  Called by all 256 threads of
// the workgroup (it synchronises); blend_finalize_kernel and latent_blend_kernel share it, so
// both build the same mask bit for bit.
__device__ __forceinline__ void build_blend_mask(const float* ws0, const float* wsb, int LH, int R, int lat_h, int lat_w,
                                 float th_pool, float th_sub, bool sub, BlendLds& L) {
  const int R2 = R * R;
  const int tid = threadIdx.x;
  // mean over the L*H maps (sum in index order, then / L*H as Tensor.mean does).  The four
  // (prompt, sum) planes -- source / b x alpha / substruct -- go to the four waves; a lane sums
  // four adjacent map pixels, so every load is one 16-byte row piece and a wave's LH loads of a
  // plane are all in flight at once (one memory round trip for the whole mask)
  {
    // (source | b) x (alpha | substruct); the wave index in a scalar register, so the plane's buffer
    // resource is scalar too (from a VGPR each of the 48 loads became a readfirstlane waterfall loop)
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6), k = g & 1, sidx = g >> 1;
    const int px0 = (tid & 63) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (px0 < R2 && (sidx == 0 || sub)) {
      const float* base = (k ? wsb : ws0) + (int64_t)sidx * LH * R2;
      if ((R2 & 3) == 0) {
        // buffer loads: maps past LH read as 0 (range-checked), so the 48 loads of a batch are
        // issued unconditionally, all before the first add; adding those +0.0 to a sum of
        // non-negative terms leaves it bit for bit (the in-order sum over j < LH)
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, (int64_t)LH * R2 * 4);
        for (int j0 = 0; j0 < LH; j0 += 48) {
          f32x4_t v[48];
#pragma unroll
          for (int u = 0; u < 48; ++u)
            v[u] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, ((j0 + u) * R2 + px0) * 4, 0, 0));
#pragma unroll
          for (int u = 0; u < 48; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += v[u][q];
        }
      } else {
        for (int j = 0; j < LH; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (px0 + q < R2) acc[q] += base[(int64_t)j * R2 + px0 + q];
      }
    }
    float* const dst = sidx == 0 ? L.mean_a[k] : L.mean_s[k];
    float pmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (px0 + q < R2) {
        const float mv = acc[q] / (float)LH;
        dst[px0 + q] = mv;
        pmax = fmaxf(pmax, mv);
      }
    // the wave holds its whole plane: its maximum needs no cross-wave reduction
    pmax = wave_max(pmax);
    if ((tid & 63) == 0) L.red[0][g] = pmax;
  }
  __syncthreads();
  if (lat_h >= R && lat_w >= R) {
    // Upsampling samples every map pixel, and a 3x3 max-pool keeps the plane's maximum (every
    // pixel lies in its own window), so the per-image maxima of the pooled / unpooled upsampled
    // maps are the four plane maxima above -- the same floats the generic path below reduces to.
    // Pool on the fly and threshold: one more barrier in all (mask per map pixel, gathered by the
    // nearest upsampling: identical per output pixel, evaluated R*R times instead of H*W)
    const float v0 = L.red[0][0], vb = L.red[0][1], s0m = L.red[0][2], sbm = L.red[0][3];
    for (int pix = tid; pix < R2; pix += 256) {
      const int y = pix / R, x = pix - y * R;
      float p0 = -INFINITY, pb = -INFINITY;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if (yy >= 0 && yy < R && xx >= 0 && xx < R) {
            p0 = fmaxf(p0, L.mean_a[0][yy * R + xx]);
            pb = fmaxf(pb, L.mean_a[1][yy * R + xx]);
          }
        }
      bool mask = p0 / v0 > th_pool || pb / vb > th_pool;
      if (sub) mask = mask && !(L.mean_s[0][pix] / s0m > th_sub || L.mean_s[1][pix] / sbm > th_sub);
      L.msrc[pix] = mask ? 1.f : 0.f;
    }
    __syncthreads();
    return;
  }
  // generic path (latent smaller than the maps: the nearest down-sampling skips map pixels)
  // 3x3 max-pool, stride 1, padding 1 (padding never wins: -inf)
  for (int i = tid; i < 2 * R2; i += 256) {
    const int k = i / R2, pix = i - k * R2;
    const int y = pix / R, x = pix - y * R;
    float m = -INFINITY;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < R && xx >= 0 && xx < R) m = fmaxf(m, L.mean_a[k][yy * R + xx]);
      }
    L.pooled[k][pix] = m;
  }
  __syncthreads();
  // per-image max of the nearest-upsampled maps.  Upsampling (latent >= map resolution) samples
  // every source pixel, so the max over the grid is the max over the R*R sources.
  const bool all_sources = lat_h >= R && lat_w >= R;
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int i = tid; i < (all_sources ? R2 : lat_h * lat_w); i += 256) {
    const int src = all_sources ? i : blend_src_of(i, R, lat_h, lat_w);
    m[0] = fmaxf(m[0], L.pooled[0][src]);
    m[1] = fmaxf(m[1], L.mean_s[0][src]);
    m[2] = fmaxf(m[2], L.pooled[1][src]);
    m[3] = fmaxf(m[3], L.mean_s[1][src]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) m[c] = wave_max(m[c]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) L.red[tid >> 6][c] = m[c];
  __syncthreads();
  float vmax[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    vmax[c] = L.red[0][c];
    for (int w = 1; w < 4; ++w) vmax[c] = fmaxf(vmax[c], L.red[w][c]);
  }
  // mask of prompt b per source pixel (the thresholds of null_text.py:62-67), then gathered by
  // the nearest upsampling: identical per output pixel, evaluated R*R times instead of H*W
  for (int pix = tid; pix < R2; pix += 256) {
    const bool m0 = L.pooled[0][pix] / vmax[0] > th_pool;
    const bool mb = L.pooled[1][pix] / vmax[2] > th_pool;
    bool mask = m0 || mb;
    if (sub) {
      const bool s0 = L.mean_s[0][pix] / vmax[1] > th_sub;
      const bool sb = L.mean_s[1][pix] / vmax[3] > th_sub;
      mask = mask && !(s0 || sb);
    }
    L.msrc[pix] = mask ? 1.f : 0.f;
  }
  __syncthreads();
}

}  // namespace p2p
