// The attention-map figures (main.py:293-350: aggregate_attention, show_cross_attention,
// show_self_attention_comp) made where the maps live.
//
// maps_aggregate_kernel: the selected prompt's average over the stored layers and their heads of
// the step-averaged maps, read straight from AttentionStore's f32 running sums.  Only the selected
// prompt's slabs are read; no scaled copy of a store is made.  The arithmetic is fixed: every term
// is s / (float)steps (an IEEE division), the terms are added in f32 one after another in the
// order aggregate_attention concatenates them (layer-major, head-minor), and the sum is divided
// once by the term count.
//
// map_panels_kernel: n maps as n grey RGB uint8 panels, normalised and upscaled as the reference's
// NumPy + PIL lines do it (main.py:320-324, :342-348).  The normalisation rounds operation by
// operation in f32 (__fmul_rn / __fdiv_rn / __fsub_rn; the object is built with -ffp-contract=off);
// the resize is PIL's 8-bit bicubic: per output pixel at most P2P_RESIZE_TAPS integer taps in
// 22-bit fixed point (built on the host, _hip.resize_coeffs), an accumulator that starts at 2^21,
// a shift and a clamp, the horizontal pass rounded to uint8 before the vertical pass.  One
// workgroup per panel: the panel, its uint8 form and the res x S intermediate stay in LDS.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {
namespace {

constexpr int kResizeBits = 22;   // PIL's PRECISION_BITS for 8-bit images (32 - 8 - 2)

__global__ __launch_bounds__(256) void maps_aggregate_kernel(p2p_maps_aggregate_args a, int64_t n_vec, int64_t pk4,
                                                             int n_terms) {
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const float steps = (float)a.steps;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  bool first = true;
  for (int l = 0; l < a.n_layers; ++l) {
    const int heads = a.heads[l];
    // the selected prompt's slabs of this layer: [heads, P * K], in four-element vectors
    const f32x4_t* const src = reinterpret_cast<const f32x4_t*>(a.stores[l]) + (int64_t)a.select * heads * pk4 + iv;
#pragma unroll 4
    for (int h = 0; h < heads; ++h) {
      const f32x4_t s = src[(int64_t)h * pk4];
      f32x4_t t;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = __fdiv_rn(s[j], steps);
      if (first) {
        acc = t;   // (not 0 + t: a -0 stays a -0)
        first = false;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], t[j]);
      }
    }
  }
  const float cnt = (float)n_terms;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = __fdiv_rn(acc[j], cnt);
  reinterpret_cast<f32x4_t*>(a.out)[iv] = acc;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kResizeBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// LDS: f32 panel [res * res] | uint8 intermediate [res][S] | uint8 panel [res * res] | 12 words of
// reduction scratch, each part rounded up to 16 bytes (map_panels_lds below)
__global__ __launch_bounds__(256) void map_panels_kernel(p2p_map_panels_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int res = a.res, S = a.S, rr = res * res;
  const int tid = threadIdx.x;
  float* const panel = reinterpret_cast<float*>(lds);
  uint8_t* const mid = lds + ((rr * 4 + 15) & ~15);
  uint8_t* const pix = mid + ((res * S + 15) & ~15);
  float* const red_max = reinterpret_cast<float*>(pix + ((rr + 15) & ~15));   // one slot per wave
  float* const red_min = red_max + 4;
  int* const red_nan = reinterpret_cast<int*>(red_min + 4);
  const float* const in = a.in + (int64_t)blockIdx.x * a.panel_stride;

  // 1. the panel into LDS; its maximum, its minimum, and whether it holds a NaN
  float vmax = -INFINITY, vmin = INFINITY;
  int nan = 0;
  if (a.pixel_stride == 1 && rr % 4 == 0 && (((uintptr_t)in) & 15) == 0) {
    for (int p = tid; p < rr / 4; p += 256) {
      const f32x4_t v = reinterpret_cast<const f32x4_t*>(in)[p];
      reinterpret_cast<f32x4_t*>(panel)[p] = v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        nan |= v[j] != v[j];
        vmax = fmaxf(vmax, v[j]);
        vmin = fminf(vmin, v[j]);
      }
    }
  } else {
    for (int p = tid; p < rr; p += 256) {
      const float v = in[(int64_t)p * a.pixel_stride];
      panel[p] = v;
      nan |= v != v;
      vmax = fmaxf(vmax, v);
      vmin = fminf(vmin, v);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
    vmin = fminf(vmin, __shfl_xor(vmin, off, 64));
    nan |= __shfl_xor(nan, off, 64);
  }
  if ((tid & 63) == 0) {
    red_max[tid >> 6] = vmax;
    red_min[tid >> 6] = vmin;
    red_nan[tid >> 6] = nan;
  }
  __syncthreads();
  vmax = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
  vmin = fminf(fminf(red_min[0], red_min[1]), fminf(red_min[2], red_min[3]));
  nan = red_nan[0] | red_nan[1] | red_nan[2] | red_nan[3];

  // 2. normalise and truncate.  MINMAX: x' = x - min, and max x' = max - min (the subtraction of
  // one value is monotone under rounding), so one reduction serves both modes
  const bool minmax = a.mode == P2P_PANEL_MINMAX;
  const float sub = minmax ? vmin : 0.f;
  const float div = minmax ? __fsub_rn(vmax, vmin) : vmax;
  const bool blank = nan || div == 0.f || div != div;   // (inf - inf: a NaN divisor)
  for (int p = tid; p < rr; p += 256) {
    float x = panel[p];
    if (minmax) x = __fsub_rn(x, sub);
    const float y = __fdiv_rn(__fmul_rn(255.f, x), div);
    pix[p] = blank ? (uint8_t)0 : (uint8_t)(int)y;
  }
  __syncthreads();

  // 3. horizontal pass: mid[y][xx] from pix[y][xmin .. xmin + n)
  for (int i = tid; i < res * S; i += 256) {
    const int y = i / S, xx = i - y * S;
    int x0 = a.bounds[2 * xx], cnt = a.bounds[2 * xx + 1];
    x0 = x0 < 0 ? 0 : (x0 > res ? res : x0);                 // a table of some other size must not
    cnt = cnt > P2P_RESIZE_TAPS ? P2P_RESIZE_TAPS : cnt;     // read past the panel
    cnt = cnt > res - x0 ? res - x0 : cnt;
    const int32_t* const k = a.coeffs + xx * P2P_RESIZE_TAPS;
    int acc = 1 << (kResizeBits - 1);
    for (int t = 0; t < cnt; ++t) acc += (int)pix[y * res + x0 + t] * k[t];
    mid[i] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  // 4. vertical pass, four output pixels per thread: their three equal bytes as three dwords
  uint8_t* const out = a.out + (int64_t)blockIdx.x * a.out_panel_stride;
  const int s4 = S / 4;
  for (int i = tid; i < S * s4; i += 256) {
    const int yy = i / s4, x4 = i - yy * s4;
    int y0 = a.bounds[2 * yy], cnt = a.bounds[2 * yy + 1];
    y0 = y0 < 0 ? 0 : (y0 > res ? res : y0);
    cnt = cnt > P2P_RESIZE_TAPS ? P2P_RESIZE_TAPS : cnt;
    cnt = cnt > res - y0 ? res - y0 : cnt;
    const int32_t* const k = a.coeffs + yy * P2P_RESIZE_TAPS;
    int acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 1 << (kResizeBits - 1);
    for (int t = 0; t < cnt; ++t) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(mid + (y0 + t) * S + 4 * x4);
      const int kt = k[t];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += (int)((u >> (8 * j)) & 0xffu) * kt;
    }
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (uint32_t)clip8(acc[j]);
    uint32_t* const dst = reinterpret_cast<uint32_t*>(out + (int64_t)yy * a.out_row_stride + 12 * x4);
    dst[0] = v[0] * 0x010101u | (v[1] << 24);
    dst[1] = v[1] * 0x0101u | (v[2] * 0x0101u << 16);
    dst[2] = v[2] | (v[3] * 0x010101u << 8);
  }
}

uint32_t map_panels_lds(int res, int S) {
  const int rr = res * res;
  return (uint32_t)(((rr * 4 + 15) & ~15) + ((res * S + 15) & ~15) + ((rr + 15) & ~15) + 48);
}

}  // namespace

int run_maps_aggregate(const p2p_maps_aggregate_args& a, hipStream_t st) {
  if (!a.out) return P2P_E_ARG;
  if (a.n_layers < 1 || a.n_layers > P2P_MAX_AGG_LAYERS) return P2P_E_ARG;
  if (a.n_prompts < 1 || a.select < 0 || a.select >= a.n_prompts) return P2P_E_ARG;
  if (a.P < 1 || a.K < 1 || a.steps < 1) return P2P_E_ARG;
  int64_t n_terms = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    if (!a.stores[l] || a.heads[l] < 1) return P2P_E_ARG;
    n_terms += a.heads[l];
  }
  if (n_terms > (1 << 24)) return P2P_E_ARG;   // the count is exact as a float
  const int64_t pk = (int64_t)a.P * a.K;
  if (pk % 4) return P2P_E_ALIGN;
  if ((uintptr_t)a.out & 15) return P2P_E_ALIGN;
  for (int l = 0; l < a.n_layers; ++l)
    if ((uintptr_t)a.stores[l] & 15) return P2P_E_ALIGN;
  const int64_t n_vec = pk / 4;
  if ((n_vec + 255) / 256 > INT32_MAX) return P2P_E_ARG;
  launch_kernel(maps_aggregate_kernel, dim3((unsigned)((n_vec + 255) / 256)), dim3(256), 0, st, a, n_vec, n_vec,
                (int)n_terms);
  return (int)hipGetLastError();
}

int run_map_panels(const p2p_map_panels_args& a, hipStream_t st) {
  if (!a.in || !a.out || !a.coeffs || !a.bounds) return P2P_E_ARG;
  if (a.mode != P2P_PANEL_MAX && a.mode != P2P_PANEL_MINMAX) return P2P_E_ARG;
  if (a.n < 1 || a.res < 1 || a.res > P2P_PANEL_MAX_RES) return P2P_E_ARG;
  if (a.S < a.res || a.S > P2P_PANEL_MAX_SIDE || a.S % 4) return P2P_E_ARG;
  if (a.pixel_stride < 1 || a.panel_stride < 0) return P2P_E_ARG;
  if (a.out_row_stride < 3 * (int64_t)a.S || a.out_panel_stride < 0) return P2P_E_ARG;
  if (((uintptr_t)a.in & 3) || ((uintptr_t)a.coeffs & 3) || ((uintptr_t)a.bounds & 3)) return P2P_E_ALIGN;
  if (((uintptr_t)a.out & 3) || (a.out_row_stride & 3) || (a.out_panel_stride & 3)) return P2P_E_ALIGN;
  launch_kernel(map_panels_kernel, dim3((unsigned)a.n), dim3(256), map_panels_lds(a.res, a.S), st, a);
  return (int)hipGetLastError();
}

}  // namespace p2p
