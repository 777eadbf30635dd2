// The image ends of the pipeline (ptp_utils.latent2image / NullInversion.image2latent): the VAE
// decoder's output as uint8 pixels, and uint8 pixels as the encoder's input.  Bandwidth-bound, one
// pass each, four pixels per thread.
//
// image_u8_kernel reproduces the reference's eager f32 arithmetic operation by operation
// (x / 2 + 0.5, clamp to [0, 1], * 255, truncate): every product and sum is rounded on its own
// (__fmul_rn / __fadd_rn: never contracted into an fma), so the bytes equal torch's.
// image_to_model_kernel computes x / 127.5 - 1 in f32 (an IEEE division, then the subtraction) and
// rounds once to the output type.
//
// Odd sizes: both kernels take height * width % 4 == 0 only and the entry points answer
// P2P_E_ALIGN otherwise (no scalar tail); the Python callers then run their torch lines.
#include "p2p_device.h"
#include "p2p_kernels.h"

namespace p2p {
namespace {

template <int DT>
struct ImgIO;
template <>
struct ImgIO<P2P_DTYPE_F32> {
  typedef f32x4_t vec;
  __device__ __forceinline__ static float get(const vec& v, int j) { return v[j]; }
  __device__ __forceinline__ static void set(vec& v, int j, float x) { v[j] = x; }
};
template <>
struct ImgIO<P2P_DTYPE_BF16> {
  typedef short4_t vec;
  __device__ __forceinline__ static float get(const vec& v, int j) { return bf2f((uint16_t)v[j]); }
  __device__ __forceinline__ static void set(vec& v, int j, float x) { v[j] = (short)f2bf(x); }
};
template <>
struct ImgIO<P2P_DTYPE_F16> {
  typedef short4_t vec;
  __device__ __forceinline__ static float get(const vec& v, int j) { return h2f((uint16_t)v[j]); }
  __device__ __forceinline__ static void set(vec& v, int j, float x) { v[j] = (short)f2h(x); }
};

// x [n, 3, hw] -> out [n, hw, 3] uint8; thread iv: pixels 4 iv .. 4 iv + 3 of one image
template <int DT>
__global__ __launch_bounds__(256) void image_u8_kernel(p2p_image_u8_args a, int64_t n_vec, int hw4) {
  using IO = ImgIO<DT>;
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int64_t n = iv / hw4;
  const int64_t pv = iv - n * hw4;
  const typename IO::vec* const x = static_cast<const typename IO::vec*>(a.x) + n * 3 * hw4 + pv;
  uint32_t bytes[12];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const typename IO::vec v = x[(int64_t)c * hw4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float y = __fadd_rn(__fmul_rn(IO::get(v, j), 0.5f), 0.5f);   // x / 2 is exact as x * 0.5
      y = fminf(fmaxf(y, 0.f), 1.f);
      bytes[3 * j + c] = (uint32_t)(int)__fmul_rn(y, 255.f);
    }
  }
  uint32_t* const out = reinterpret_cast<uint32_t*>(a.out) + iv * 3;
#pragma unroll
  for (int w = 0; w < 3; ++w)
    out[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | (bytes[4 * w + 3] << 24);
}

// img [n, hw, 3] uint8 -> out [n, 3, hw]
template <int DT>
__global__ __launch_bounds__(256) void image_to_model_kernel(p2p_image_to_model_args a, int64_t n_vec, int hw4) {
  using IO = ImgIO<DT>;
  const int64_t iv = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (iv >= n_vec) return;
  const int64_t n = iv / hw4;
  const int64_t pv = iv - n * hw4;
  const uint32_t* const in = reinterpret_cast<const uint32_t*>(a.img) + iv * 3;
  uint32_t bytes[12];
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const uint32_t u = in[w];
#pragma unroll
    for (int b = 0; b < 4; ++b) bytes[4 * w + b] = (u >> (8 * b)) & 0xffu;
  }
  typename IO::vec* const out = static_cast<typename IO::vec*>(a.out) + n * 3 * hw4 + pv;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    typename IO::vec v;
#pragma unroll
    for (int j = 0; j < 4; ++j) IO::set(v, j, __fsub_rn(__fdiv_rn((float)bytes[3 * j + c], 127.5f), 1.0f));
    out[(int64_t)c * hw4] = v;
  }
}

bool dtype_ok(int dt) { return dt == P2P_DTYPE_F32 || dt == P2P_DTYPE_BF16 || dt == P2P_DTYPE_F16; }

// the checks both entry points share; n_vec: four-pixel vectors of the launch
int check_image(const void* in, const void* out, int n, int h, int w, int dtype, int64_t* n_vec) {
  if (!in || !out) return P2P_E_ARG;
  if (n < 1 || h < 1 || w < 1) return P2P_E_ARG;
  if (!dtype_ok(dtype)) return P2P_E_DTYPE;
  const int64_t hw = (int64_t)h * w;
  if (hw > INT32_MAX) return P2P_E_ARG;
  if (hw % 4) return P2P_E_ALIGN;
  *n_vec = (int64_t)n * (hw / 4);
  if ((*n_vec + 255) / 256 > INT32_MAX) return P2P_E_ARG;
  return 0;
}

}  // namespace

int run_image_u8(const p2p_image_u8_args& a, hipStream_t st) {
  int64_t n_vec = 0;
  const int rc = check_image(a.x, a.out, a.n, a.height, a.width, a.dtype, &n_vec);
  if (rc) return rc;
  if (((uintptr_t)a.x & 15) || ((uintptr_t)a.out & 3)) return P2P_E_ALIGN;
  const int hw4 = (int)((int64_t)a.height * a.width / 4);
  const dim3 grid((unsigned)((n_vec + 255) / 256));
  if (a.dtype == P2P_DTYPE_F32) launch_kernel(image_u8_kernel<P2P_DTYPE_F32>, grid, dim3(256), 0, st, a, n_vec, hw4);
  else if (a.dtype == P2P_DTYPE_BF16) launch_kernel(image_u8_kernel<P2P_DTYPE_BF16>, grid, dim3(256), 0, st, a, n_vec, hw4);
  else launch_kernel(image_u8_kernel<P2P_DTYPE_F16>, grid, dim3(256), 0, st, a, n_vec, hw4);
  return (int)hipGetLastError();
}

int run_image_to_model(const p2p_image_to_model_args& a, hipStream_t st) {
  int64_t n_vec = 0;
  const int rc = check_image(a.img, a.out, a.n, a.height, a.width, a.dtype, &n_vec);
  if (rc) return rc;
  if (((uintptr_t)a.img & 3) || ((uintptr_t)a.out & 15)) return P2P_E_ALIGN;
  const int hw4 = (int)((int64_t)a.height * a.width / 4);
  const dim3 grid((unsigned)((n_vec + 255) / 256));
  if (a.dtype == P2P_DTYPE_F32)
    launch_kernel(image_to_model_kernel<P2P_DTYPE_F32>, grid, dim3(256), 0, st, a, n_vec, hw4);
  else if (a.dtype == P2P_DTYPE_BF16)
    launch_kernel(image_to_model_kernel<P2P_DTYPE_BF16>, grid, dim3(256), 0, st, a, n_vec, hw4);
  else
    launch_kernel(image_to_model_kernel<P2P_DTYPE_F16>, grid, dim3(256), 0, st, a, n_vec, hw4);
  return (int)hipGetLastError();
}

}  // namespace p2p
