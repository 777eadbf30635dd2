// run_self / run_cross / run_conv3x3 / run_linear: pick the kernel form (p2p_select.h) and hand it to its file's launcher.
// Host code only; nothing here decides.
#include "p2p_kernels.h"

namespace p2p {

int run_self(const SelfArgs& a, int io_dtype, int compute, int d, int mode, hipStream_t st) {
  const int sel = select_self(a, io_dtype, compute, d, mode);
  if (sel < 0) return sel;
  const SelfKernel k = (SelfKernel)sel;
  switch (self_info(k).family) {
    case FAM_MULTI: return launch_self_multi(a, k, st);
    case FAM_SELF40: return launch_self40(a, k, st);
    case FAM_SPLIT:
    case FAM_HALVES:
    case FAM_RING: return launch_self_split(a, k, st);
    case FAM_WIDE: return launch_self_wide(a, select_precision(io_dtype, compute), st);
    default: return launch_self_fused(a, select_precision(io_dtype, compute), d, k, st);
  }
}

int run_cross(const CrossArgs& a, int io_dtype, int compute, int d, hipStream_t st) {
  const int sel = select_cross(a, io_dtype, compute, d);
  if (sel < 0) return sel;
  const CrossKernel k = (CrossKernel)sel;
  if (is_group(k)) return launch_cross_group(a, d, k, st);
  return launch_cross_entry(a, select_precision(io_dtype, compute), d, k, st);
}

int run_conv3x3_ex(const p2p_conv3x3_ex_args& a, hipStream_t st) {
  if (!a.x || !a.weight || !a.y) return P2P_E_ARG;
  const int rc = conv3x3_check_sizes(a.form, a.n, a.in_height, a.in_width, a.c_in, a.c_out);
  if (rc == P2P_E_ARG) return rc;
  if (a.dtype != P2P_DTYPE_BF16 && a.dtype != P2P_DTYPE_F16) return P2P_E_DTYPE;
  if (rc < 0) return rc;
  if (((uintptr_t)a.x | (uintptr_t)a.weight | (uintptr_t)a.y | (uintptr_t)a.workspace) & 15) return P2P_E_ALIGN;
  if ((uintptr_t)a.bias & 1) return P2P_E_ALIGN;
  int oh = 0, ow = 0;
  conv3x3_out_map(a.form, a.in_height, a.in_width, &oh, &ow);   // (checked above)
  const ConvPlan plan = select_conv3x3(a.form, a.n, oh, ow, a.c_in, a.c_out);
  if (plan.split < 1) return P2P_E_ALIGN;   // a size the selection leaves to the caller's convolution
  if (plan.split > 1 && !a.workspace) return P2P_E_ARG;
  return launch_conv3x3(a, oh, ow, plan, st);
}

int run_conv3x3(const p2p_conv3x3_args& a, hipStream_t st) {
  p2p_conv3x3_ex_args e = {};
  e.x = a.x, e.weight = a.weight, e.y = a.y, e.workspace = a.workspace;
  e.n = a.n, e.in_height = a.height, e.in_width = a.width, e.c_in = a.c_in, e.c_out = a.c_out;
  e.dtype = a.dtype, e.form = P2P_CONV_SAME;
  return run_conv3x3_ex(e, st);
}

int run_linear(const p2p_linear_args& a, hipStream_t st) {
  if (!a.x || !a.weight || !a.y || (a.form == P2P_LINEAR_RESIDUAL && !a.res)) return P2P_E_ARG;
  const int rc = linear_check_sizes(a.form, a.m, a.k, a.n);
  if (rc == P2P_E_ARG) return rc;
  const bool residual = a.form == P2P_LINEAR_RESIDUAL;
  // x's and res's element offsets are 32-bit in the kernel too
  if (a.x_row_stride < 0 || (int64_t)(a.m - 1) * a.x_row_stride + a.k > INT32_MAX) return P2P_E_ARG;
  if (residual && (a.res_row_stride < 0 || (int64_t)(a.m - 1) * a.res_row_stride + a.n > INT32_MAX)) return P2P_E_ARG;
  if (a.dtype != P2P_DTYPE_BF16 && a.dtype != P2P_DTYPE_F16) return P2P_E_DTYPE;
  if (rc < 0) return rc;
  if (a.x_row_stride % 8 || a.x_row_stride < a.k) return P2P_E_ALIGN;
  if (residual && (a.res_row_stride % 8 || a.res_row_stride < a.n)) return P2P_E_ALIGN;
  uintptr_t ptrs = (uintptr_t)a.x | (uintptr_t)a.weight | (uintptr_t)a.y | (uintptr_t)a.workspace;
  if (residual) ptrs |= (uintptr_t)a.res;
  if (a.form == P2P_LINEAR_GEGLU) ptrs |= (uintptr_t)a.p_out;
  if ((ptrs & 15) || ((uintptr_t)a.bias & 1)) return P2P_E_ALIGN;
  const LinearPlan plan = select_linear(a.form, a.m, a.k, a.n);
  if (plan.split < 1) return P2P_E_ALIGN;   // a shape the selection leaves to the caller's GEMM
  if (plan.split > 1 && !a.workspace) return P2P_E_ARG;
  return launch_linear(a, plan, st);
}

}  // namespace p2p
