// run_self / run_cross: pick the kernel form (p2p_select.h) and hand it to its file's launcher.
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

}  // namespace p2p
