// The all-precision attention kernels as ONE object: self_attn_fused_kernel / self_pv_kernel
// (p2p_self.hip) and cross_attn_kernel (p2p_cross_entry.hip).  The two files are split by role and
// read on their own, but they are compiled together: hipcc optimises the device helpers they share
// per translation unit, before inlining them, and as separate objects the sixteen exact-f32
// self kernels (self_pv_kernel<float, MmaF32, *>, self_attn_fused_kernel<float, QkF32, MmaF32,
// 80 | 160, ...>) came out with other LDS address arithmetic and 2-8 more registers (f32 P V up to
// 3.4 % slower).  In this order every kernel is instruction for instruction what the undivided
// source gave.
#include "p2p_self.hip"
#include "p2p_cross_entry.hip"
