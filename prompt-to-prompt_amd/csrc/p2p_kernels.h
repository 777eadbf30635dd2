// Kernel-argument structs shared by the kernels and the C-ABI shim (passed by value).
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2p_hip.h"
#include "p2p_select.h"

namespace p2p {

// Kernel timing events of the calling thread (p2p_set_launch_events, ABI 15; measurement only):
// while set, launches go through hipExtLaunchKernel, which records the events from the kernel's own
// dispatch -- the first kernel of a C-ABI call takes `start`, every kernel takes `stop` (the last
// one's stands) -- instead of extra marker packets queued around the call.
struct LaunchEvents {
  hipEvent_t start = nullptr, stop = nullptr;
};
LaunchEvents& launch_events();

template <typename F, typename... Args>
inline void launch_kernel(F kernel, const dim3& grid, const dim3& block, uint32_t shmem, hipStream_t st,
                          Args... args) {
  LaunchEvents& ev = launch_events();
  if (!ev.start && !ev.stop) {
    hipLaunchKernelGGL(kernel, grid, block, shmem, st, args...);
    return;
  }
  hipEvent_t start = ev.start;
  ev.start = nullptr;
  hipExtLaunchKernelGGL(kernel, grid, block, shmem, st, start, ev.stop, 0u, args...);
}

struct SelfArgs {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t ldq, ldk, ldv, ldo;  // token strides (elements)
  int64_t bsq, bsk, bsv, bso;  // batch strides (elements)
  int N, P, K, H;
  float scale_log2;            // CrossAttention.scale * log2(e)
  int n_qtiles;
  float* store;                // AttentionStore maps [*, P, K] (or materialised probs)
  const float* probs;          // MODE_PV input [N*H, P, K]
  const uint8_t* key_mask;     // optional [N, K]
  int store_accumulate;
  int variant;                 // a Variant of p2p_select.h (P2P_SELF_VARIANT, experiments build only), else 0
  float* lse;                  // optional [N*H, P] row log-sum-exp output (fused mode, autograd)
  int qk_src[P2P_MAX_BATCH];
  int store_slot[P2P_MAX_BATCH];
  int n_maps;                  // self_maps_kernel: entries in map_entry
  int map_entry[P2P_MAX_BATCH];  // self_maps_kernel: the stored entries (store_slot >= 0)
};

// mutual_attn_kernel (p2p_mutual.hip): its own arguments, SelfArgs stays as it is
struct MutualArgs {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t ldq, ldk, ldv, ldo;  // token strides (elements)
  int64_t bsq, bsk, bsv, bso;  // batch strides (elements)
  int N, P, K, H;              // (P == K)
  float scale_log2;
  int n_qtiles;                // launcher-filled
  const uint8_t* token_class;  // optional [N, P], 0 or 1 per token
  int n_active;                // entries in ent
  int ent[P2P_MAX_BATCH];      // the entries that run (kv_src >= 0), ascending
  int kv_src[P2P_MAX_BATCH];   // per entry: whose K and V it reads, -1 = skipped
};

struct CrossArgs {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t ldq, ldk, ldv, ldo;
  int64_t bsq, bsk, bsv, bso;
  int N, P, K, H;
  float scale_log2;
  int n_qtiles;
  int n_groups;                  // prompt groups (grp_* entries)
  float* store;
  int store_accumulate;
  int any_store;                 // some entry stores its maps
  int edit_terms;                // some group edits through the term planes (LDS gather)
  int edit_dense;                // some group carries the dense f16 mapper tile
  int slab;                      // launcher-filled: the launch allocates the LDS slab
  int slab_stride;               // launcher-filled
  int variant;                   // a Variant of p2p_select.h (P2P_SELF_VARIANT, experiments build only), else 0
  int store_slot[P2P_MAX_BATCH];
  int ent_group[P2P_MAX_BATCH];  // prompt group of every batch entry
  // per entry, packed so ONE kernel-argument load after n decides the path: group (bits 0-7),
  // position in the group (8-15), edits (16), keeps its maps (17), dense edit whose group is
  // flagged P2P_GROUP_F_R_ONLY (18)
  int ent_info[P2P_MAX_BATCH];
  int grp_first[P2P_MAX_GROUPS];
  int grp_count[P2P_MAX_GROUPS];
  const void* grp_prog[P2P_MAX_GROUPS];
  const void* grp_dense[P2P_MAX_GROUPS];   // the program's dense f16 tiles (host-computed offset)
  const float* grp_alpha[P2P_MAX_GROUPS];
  int grp_flags[P2P_MAX_GROUPS];
  float* grp_bsum[P2P_MAX_GROUPS];         // LocalBlend word sums (p2p_group.blend_*)
  const float* grp_balpha[P2P_MAX_GROUPS];
  const float* grp_bsub[P2P_MAX_GROUPS];
  int grp_bcol[P2P_MAX_GROUPS];
  int grp_blh[P2P_MAX_GROUPS];
};

// The kernel a launch runs (p2p_select.h) from its arguments: what run_self / run_cross launch and
// what the p2p_*_attn_kernel queries name.  A SelfKernel / CrossKernel, or a negative P2P_E_* code.
inline int select_self(const SelfArgs& a, int io_dtype, int compute, int d, int mode) {
  return select_self(io_dtype, compute, d, a.P, a.K, mode, a.lse != nullptr, a.n_maps > 0, a.variant);
}
inline int select_cross(const CrossArgs& a, int io_dtype, int compute, int d) {
  return select_cross(io_dtype, compute, d, a.n_groups, a.H, a.P, a.K, a.edit_terms != 0, a.edit_dense != 0,
                      a.any_store != 0, a.variant);
}

// select, then launch (p2p_dispatch.hip)
int run_self(const SelfArgs& a, int io_dtype, int compute, int d, int mode, hipStream_t st);
int run_cross(const CrossArgs& a, int io_dtype, int compute, int d, hipStream_t st);

// The kernel files' launchers: "launch this form with these arguments", no decisions.
// self_attn_fused_kernel / self_pv_kernel (p2p_self.hip)
int launch_self_fused(const SelfArgs& a, int prec, int d, SelfKernel k, hipStream_t st);
// self_attn_multi_kernel (p2p_selfmulti.hip): d = 40, bf16 / f32 inputs
int launch_self_multi(const SelfArgs& a, SelfKernel k, hipStream_t st);
// self40_kernel (p2p_self40.hip): d = 40 / 80, bf16 / fp16 inputs, O only
int launch_self40(const SelfArgs& a, SelfKernel k, hipStream_t st);
// self_split_kernel / self_halves_kernel / self_ring_kernel (p2p_selfsplit.hip): d = 160, bf16, O only
int launch_self_split(const SelfArgs& a, SelfKernel k, hipStream_t st);
// self_wide_kernel (p2p_selfwide.hip): d = 512, bf16 / fp16 inputs, O only
int launch_self_wide(const SelfArgs& a, int prec, hipStream_t st);
// mutual_attn_kernel (p2p_mutual.hip): select_mutual, then launch; and the token classes it reads
int run_mutual(const MutualArgs& a, int io_dtype, int compute, int d, hipStream_t st);
int launch_mutual(const MutualArgs& a, int prec, int d, MutualKernel k, hipStream_t st);
int run_token_classes(const p2p_token_classes_args& a, hipStream_t st);   // every argument check is in here
// AttentionStore epilogue of the self layers whose maps are kept (p2p_selfmaps.hip): p = exp2(c s -
// lse) for the entries a.map_entry[0 .. n_maps) (a.lse filled by a preceding MODE_FUSED_ launch)
int run_self_maps(const SelfArgs& a, int io_dtype, int compute, int d, hipStream_t st);
// materialise protocol: probs (a.store) [N*H, P, K] = softmax(Q K^T * scale), optional key mask
int run_self_probs(const SelfArgs& a, int io_dtype, int compute, int d, hipStream_t st);
// cross_attn_kernel, one workgroup per entry (p2p_cross_entry.hip)
int launch_cross_entry(const CrossArgs& a, int prec, int d, CrossKernel k, hipStream_t st);
// cross_group_kernel, one workgroup per prompt group (p2p_cross.hip): bf16 inputs and compute
int launch_cross_group(const CrossArgs& a, int d, CrossKernel k, hipStream_t st);
int run_localblend(const p2p_blend_args& a, hipStream_t st);
int run_latent_step(const p2p_latent_step_args& a, hipStream_t st);
int run_plms_step(const p2p_plms_step_args& a, hipStream_t st);
int run_dpm_step(const p2p_dpm_step_args& a, hipStream_t st);
int run_direct_step(const p2p_direct_step_args& a, hipStream_t st);
int run_direct_offset(const p2p_direct_offset_args& a, hipStream_t st);
int run_ddpm_step(const p2p_ddpm_step_args& a, hipStream_t st);
int run_ddpm_noise(const p2p_ddpm_noise_args& a, hipStream_t st);

// attention backward (p2p_bwd.hip)
struct BwdArgs {
  const void *q, *k, *v, *o, *dout;
  void *dq, *dk, *dv;          // dq in IO dtype; dk/dv f32 accumulators when kv_split > 1 else IO dtype
  const float* lse;            // [N*H, P] from the forward
  float* delta;                // workspace [N*H, P]
  int64_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;   // token strides (elements)
  int64_t bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv;   // batch strides (elements)
  int N, P, K, H;
  float scale, scale_log2;
  int n_tiles;                 // launcher-filled
  int kv_split;                // query splits of the dK/dV pass (>1: partials in ws, then a reduction)
  int kv_f32;                  // dk/dv are f32 buffers
  float* ws;                   // [2 (dK, dV)][kv_split][N][K][H*D] f32 partials when kv_split > 1
};
// the head dims with compiled backward kernels (dispatch_bwd's cases)
#define P2P_FOR_EACH_BWD_D(X) X(40) X(64) X(80) X(160)
inline bool bwd_head_dim_compiled(int d) {
  switch (d) {
#define P2P_CASE(DD) case DD:
    P2P_FOR_EACH_BWD_D(P2P_CASE)
#undef P2P_CASE
    return true;
    default: return false;
  }
}
int run_attn_bwd(const BwdArgs& a, int io_dtype, int d, hipStream_t st);
int bwd_kv_split(int N, int H, int P, int K, int d);   // launcher's query split (workspace sizing)
int run_store_scale(const float* src, float* dst, float divisor, int64_t n, hipStream_t st);
// U-Net glue (p2p_unet.hip): every argument check happens in these, before the first launch
constexpr int64_t kGnStatsWide = 32768;   // slab elements from which the statistics kernel runs 1024 threads
// Slab elements from which the statistics run in the split form (one workgroup per chunk, then a
// combine launch).  It has to lie strictly above the U-Net's largest slab, 30 channels x 4096
// pixels = 122,880 elements, so that every U-Net launch stays on gn_stats_kernel and keeps its bits.
// Timed against the one-workgroup form on the VAE decoder's norms (statistics + apply, same box,
// runs alternated, profiles/r09/vae/gn_stats.txt): 262,144 elements 34.1 -> 22.1 us, 524,288
// 58.2 -> 33.3, 1,048,576 130 -> 55, 2,097,152 246 -> 97; the split form is taken from the smallest
// of these (sizes between it and 122,880 do not occur in the VAE and were not timed).
constexpr int64_t kGnStatsSplit = 262144;
constexpr int64_t kGnStatsChunk = 32768;   // target elements per chunk (a 1024-thread sweep, as kGnStatsWide)
constexpr int kGnStatsMaxChunks = 256;
// chunks of a slab: a function of its size only (never of the device), 1 = the one-workgroup form
constexpr int gn_stats_chunks(int64_t slab) {
  if (slab < kGnStatsSplit) return 1;
  const int64_t c = (slab + kGnStatsChunk - 1) / kGnStatsChunk;
  return (int)(c > kGnStatsMaxChunks ? kGnStatsMaxChunks : c);
}
// f32 elements of p2p_group_norm_args.stats: {mean, rstd} per slab, then the split form's partials
constexpr int64_t gn_stats_floats(int64_t slabs, int64_t slab) {
  const int c = gn_stats_chunks(slab);
  return slabs * 2 + (c > 1 ? slabs * c * 3 : 0);
}
int run_group_norm(const p2p_group_norm_args& a, hipStream_t st);
int run_bias_residual(const p2p_bias_residual_args& a, hipStream_t st);
int run_geglu(const p2p_geglu_args& a, hipStream_t st);
// the resnets' 3x3 convolution: checks and selection (p2p_dispatch.hip), conv3x3_kernel and its
// reduce launch (p2p_conv.hip), and the once-per-model weight repack
int run_conv3x3(const p2p_conv3x3_args& a, hipStream_t st);   // forwards to run_conv3x3_ex
int run_conv3x3_ex(const p2p_conv3x3_ex_args& a, hipStream_t st);
int launch_conv3x3(const p2p_conv3x3_ex_args& a, int out_h, int out_w, const ConvPlan& plan, hipStream_t st);
int run_conv3x3_pack(const p2p_conv3x3_pack_args& a, hipStream_t st);
int set_conv3x3_loop(int loop);   // p2p_conv3x3_set_loop: a ConvLoop, or P2P_E_ARG
// the feed-forward GEMMs: checks and selection (p2p_dispatch.hip), linear_kernel and its reduce
// launch (p2p_linear.hip)
int run_linear(const p2p_linear_args& a, hipStream_t st);
int launch_linear(const p2p_linear_args& a, const LinearPlan& plan, hipStream_t st);
// the glue's backward.  From kGnBwdWideRow pixels a channel's row of the NCHW reduce takes a whole
// workgroup (four waves), below it one wave; token-major dy leaves one partial per 64-pixel tile.
constexpr int kGnBwdWideRow = 2048;
constexpr int kGnBwdTile = 64;   // the transpose tile's pixels (kTile of p2p_unet.hip)
// f32 elements of p2p_group_norm_bwd_args.workspace: {sum g, sum g xh} per (n, channel, part) for
// the layout with the most parts, then {m1, m2} per slab
constexpr int64_t gn_bwd_workspace_floats(int64_t n, int64_t channels, int64_t hw, int64_t groups) {
  return 2 * n * channels * ((hw + kGnBwdTile - 1) / kGnBwdTile) + 2 * n * groups;
}
int run_group_norm_bwd(const p2p_group_norm_bwd_args& a, hipStream_t st);
int run_geglu_bwd(const p2p_geglu_bwd_args& a, hipStream_t st);
int run_nchw_to_tokens(const p2p_nchw_to_tokens_args& a, hipStream_t st);
// the time path (p2p_unet.hip): every argument check happens in these, before the launch
int run_time_embed(const p2p_time_embed_args& a, hipStream_t st);
int run_time_proj(const p2p_time_proj_args& a, hipStream_t st);
// the image ends (p2p_image.hip): every argument check happens in these, before the launch
int run_image_u8(const p2p_image_u8_args& a, hipStream_t st);
int run_image_to_model(const p2p_image_to_model_args& a, hipStream_t st);
// the text encoders' kernels (p2p_text.hip).  text_attn_kernel: head dim 64, T <= P2P_MAX_KEYS_CROSS
// tokens, bf16 / fp16 inputs (p2p_causal_attn_fwd and p2p_text_attn_fwd check all of it before
// filling these)
struct TextAttnArgs {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t ldq, ldk, ldv, ldo;  // token strides (elements)
  int64_t bsq, bsk, bsv, bso;  // batch strides (elements)
  int N, T, H;
  float scale_log2;            // scale * log2(e)
  const int32_t* key_counts;   // bidirectional only: null, or N device counts (clamped into [1, T])
};
int run_text_attn(const TextAttnArgs& a, bool causal, int io_dtype, hipStream_t st);
// every argument check happens in these, before the launch
int run_layer_norm(const p2p_layer_norm_args& a, hipStream_t st);
int run_bias_act(const p2p_bias_act_args& a, bool erf, hipStream_t st);   // quick-GELU, or the erf GELU
// the attention-map figures (p2p_viz.hip): every argument check happens in these, before the launch
int run_maps_aggregate(const p2p_maps_aggregate_args& a, hipStream_t st);
int run_map_panels(const p2p_map_panels_args& a, hipStream_t st);
// batched null-text inversion (p2p_null.hip): every argument check happens in these, before the launch
int run_null_loss(const P2PNullLossArgs& a, hipStream_t st);
int run_null_adam(const P2PNullAdamArgs& a, hipStream_t st);
int run_clock_probe(unsigned long long* out, int n_wg, int ticks, hipStream_t st);

}  // namespace p2p
