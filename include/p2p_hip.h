/*
 * p2p_hip.h -- C ABI of the MI355X (gfx950) Prompt-to-Prompt attention-control library.
 *
 * Every entry point replaces one call site of the reference's attention-control hot path
 * (KIMGEONUNG/prompt-to-prompt; file:line below).  Conventions:
 *   - all tensor pointers are DEVICE pointers, row-major, caller-owned; the library never
 *     allocates, never synchronises, and launches on the given stream only;
 *   - small per-call tables (batch index maps, group lists) are HOST arrays, copied into the
 *     kernel arguments (no device upload per call);
 *   - the return value is 0 on success, a hipError_t value (> 0) on a launch failure, or a
 *     negative P2P_E_* code when the arguments are rejected before anything is launched.
 *   - q/k/v/o use the projection layout [n_batch, tokens, n_heads * head_dim] (the to_q /
 *     to_k / to_v outputs); the head split of ptp_utils.py:191-193 and the merge of :207 are
 *     done by strides, not copies.
 */
#ifndef P2P_HIP_H
#define P2P_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2P_ABI_VERSION 16
#define P2P_MAX_BATCH 64  /* entries per launch (U-Net batch: 2 x prompts x groups)   */
#define P2P_MAX_GROUPS 32 /* prompt groups per cross-attention launch                 */
#define P2P_MAX_KEYS_CROSS 96
#define P2P_PROGRAM_COLS 128 /* column stride of an edit program (>= n_key)          */
#define P2P_PROGRAM_TMAX 8   /* term planes per edit (source words per target word)  */
/* bytes of one edit's record: c_rep f32[COLS] | post f32[COLS] | {i32 row, f32 val}[TMAX][COLS] */
#define P2P_PROGRAM_REC_BYTES (2 * 4 * P2P_PROGRAM_COLS + 8 * P2P_PROGRAM_TMAX * P2P_PROGRAM_COLS)
#define P2P_PROGRAM_HEADER_BYTES 32
#define P2P_PROGRAM_DENSE 96 /* dense mapper tile: f16 [DENSE][DENSE] per edit              */
enum {
  P2P_PROGRAM_F_DENSE = 1, /* p2p_group.flags: the program carries the dense f16 tile           */
  /* p2p_group.flags (ABI 14), a per-call hint: for this call's alpha row every edit's blend
   * coefficient A[w] = alpha[w] * post[w] * c_rep[w] + 1 - alpha[w] is 0 (a Replace or Reweight
   * step inside cross_replace_steps, main.py:189), so P_e' = R and the edit entries' own Q K^T
   * softmax, Q and K are not needed -- the bf16 dense kernels then load only their V.  The
   * kernel re-derives A from the program and falls back to the full edit if the hint is wrong. */
  P2P_GROUP_F_R_ONLY = 2,
  /* p2p_group.flags (ABI 15), a caller guarantee, also for groups without a program: every entry
   * of the group has the SAME K and V values as its first entry (the uncond prompts "" of a group,
   * ptp_utils.py:150-156, whose context rows are equal).  The group kernel then stages them once
   * per workgroup instead of per entry; results are bit-identical when the guarantee holds. */
  P2P_GROUP_F_SHARED_KV = 4
};

/* Element types of q, k, v, o (and of the latent step's eps).  P2P_DTYPE_F16 (ABI 16): IEEE
 * binary16, what a Stable Diffusion model loaded with torch_dtype=torch.float16 produces. */
enum { P2P_DTYPE_F32 = 0, P2P_DTYPE_BF16 = 1, P2P_DTYPE_F16 = 2 };
/* P2P_COMPUTE_BF16 names the 16-bit MFMA pipe; the operand format follows the inputs: bf16
 * MFMAs for bf16 (and, split, for f32) inputs, f16 MFMAs for f16 inputs (the name predates
 * ABI 16 and is kept).  P2P_COMPUTE_F32 is the exact-f32 check mode, f32 inputs only: bf16 or
 * f16 inputs with it are rejected (P2P_E_DTYPE). */
enum { P2P_COMPUTE_BF16 = 0, P2P_COMPUTE_F32 = 1 };

enum {
  P2P_E_ARG = -1,       /* null pointer / inconsistent sizes                             */
  P2P_E_HEAD_DIM = -2,  /* head_dim without a compiled kernel                             */
  P2P_E_DTYPE = -3,     /* io_dtype / compute combination not supported                   */
  P2P_E_KEYS = -4,      /* n_key above P2P_MAX_KEYS_CROSS for the cross kernel            */
  P2P_E_BATCH = -5,     /* n_batch above P2P_MAX_BATCH or group list inconsistent         */
  P2P_E_ALIGN = -6      /* a pointer / stride breaks the 16-byte vector-load alignment    */
};

typedef void* p2p_stream_t; /* a hipStream_t */

/* One attention call: q [n_batch, n_query, *], k/v [n_batch, n_key, *], o like q.
 * Strides are in elements.  scale is CrossAttention.scale (head_dim ** -0.5,
 * ptp_utils.py:195).
 *
 * Operand layout contract.  An operand is a view: element (n, row, c) is at
 * base + n * batch_stride + row * row_stride + c, c < n_heads * head_dim, unit last stride -- so
 * q, k, v may be column slices of one fused projection ([n, tokens, 3C] / [n, n_key, 2C]: row
 * stride 3C / 2C, bases C apart), padded rows, or one entry broadcast (batch stride 0).  For every
 * operand the call needs (a call that takes no v or no q ignores its strides but for alignment):
 *   - pointers and strides are multiples of 16 bytes, else P2P_E_ALIGN;
 *   - row stride >= n_heads * head_dim (rows do not overlap; no negative strides);
 *   - batch stride >= 0; 0 is legal on q, k, v;
 *   - for o with n_batch > 1, batch stride >= (n_query - 1) * o_row_stride + n_heads * head_dim
 *     (entries do not overlap: every element of o has one writer);
 *   - the span ((rows - 1) * row_stride + n_heads * head_dim) * element size <= INT32_MAX, rows =
 *     n_query for q and o, n_key for k and v (the kernels index inside an entry with 32-bit byte
 *     offsets);
 * else P2P_E_ARG, before anything is launched (checked after the call's other arguments).  The
 * kernels read nothing they use, and write nothing at all, outside the elements of the views:
 * row padding, the slack between entries and the columns of a fused projection that belong to
 * another operand keep their bits (tests/test_gpu_layouts.py). */
typedef struct {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t q_row_stride, k_row_stride, v_row_stride, o_row_stride;
  int64_t q_batch_stride, k_batch_stride, v_batch_stride, o_batch_stride;
  int32_t n_batch, n_query, n_key, n_heads, head_dim;
  int32_t io_dtype; /* P2P_DTYPE_*  (element type of q, k, v, o)                      */
  int32_t compute;  /* P2P_COMPUTE_* (16-bit MFMA pipe, or exact-f32 MFMA check mode)   */
  float scale;
} p2p_attn_tensors;

/* Self-attention (ptp_utils.py:183-208 with context=None) fused with the controller's
 * self-attention edit and the AttentionStore epilogue:
 *   O[n] = softmax(Q[qk_src[n]] K[qk_src[n]]^T * scale) V[n]
 * qk_src (host, n_batch entries, NULL = identity) implements the source-map injection of
 * AttentionControlEdit.replace_self_attention (main.py:169-174, null_text.py:224-230): an
 * edit inside the self_replace window reads the SOURCE prompt's probabilities and its OWN
 * values.  store (nullable) receives the normalised probabilities of every entry whose
 * store_slot (host) is >= 0 at maps [store_slot[n] + head] of a [*, n_query, n_key] f32
 * tensor, overwritten (store_accumulate = 0, first step) or added (= 1): the running sum
 * of AttentionStore.between_steps (main.py:135-142).  lse_workspace: f32
 * [n_batch * n_heads, n_query] scratch, required (16-byte aligned) when some entry stores its
 * maps, else ignored: the fused pass leaves each row's log-sum-exp there and the map pass
 * recomputes the probabilities from it. */
int p2p_self_attn_fwd(const p2p_attn_tensors* t, const int32_t* qk_src, float* store,
                      const int32_t* store_slot, int32_t store_accumulate, float* lse_workspace,
                      p2p_stream_t stream);

/* A prompt group of a cross-attention launch: entries [first, first + count) of the batch;
 * entry `first` is the source prompt, the others its edits (main.py:187).  program is the
 * device edit program or NULL
 * for no edit; alpha is the device [count - 1][n_key] row cross_replace_alpha[cur_step]
 * (main.py:189).  Program layout (p2p_amd/programs.py): int32 header[8] {n_edits, n_cols, tmax,
 * P2P_PROGRAM_COLS, dense, dense_offset, 0, 0}, then per edit e at byte
 * P2P_PROGRAM_HEADER_BYTES + e * P2P_PROGRAM_REC_BYTES: c_rep f32[COLS],
 * post f32[COLS], term planes {i32 row, f32 val}[P2P_PROGRAM_TMAX][COLS] -- plane t of column
 * w is the t-th source row feeding target word w, (0, 0.0) past its last term; tmax <= TMAX is
 * the number of planes the kernel walks:
 *   R[w] = post[w] * (c_rep[w] * P_e[w] + sum_{t < tmax} val[t][w] * P_0[row[t][w]])
 *   P_e'[w] = alpha[w] * R[w] + (1 - alpha[w]) * P_e[w]
 * When every term value is exact in f16 the program also holds, at byte dense_offset, the
 * dense mapper of each edit as f16 [P2P_PROGRAM_DENSE rows (source word)][P2P_PROGRAM_DENSE
 * cols (target word)] (zeros elsewhere), and the host sets P2P_PROGRAM_F_DENSE in flags: the
 * bf16 kernels then form sum_t val * P_0[row] as one f16 MFMA product P_0 . M_e (P_0 rounded
 * to 11 significant bits, <= 2^-12 relative) instead of an LDS gather.  (ABI 12: f16 tile.)  */
typedef struct {
  int32_t first;
  int32_t count;
  const void* program;
  const float* alpha;
  int32_t flags;   /* P2P_PROGRAM_F_* of program (host-known: sizes the launch's LDS) */
  int32_t n_edits; /* edit records the program holds (its header[0]); a group with
                      count - 1 > n_edits is rejected (P2P_E_BATCH) before any launch */
  /* LocalBlend's word reduction folded into the store epilogue (null_text.py:41-46,
   * main.py:37-44: (maps * alpha).sum(-1) of the five 16x16 cross layers), nullable: for entry
   * b of the group, head h and query row p
   *   blend_sums[((b * 2 + s) * blend_lh + blend_col + h) * n_query + p]  = / +=
   *       sum_w P'[p][w] * alpha_s[b][w],   alpha_0 = blend_alpha, alpha_1 = blend_sub (or 0)
   * with P' the post-edit probabilities the store receives, written when store_accumulate = 0
   * and added otherwise -- the running sum of the word sums, which is what p2p_localblend
   * (word_sums_ready) reads instead of re-reading the maps.  Needs every entry of the group to
   * store (store_slot >= 0). */
  float* blend_sums;
  const float* blend_alpha; /* [count][n_key] f32                                          */
  const float* blend_sub;   /* [count][n_key] f32 or NULL                                  */
  int32_t blend_col;        /* this layer's first column (layer index * n_heads)            */
  int32_t blend_lh;         /* columns of the sums: blended layers * n_heads                */
} p2p_group;

/* Cross-attention (ptp_utils.py:183-208 with context=...) with the controller's cross edit
 * applied in registers between softmax and PV (AttentionControlEdit.forward, main.py:180-197:
 * Replace :217-218, Refine :235-239, Reweight :258-264) and the AttentionStore epilogue
 * (store/store_slot/store_accumulate as for p2p_self_attn_fwd; stored maps are the
 * post-edit probabilities, as the reference's aliasing store holds). */
int p2p_cross_attn_fwd(const p2p_attn_tensors* t, const p2p_group* groups, int32_t n_groups,
                       float* store, const int32_t* store_slot, int32_t store_accumulate,
                       p2p_stream_t stream);

/* Which kernel the two calls above would launch: the same validation and the same selection
 * (csrc/p2p_select.h), nothing launched and no pointer dereferenced beyond t and groups.  Returns
 * the kernel's name as DESIGN.md §4 writes it ("self40_kernel<40,8,2,256>"; "…" stands for the
 * precision's template arguments and D for head_dim), a static string, or NULL where the forward
 * call would be rejected.  keeps_maps: some entry has store_slot >= 0 (p2p_self_attn_fwd with a
 * store); wants_lse without keeps_maps: p2p_attn_fwd_lse; any_store: some entry of the cross call
 * keeps its maps.  (Additive; ABI 16.) */
const char* p2p_self_attn_kernel(const p2p_attn_tensors* t, int32_t keeps_maps, int32_t wants_lse);
const char* p2p_cross_attn_kernel(const p2p_attn_tensors* t, const p2p_group* groups,
                                  int32_t n_groups, int32_t any_store);

/* Mutual self-attention (MasaCtrl, Cao et al. 2023, §3.2-3.3).  n_query == n_key.
 *   s = kv_src[n]  (host, n_batch entries, NULL = identity);  s < 0: entry n is skipped, o[n] keeps its bits
 *   O[n] = softmax(Q[n] K[s]^T * scale + M) V[s]
 * token_class (device, nullable): uint8 [n_batch, n_query], 0 or 1 per token.  For s != n and a
 * non-null token_class, key j is admitted for query p iff token_class[s][j] == token_class[n][p];
 * a query whose class has NO key in entry s admits every key (unrestricted attention, never a
 * uniform or NaN row).  M = 0 on admitted keys, -inf elsewhere.  s == n: plain self-attention.
 * Rejected before anything is launched or dereferenced: a null operand or n_query != n_key
 * (P2P_E_ARG), kv_src[n] >= n_batch or n_batch > P2P_MAX_BATCH (P2P_E_BATCH), and what
 * p2p_self_attn_fwd rejects for the same tensors (the operand layout contract above, batch stride
 * 0 and fused-projection views included).  O only: nothing is stored, no lse.  Every precision and
 * every compiled head dim.  (Additive; ABI 16.) */
int p2p_mutual_attn_fwd(const p2p_attn_tensors* t, const int32_t* kv_src,
                        const uint8_t* token_class, p2p_stream_t stream);
/* The kernel p2p_mutual_attn_fwd would launch (csrc/p2p_select.h, select_mutual), as
 * p2p_self_attn_kernel reports the self kernels; masked: the call carries token classes. */
const char* p2p_mutual_attn_kernel(const p2p_attn_tensors* t, int32_t masked);

/* The token classes p2p_mutual_attn_fwd reads, from the running word sums the cross store epilogue
 * folds (p2p_group.blend_sums with a one-hot alpha row on the object word(s) of each prompt).  Per
 * prompt b of group g: the mean over the lh maps of plane 0 (sums[g][b][0][l][*], in index order),
 * min-max normalised over the res^2 pixels, class = (value >= threshold); a constant map (max ==
 * min) is class 0 everywhere.  The res x res classes are nearest-resized to each side[r] and
 * written to row n_groups * group_size * cfg + g * group_size + b of out[r] (uint8 [n_batch,
 * side[r]^2]) and, with cfg = 1, to row g * group_size + b as well: the uncond entry of a prompt
 * gets its cond entry's row.  No host read, no allocation: capture-safe.
 * Rejected before the launch: a null pointer, n_groups outside [1, P2P_MAX_GROUPS], group_size,
 * lh or res < 1, res^2 > 1024, n_res outside [1, 3], a side outside [1, 1024], a NaN threshold
 * (P2P_E_ARG); more than P2P_MAX_BATCH rows (P2P_E_BATCH); sums off 4 bytes (P2P_E_ALIGN). */
typedef struct {
  const float* sums[P2P_MAX_GROUPS]; /* per group [group_size, 2, lh, res^2] f32 (plane 0 is read) */
  int32_t n_groups, group_size, lh, res;
  float threshold;
  int32_t cfg;                       /* 1: out has the uncond rows in front of the cond rows   */
  int32_t n_res;
  int32_t side[3];
  uint8_t* out[3];
} p2p_token_classes_args;
int p2p_token_classes(const p2p_token_classes_args* a, p2p_stream_t stream);

/* Materialise mode, for controllers that override forward(attn, ...) (the reference
 * protocol, main.py:85-98): probs[n*H + h] = softmax(Q K^T * scale) as an f32
 * [n_batch * n_heads, n_query, n_key] tensor (ptp_utils.py:195-204).  key_mask (nullable,
 * uint8 [n_batch, n_key], nonzero = keep) reproduces ptp_utils.py:197-201, including its
 * head-major repeat of the mask rows: a masked key scores -FLT_MAX after the scale, so it gets
 * p = 0 beside any kept key and a fully masked row is uniform, 1/n_key. */
int p2p_attn_probs(const p2p_attn_tensors* t, const uint8_t* key_mask, float* probs,
                   p2p_stream_t stream);

/* Materialise mode, second half: O[n] = probs[n*H + h] V[n] (ptp_utils.py:206-207). */
int p2p_attn_pv(const p2p_attn_tensors* t, const float* probs, p2p_stream_t stream);

/* Attention with its gradient -- what null-text inversion needs (null_text.py:574-606: Adam on
 * the null embedding through every patched attention of the U-Net).  Forward: O as
 * p2p_self_attn_fwd with no controller edit, plus lse [n_batch * n_heads, n_query] f32, the row
 * log-sum-exp in the log2 domain with the scale folded in (softmax row = exp2(scale * log2(e) *
 * s - lse)).  Any n_key (self- or cross-attention); bf16 compute only, f32 or bf16 tensors
 * (P2P_DTYPE_F16 is rejected with P2P_E_DTYPE here and by the backward: ABI 16). */
int p2p_attn_fwd_lse(const p2p_attn_tensors* t, float* lse, p2p_stream_t stream);

/* Backward of O = softmax(Q K^T * scale) V for the same tensors (t->o = the forward's O):
 *   dV = P^T dO,  dS = P o (dO V^T - rowsum(dO o O)),  dQ = scale dS K,  dK = scale dS^T Q.
 * dout is read with t->o's row and batch strides, dq is written with t->q's (elements past
 * n_heads * head_dim of a dq row are left alone); dk, dv are packed [n_batch, n_key,
 * n_heads * head_dim], written (not accumulated) in io_dtype, or in f32 when kv_f32 = 1.
 * delta: workspace [n_batch * n_heads, n_query] f32.  workspace: p2p_attn_bwd_workspace(t)
 * bytes (NULL when that is 0): when the key tiles alone would leave the chip idle (cross
 * attention, small batches) the key/value pass splits the queries over workgroups, each split
 * stores its partial dK/dV there and a reduction adds them in split order -- deterministic,
 * no atomics.  P is recomputed from lse; bf16 MFMA operands, f32 accumulation. */
int64_t p2p_attn_bwd_workspace(const p2p_attn_tensors* t);
int p2p_attn_bwd(const p2p_attn_tensors* t, const void* dout, const float* lse, float* delta, void* dq,
                 void* dk, void* dv, int32_t kv_f32, void* workspace, int64_t workspace_bytes,
                 p2p_stream_t stream);

/* LocalBlend (null_text.py:41-70; main.py:35-52 is the B=2 special case) for one prompt
 * group: maps[l] are the running-sum cross maps of the blended layers (Stable Diffusion: the
 * five 16x16 layers down_cross[2:4] + up_cross[:3]), each [n_prompts * heads_per_map,
 * map_res^2, n_words] f32.  Served, and tested at their edges (tests/test_gpu_blend_geometry.py):
 * 1 <= n_prompts <= 16, 1 <= n_maps <= 8, n_words <= 128, map_res^2 <= 256 (any map_res, odd
 * ones included), any heads_per_map >= 1 and any lat_h, lat_w >= 1 -- larger or smaller than
 * map_res, square or not (nearest resampling as F.interpolate's); anything else is P2P_E_ARG. */
typedef struct {
  const float* maps[8];
  int32_t n_maps;
  int32_t heads_per_map;
  int32_t n_prompts;
  int32_t n_words;
  int32_t map_res;                 /* maps are map_res x map_res; map_res^2 <= 256     */
  const float* alpha_layers;       /* [n_prompts, n_words]                             */
  const float* substruct_layers;   /* [n_prompts, n_words] or NULL                     */
  float th_pool, th_sub;           /* th[0], th[1] (main form: threshold, unused)      */
  float* x_t;                      /* [n_prompts, channels, lat_h, lat_w] in/out       */
  int32_t channels, lat_h, lat_w;
  float* word_sums;                /* workspace [n_prompts, 2, n_maps*heads, res*res]  */
  uint8_t* mask_out;               /* optional [n_prompts, lat_h, lat_w] final mask    */
  int32_t word_sums_ready;         /* 1: word_sums already hold the word reductions (the
                                      running sums folded by p2p_cross_attn_fwd's
                                      blend_sums); maps are then not read (may be NULL)   */
} p2p_blend_args;

/* x_t may be NULL when mask_out is given: the mask is computed and nothing is blended (the
 * latent blend then happens inside p2p_latent_step). */
int p2p_localblend(const p2p_blend_args* a, p2p_stream_t stream);

/* One denoising step's latent update, fused (ptp_utils.py:72-75 diffusion_step tail):
 *   noise = eps_u + guidance * (eps_c - eps_u)                      (cfg = 1; else noise = eps)
 *   x0    = (x - sqrt_beta_t * noise) / sqrt_alpha_t                 (null_text.py:475-479:
 *   out   = sqrt_alpha_prev * x0 + sqrt_one_minus_alpha_prev * noise  prev_step; next_step with
 *                                                                      the inversion coefficients)
 *   out[b] = out[g0] + mask[b] * (out[b] - out[g0])  b not a group's  (LocalBlend, mask nullable;
 *                                                    first prompt g0     g0 = first prompt of b's
 *                                                                        group of group_size)
 * eps [cfg ? 2B : B, C, H, W] in eps_dtype (uncond block first, as torch.cat([latents] * 2)),
 * x / out [B, C, H, W] f32 (out may alias x), mask uint8 [B, H, W] (p2p_localblend mask_out).
 * The four coefficients are the host-side 0-dim values the scheduler computes (beta_t ** 0.5 ...).
 * Intermediates are rounded as the reference's eager torch ops round them (bf16 products for a
 * bf16 eps, f16 products for an f16 eps), so the result is bit-identical to the unfused sequence. */
typedef struct {
  const void* eps;
  int32_t eps_dtype;               /* P2P_DTYPE_*                                      */
  int32_t cfg;
  float guidance;
  const float* x;
  float* out;
  int32_t n_prompts, channels, height, width;
  float sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_one_minus_alpha_prev;
  const uint8_t* mask;
  int32_t group_size;              /* prompts per prompt group (0 = one group of n_prompts) */
  const uint8_t* group_blend;      /* [n_prompts / group_size] 1 = blend this group, NULL = all */
  /* LocalBlend in the same launch (one kernel per denoising step): when blend_sums[g] is set,
   * prompt group g's mask is built here from the running word sums the cross-attention store
   * epilogue folded (p2p_group.blend_sums: [group_size, 2, blend_lh, blend_res^2] f32) --
   * mean over the blend_lh layer x head maps, 3x3 max-pool, nearest upsampling, per-image max
   * normalisation, thresholds, mask[:1] | mask and the substruct gate (null_text.py:41-67),
   * exactly as p2p_localblend with word_sums_ready = 1 builds it -- and the blend of
   * null_text.py:68-70 follows.  `mask` must then be NULL; NULL entries do not blend.
   * (ptp_utils.py:75 step_callback + null_text.py:41-70, fused with the CFG/DDIM update.) */
  const float* blend_sums[P2P_MAX_GROUPS];
  int32_t blend_lh;                /* layer x head maps per prompt, any >= 1 (SD: 5 x 8)     */
  int32_t blend_res;               /* map resolution >= 1; res^2 <= 256, res <= height, width;
                                      height * width % 4 == 0; x, out, eps 16-byte aligned;
                                      any channels >= 1 (else P2P_E_ARG, before any launch)  */
  float blend_th_pool, blend_th_sub;
  int32_t blend_sub;               /* 1: the substruct sums (index 1) gate the mask          */
} p2p_latent_step_args;

int p2p_latent_step(const p2p_latent_step_args* a, p2p_stream_t stream);

/* The same latent update for the PLMS sampler (PNDM with skip_prk_steps: the scheduler of the
 * Stable Diffusion v1.4 pipeline main.py:29 loads; p2p_amd/pndm.py), additive to ABI 16:
 *   e     = eps_u + guidance * (eps_c - eps_u)        (cfg = 1, rounded in eps_dtype as above;
 *                                                      else e = eps), upcast to f32
 *   hist_out = e                                      (nullable: the scheduler's eps history)
 *   m     = w[0] * e + w[1] * hist[0] + ... + w[n_hist] * hist[n_hist - 1]
 *                                                     (f32 products summed left to right: the
 *                                                      linear multistep combination, e.g.
 *                                                      (55, -59, 37, -9) / 24 from the fourth call)
 *   out   = sample_coeff * x - (eps_num * m) / eps_den          (one IEEE division)
 * with, for the step from alpha_cumprod a_t to a_p, sample_coeff = sqrt(a_p / a_t), eps_num =
 * a_p - a_t and eps_den = a_t * sqrt(1 - a_p) + sqrt(a_t * (1 - a_t) * a_p): the three host-side
 * 0-dim values of PNDMScheduler.plan_step.  Then the LocalBlend blend of p2p_latent_step, in
 * either form: mask / group_size / group_blend / blend_* mean what they mean there, with the same
 * preconditions (in the blend_sums form also: every hist pointer in use and hist_out 16-byte
 * aligned).  hist[i]: f32 [B, C, H, W], newest first; x is the sample the scheduler steps from (its
 * kept sample on the corrector call).  Every f32 operation is rounded to nearest, none contracted,
 * so out and hist_out are bit-identical to PNDMScheduler.step on the same inputs.
 * Rejected with P2P_E_ARG before any launch: a NULL eps / x / out, n_hist outside 0..4, a NULL
 * hist[i] below n_hist, hist_out equal to a hist[i] in use or to x or out, eps_den == 0. */
typedef struct {
  const void* eps;
  int32_t eps_dtype;               /* P2P_DTYPE_*                                      */
  int32_t cfg;
  float guidance;
  const float* x;
  float* out;                      /* may alias x (not in the blend_sums form)         */
  int32_t n_prompts, channels, height, width;
  const uint8_t* mask;
  int32_t group_size;
  const uint8_t* group_blend;
  const float* blend_sums[P2P_MAX_GROUPS];
  int32_t blend_lh;
  int32_t blend_res;
  float blend_th_pool, blend_th_sub;
  int32_t blend_sub;
  const float* hist[4];            /* stored eps, newest first                         */
  int32_t n_hist;                  /* 0..4 entries of hist used                        */
  float w[5];                      /* w[0]: the new eps; w[1 + i]: hist[i]             */
  float* hist_out;                 /* NULL, or f32 [B, C, H, W]: the new eps           */
  float sample_coeff, eps_num, eps_den;
} p2p_plms_step_args;

int p2p_plms_step(const p2p_plms_step_args* a, p2p_stream_t stream);

/* The same latent update for the DPM-Solver++ (2M) sampler (second-order multistep, data
 * prediction: Lu et al. 2022, Algorithm 2; p2p_amd/dpm.py), additive to ABI 16:
 *   e     = eps_u + guidance * (eps_c - eps_u)        (cfg = 1, rounded in eps_dtype as above;
 *                                                      else e = eps), upcast to f32
 *   m0    = (x - sigma_s * e) / alpha_s               (the data prediction; one IEEE division)
 *   hist_out = m0                                     (nullable: NULL on the last call)
 *   out   = x_coeff * x - m0_coeff * m0               (n_hist = 0: the first-order update)
 *   out   = out - diff_coeff * (m0 - hist[0])         (n_hist = 1: the 2M term, hist[0] the
 *                                                      previous call's m0)
 * with, for the call at timestep s stepping to t (a = sqrt(alpha_cumprod), sg = sqrt(1 -
 * alpha_cumprod), lambda = log a - log sg, h = lambda_t - lambda_s, r0 = (lambda_s - lambda_s') / h,
 * s' the previous call's timestep): sigma_s = sg_s, alpha_s = a_s, x_coeff = sg_t / sg_s, m0_coeff =
 * a_t * expm1(-h), diff_coeff = 0.5 * a_t * expm1(-h) / r0 -- the five host-side values of
 * DPMSolverMultistepScheduler.plan_step, computed in double and rounded once to f32.  Then the
 * LocalBlend blend of p2p_latent_step, in either form: mask / group_size / group_blend / blend_*
 * mean what they mean there, with the same preconditions (in the blend_sums form also: hist[0] in
 * use and hist_out 16-byte aligned).  hist[0], hist_out: f32 [B, C, H, W].  Every f32 operation is
 * rounded to nearest, none contracted, so out and hist_out are bit-identical to
 * DPMSolverMultistepScheduler.step on the same inputs.
 * Rejected with P2P_E_ARG before any launch: a NULL eps / x / out, n_hist outside 0..1, a NULL
 * hist[0] with n_hist = 1, hist_out equal to hist[0] in use or to x or out, alpha_s == 0, and what
 * p2p_latent_step rejects (its geometry and, as there and in p2p_plms_step, a misaligned pointer of
 * the blend_sums form: none of the three step forms answers P2P_E_ALIGN); P2P_E_DTYPE: an unknown
 * eps_dtype. */
typedef struct {
  const void* eps;
  int32_t eps_dtype;               /* P2P_DTYPE_*                                      */
  int32_t cfg;
  float guidance;
  const float* x;
  float* out;                      /* may alias x (not in the blend_sums form)         */
  int32_t n_prompts, channels, height, width;
  const uint8_t* mask;
  int32_t group_size;
  const uint8_t* group_blend;
  const float* blend_sums[P2P_MAX_GROUPS];
  int32_t blend_lh;
  int32_t blend_res;
  float blend_th_pool, blend_th_sub;
  int32_t blend_sub;
  const float* hist[1];            /* the previous call's data prediction              */
  int32_t n_hist;                  /* 0 or 1                                           */
  float* hist_out;                 /* NULL, or f32 [B, C, H, W]: this call's m0        */
  float sigma_s, alpha_s, x_coeff, m0_coeff, diff_coeff;
} p2p_dpm_step_args;

int p2p_dpm_step(const p2p_dpm_step_args* a, p2p_stream_t stream);

/* The DDIM latent update of p2p_latent_step for the edit loop of Direct Inversion (Ju et al. 2023,
 * "Direct Inversion: Boosting Diffusion-based Editing with 3 Lines of Code"; p2p_amd/
 * direct_inversion.py), additive to ABI 16: the update, then the LocalBlend blend, then
 *   out[g0] = out[g0] + offset[g]         g0 the first prompt of prompt group g
 * -- the order of the eager lines (diffusion_step with its step_callback, then the add on the source
 * row): the blend of the rows b != g0 reads the un-offset out[g0].  Every field of
 * p2p_latent_step_args means what it means there, in all three forms (no mask, `mask` with groups,
 * blend_sums), with the same preconditions; offset is f32 [n_prompts / group_size, C, H, W], one row
 * with group_size = 0.  out is bit-identical to p2p_latent_step followed by torch's add.
 * Rejected with P2P_E_ARG before any launch: a NULL offset, an offset that overlaps x or out, and
 * what p2p_latent_step rejects (n_prompts not a multiple of group_size among it; in the blend_sums
 * form a misaligned pointer, offset included -- none of the four step forms answers P2P_E_ALIGN);
 * P2P_E_DTYPE: an unknown eps_dtype. */
typedef struct {
  const void* eps;
  int32_t eps_dtype;               /* P2P_DTYPE_*                                      */
  int32_t cfg;
  float guidance;
  const float* x;
  float* out;                      /* may alias x (not in the blend_sums form)         */
  int32_t n_prompts, channels, height, width;
  float sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev, sqrt_one_minus_alpha_prev;
  const uint8_t* mask;
  int32_t group_size;
  const uint8_t* group_blend;
  const float* blend_sums[P2P_MAX_GROUPS];
  int32_t blend_lh;
  int32_t blend_res;
  float blend_th_pool, blend_th_sub;
  int32_t blend_sub;
  const float* offset;             /* f32 [n_prompts / group_size, C, H, W]            */
} p2p_direct_step_args;

int p2p_direct_step(const p2p_direct_step_args* a, p2p_stream_t stream);

/* Direct Inversion's offsets for R rows in one launch -- R timesteps of one image, or R images:
 *   rec[r]    = prev_step(eps_u[r] + guidance * (eps_c[r] - eps_u[r]), x[r])   with coef[r]
 *   offset[r] = target[r] - rec[r]
 * eps [2R, n] in eps_dtype (uncond block first), x / target / offset f32 [R, n] (n = C * H * W),
 * coef f32 [R, 4] in DEVICE memory: row r's own sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev),
 * sqrt(1 - a_prev) (DDIMScheduler.prev_coeffs), since the rows may be different timesteps and a
 * graph captured once is refilled per call.  Rounded as p2p_latent_step rounds (CFG products in
 * the eps dtype, the rest in f32, nothing contracted): rec[r] is bit-identical to p2p_latent_step
 * without a mask on row r with that row's coefficients, and offset[r] to torch's subtraction.
 * Rejected before anything is launched: a null pointer, R <= 0 or n <= 0 (P2P_E_ARG); an unknown
 * eps_dtype (P2P_E_DTYPE); R > 65535 (P2P_E_BATCH); n % 4 != 0, or eps / x / target / coef /
 * offset off 16 bytes (P2P_E_ALIGN, the rules of p2p_null_loss). */
typedef struct {
  const void* eps;        /* [2R, n] in eps_dtype                                       */
  int32_t eps_dtype;      /* P2P_DTYPE_F32 / P2P_DTYPE_BF16 / P2P_DTYPE_F16             */
  float guidance;
  const float* x;         /* [R, n] the trajectory latent at each row's timestep        */
  const float* target;    /* [R, n] the next cleaner trajectory latent                  */
  const float* coef;      /* [R, 4] f32, device                                         */
  float* offset;          /* [R, n] out                                                 */
  int32_t R, n;
} p2p_direct_offset_args;

int p2p_direct_offset(const p2p_direct_offset_args* a, p2p_stream_t stream);

/* The stochastic (eta > 0) DDIM step with a caller-supplied variance noise, for the edit loop of the
 * edit-friendly DDPM inversion (Huberman-Spiegelglas, Kulikov, Michaeli, CVPR 2024, "An Edit
 * Friendly DDPM Noise Space: Inversion and Manipulations"; p2p_amd/ddpm_inversion.py), additive to
 * ABI 16:
 *   out[b] = mu(x[b], eps[b]) + sigma * noise[g]      g the prompt group of prompt b
 * and then the LocalBlend blend -- the order of scheduler.ddpm_step(..., variance_noise) followed by
 * step_callback: the noise goes to EVERY prompt of the group, before the blend, so the rows b != g0
 * blend towards the noised out[g0] (p2p_direct_step adds its offset to g0 alone, after the blend).
 * mu is p2p_latent_step's update with sqrt_one_minus_alpha_prev carrying
 * sqrt(1 - a_prev - sigma^2) (DDIMScheduler.ddpm_coeffs); sigma * noise is one f32 product, then one
 * f32 sum, nothing contracted.  Every field of p2p_latent_step_args means what it means there, in
 * all three forms (no mask, `mask` with groups, blend_sums), with the same preconditions; noise is
 * f32 [n_prompts / group_size, C, H, W], one row with group_size = 0.  out is bit-identical to the
 * eager lines; with sigma = 0 (legal: the last step of the grid) and a finite noise, to
 * p2p_latent_step with the same four factors.
 * Rejected with P2P_E_ARG before any launch: a NULL noise, a noise that overlaps x or out, a
 * negative or non-finite sigma, and what p2p_direct_step rejects (in the blend_sums form a
 * misaligned pointer, noise included); P2P_E_DTYPE: an unknown eps_dtype. */
typedef struct {
  const void* eps;
  int32_t eps_dtype;               /* P2P_DTYPE_*                                      */
  int32_t cfg;
  float guidance;
  const float* x;
  float* out;                      /* may alias x (not in the blend_sums form)         */
  int32_t n_prompts, channels, height, width;
  float sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev;
  float sqrt_one_minus_alpha_prev; /* sqrt(1 - a_prev - sigma^2)                       */
  const uint8_t* mask;
  int32_t group_size;
  const uint8_t* group_blend;
  const float* blend_sums[P2P_MAX_GROUPS];
  int32_t blend_lh;
  int32_t blend_res;
  float blend_th_pool, blend_th_sub;
  int32_t blend_sub;
  float sigma;                     /* >= 0, finite                                     */
  const float* noise;              /* f32 [n_prompts / group_size, C, H, W]            */
} p2p_ddpm_step_args;

int p2p_ddpm_step(const p2p_ddpm_step_args* a, p2p_stream_t stream);

/* The noise maps of the edit-friendly DDPM inversion for R rows in one launch -- R timesteps of one
 * image, or of several:
 *   mu[r]    = c2 * ((x[r] - c0 * e[r]) / c1) + c3' * e[r]    e = eps_u[r] + guidance * (eps_c[r] - eps_u[r])
 *   noise[r] = c4 > 0 ? (target[r] - mu[r]) / c4 : 0          (one IEEE division)
 * eps [2R, n] in eps_dtype (uncond block first), x / target / noise f32 [R, n] (n = C * H * W),
 * coef f32 [R, 5] in DEVICE memory: row r's own c0 = sqrt(1 - a_t), c1 = sqrt(a_t),
 * c2 = sqrt(a_prev), c3' = sqrt(1 - a_prev - sigma^2), c4 = sigma (DDIMScheduler.ddpm_coeffs), since
 * the rows are different timesteps and a graph captured once is refilled per call.  mu[r] is
 * bit-identical to p2p_ddpm_step without a mask on row r with sigma = 0 and that row's c0 .. c3'.
 * Rejections as p2p_direct_offset's: a null pointer, R <= 0 or n <= 0 (P2P_E_ARG); an unknown
 * eps_dtype (P2P_E_DTYPE); R > 65535 (P2P_E_BATCH); n % 4 != 0, or eps / x / target / coef / noise
 * off 16 bytes (P2P_E_ALIGN; coef's rows of five are read as scalars, only its base is checked). */
typedef struct {
  const void* eps;        /* [2R, n] in eps_dtype                                       */
  int32_t eps_dtype;      /* P2P_DTYPE_F32 / P2P_DTYPE_BF16 / P2P_DTYPE_F16             */
  float guidance;
  const float* x;         /* [R, n] the noisy latent at each row's timestep             */
  const float* target;    /* [R, n] the next cleaner level                              */
  const float* coef;      /* [R, 5] f32, device                                         */
  float* noise;           /* [R, n] out                                                 */
  int32_t R, n;
} p2p_ddpm_noise_args;

int p2p_ddpm_noise(const p2p_ddpm_noise_args* a, p2p_stream_t stream);

/* AttentionStore.get_average_attention (main.py:144-149): dst = src / divisor, computed as
 * src * (1.0f / divisor) -- what torch does for `cuda_tensor / python_scalar` on the
 * reference's cuda:0 device. */
int p2p_store_scale(const float* src, float* dst, float divisor, int64_t n, p2p_stream_t stream);

/* U-Net glue between the convolutions and GEMMs (p2p_amd/unet.py; additive to ABI 16): 16-bit
 * tensors only (dtype = P2P_DTYPE_BF16 or P2P_DTYPE_F16, anything else is P2P_E_DTYPE), f32
 * arithmetic, one rounding at the store, fixed-order reductions (bit-identical from launch to
 * launch).  Tensors are dense; x / y / a / b / out pointers are 16-byte aligned and hw % 8 == 0
 * (token-major tensors also need channels % 8 == 0), else P2P_E_ALIGN. */
enum { P2P_ACT_NONE = 0, P2P_ACT_SILU = 1 };
enum { P2P_LAYOUT_NCHW = 0,    /* [n, channels, hw]                                         */
       P2P_LAYOUT_TOKENS = 1   /* [n, hw, channels] (the transformer blocks' token layout)  */ };

/* y = act(GroupNorm(x + chan_add + chan_bias) * gamma + beta): nn.GroupNorm (+ F.silu) with the
 * per-channel adds in front of it (ResnetBlock2D: conv1's bias and the time-embedding projection)
 * taken on load.  Statistics per (n, group): mean, then the centred variance (biased, as torch),
 * both f32.  x is NCHW; y is NCHW or token-major. */
typedef struct {
  const void* x;            /* [n, channels, hw]                                           */
  const void* chan_add;     /* nullable: [n, channels] (stride = channels) or [channels] (0) */
  int64_t chan_add_stride;  /* 0 or channels                                                */
  const void* chan_bias;    /* nullable [channels], added like chan_add                     */
  const void* gamma;        /* [channels]                                                   */
  const void* beta;         /* [channels]                                                   */
  void* y;
  float* stats;             /* workspace, p2p_group_norm_stats_floats() f32: {mean, rstd} per
                             * slab -- n * groups * 2, all of it for slabs (channels / groups *
                             * hw) below 262,144 elements -- then, from that size, the
                             * per-chunk partials of the split statistics                    */
  int32_t n, channels, hw, groups;
  float eps;
  int32_t act;              /* P2P_ACT_*                                                    */
  int32_t y_layout;         /* P2P_LAYOUT_*                                                 */
  int32_t dtype;            /* P2P_DTYPE_BF16 / P2P_DTYPE_F16: every tensor but stats       */
} p2p_group_norm_args;

int p2p_group_norm(const p2p_group_norm_args* a, p2p_stream_t stream);
/* f32 elements p2p_group_norm needs behind `stats` for these sizes (a function of the sizes only),
 * or P2P_E_ARG. */
int64_t p2p_group_norm_stats_floats(int32_t n, int32_t channels, int32_t hw, int32_t groups);

/* out[n, c, hw] = a[n, c, hw] + b + bias[c] + bias2[c]: the residual add of ResnetBlock2D with the
 * biases of conv2 and of the shortcut conv (b NCHW), and of Transformer2DModel (b = the proj_out
 * tokens, token-major).  a and out are NCHW (out may be a); the biases are nullable. */
typedef struct {
  const void* a;
  const void* b;
  const void* bias;   /* nullable [channels] */
  const void* bias2;  /* nullable [channels] */
  void* out;
  int32_t n, channels, hw;
  int32_t b_layout;   /* P2P_LAYOUT_* */
  int32_t dtype;
} p2p_bias_residual_args;

int p2p_bias_residual(const p2p_bias_residual_args* a, p2p_stream_t stream);

/* p2p_conv3x3: the resnets' 3x3 convolution (stride 1, padding 1, no bias; additive to ABI 16) as
 * an implicit GEMM on the 16-bit MFMAs, under the glue's contract: f32 accumulation, one rounding
 * at the store, no atomics, the same bits on every launch.  x is token-major [n, height * width,
 * c_in] -- what p2p_group_norm writes with y_layout = P2P_LAYOUT_TOKENS -- `weight` the packed image
 * p2p_conv3x3_pack makes of nn.Conv2d's [c_out, c_in, 3, 3] (once per model: [9, c_out, c_in]),
 * y is NCHW [n, c_out, height * width].  Small maps split K over several workgroups per tile; their
 * f32 partials go through `workspace` and are summed in a fixed order by a second launch.
 * Rejected before any launch: a null x / weight / y, a size < 1, n * height * width (or an element
 * count of x, y or the weights) beyond int32, a null workspace where the sizes need one (P2P_E_ARG);
 * f32 (P2P_E_DTYPE); c_in % 32, c_out % 32, height * width % 8, a pointer off 16 bytes, and a size
 * p2p_conv3x3_split answers 0 for (P2P_E_ALIGN: the caller runs its own convolution). */
typedef struct {
  const void* x;       /* [n, height * width, c_in]                                            */
  const void* weight;  /* [9, c_out, c_in], from p2p_conv3x3_pack                              */
  void* y;             /* [n, c_out, height * width]                                           */
  float* workspace;    /* p2p_conv3x3_workspace_floats() f32; may be NULL where that is 0      */
  int32_t n, height, width, c_in, c_out;
  int32_t dtype;       /* P2P_DTYPE_BF16 / P2P_DTYPE_F16: x, weight and y                      */
} p2p_conv3x3_args;

int p2p_conv3x3(const p2p_conv3x3_args* a, p2p_stream_t stream);
/* Workgroups along K per output tile for these sizes (a function of the sizes only): 1 = one launch,
 * > 1 = the split form with its reduce launch, 0 = not served (a map above 64 x 64 pixels: not
 * measured), or the P2P_E_* code p2p_conv3x3 answers for the sizes. */
int p2p_conv3x3_split(int32_t n, int32_t height, int32_t width, int32_t c_in, int32_t c_out);
/* f32 elements p2p_conv3x3 needs behind `workspace` (0 without a split), or the P2P_E_* code. */
int64_t p2p_conv3x3_workspace_floats(int32_t n, int32_t height, int32_t width, int32_t c_in, int32_t c_out);

/* p2p_conv3x3_ex: the same kernel with a sampling form and an optional bias (additive to ABI 16).
 *   P2P_CONV_SAME   stride 1, padding 1: p2p_conv3x3 (which forwards here with a null bias);
 *   P2P_CONV_UP2    F.interpolate(scale_factor=2, mode="nearest") followed by the padded stride-1
 *                   convolution, the upsampled map never written: x is the low-resolution map, y
 *                   is 2 in_height x 2 in_width;
 *   P2P_CONV_DOWN2  stride 2, padding 1, even in_height and in_width: y is in_height / 2 x in_width / 2.
 * x is token-major [n, in_height * in_width, c_in], y NCHW on the output map, `weight` the image of
 * p2p_conv3x3_pack for every form.  bias: [c_out] in the tensors' dtype or NULL; it is added to the
 * f32 accumulator (in the split form to the sum of the partials) before the one rounding, and with
 * NULL the bits are those of the call without it.  The checks and codes are p2p_conv3x3's, on the
 * output map and on x's element count: also an unknown form (P2P_E_ARG), a bias off 2 bytes and odd
 * input sizes for P2P_CONV_DOWN2 (P2P_E_ALIGN). */
enum { P2P_CONV_SAME = 0, P2P_CONV_UP2 = 1, P2P_CONV_DOWN2 = 2 };

typedef struct {
  const void* x;       /* [n, in_height * in_width, c_in]                                      */
  const void* weight;  /* [9, c_out, c_in], from p2p_conv3x3_pack                              */
  const void* bias;    /* [c_out] or NULL                                                      */
  void* y;             /* [n, c_out, out_height * out_width]                                   */
  float* workspace;    /* p2p_conv3x3_ex_workspace_floats() f32; may be NULL where that is 0   */
  int32_t n, in_height, in_width, c_in, c_out;
  int32_t dtype;       /* P2P_DTYPE_BF16 / P2P_DTYPE_F16: x, weight, bias and y                */
  int32_t form;        /* P2P_CONV_*                                                           */
} p2p_conv3x3_ex_args;

int p2p_conv3x3_ex(const p2p_conv3x3_ex_args* a, p2p_stream_t stream);
/* p2p_conv3x3_split / _workspace_floats for a form, from the input map: the split comes from the
 * output map exactly as p2p_conv3x3_split's does; 0 = not served, or the P2P_E_* code. */
int p2p_conv3x3_ex_split(int32_t form, int32_t n, int32_t in_height, int32_t in_width, int32_t c_in, int32_t c_out);
int64_t p2p_conv3x3_ex_workspace_floats(int32_t form, int32_t n, int32_t in_height, int32_t in_width, int32_t c_in,
                                        int32_t c_out);

/* p2p_conv3x3_set_loop: which tile loop p2p_conv3x3 / p2p_conv3x3_ex launch where the plan is 64
 * channels a step and 160 output channels a tile (additive to ABI 16; process-wide, for tests and A/B
 * measurements; never change it while a stream is being captured).  0: the selection's choice per
 * shape (the default); 1: the register-staged loop everywhere; 2 / 3: the global_load_lds ring on 128 /
 * 256 pixels per workgroup wherever that tile holds.  The output bits are the same under every value.
 * Any other value: P2P_E_ARG, nothing changes. */
int p2p_conv3x3_set_loop(int32_t loop);

/* packed[tap, co, ci] = weight[co, ci, tap / 3, tap % 3]: the K-major image p2p_conv3x3 stages.
 * c_in % 32 and c_out % 32, packed on 16 bytes (else P2P_E_ALIGN). */
typedef struct {
  const void* weight;  /* [c_out, c_in, 3, 3], dense */
  void* packed;        /* [9, c_out, c_in]           */
  int32_t c_in, c_out;
  int32_t dtype;
} p2p_conv3x3_pack_args;

int p2p_conv3x3_pack(const p2p_conv3x3_pack_args* a, p2p_stream_t stream);

/* p2p_linear: y = epilogue(x[m, k] . weight[n, k]^T), the transformer blocks' feed-forward GEMMs on
 * the tile loop of p2p_conv3x3 (additive to ABI 16), under the glue's contract: 16-bit tensors, f32
 * accumulation, ONE rounding per output, no atomics, the same bits on every launch.  x is token-major
 * with a row stride in elements (% 8 == 0, >= k); weight is nn.Linear's own dense weight; y is dense.
 *   P2P_LINEAR_BIAS      y[m, j] = acc + bias[j];
 *   P2P_LINEAR_GEGLU     weight is [2 n, k], bias [2 n]: y[m, j] = (acc[m, j] + bias[j]) *
 *                        gelu(acc[m, n + j] + bias[n + j]), j < n, gelu the exact erf form in f32.
 *                        p_out (nullable): [m, 2 n] dense, the rounded pre-activation acc + bias;
 *                        asking for it does not change y's bits;
 *   P2P_LINEAR_RESIDUAL  y[m, j] = acc + bias[j] + res[m, j], res token-major with a row stride
 *                        (% 8 == 0, >= n).
 * bias is nullable in every form.  Small m splits k over several workgroups per tile (never the
 * GEGLU form); their f32 partials go through `workspace` and a second launch sums them in split
 * order and adds bias and residual.
 * Rejected before any launch: a null x / weight / y (res in the RESIDUAL form), an unknown form, a
 * size < 1, an element offset of x, weight, y, res or p_out beyond int32, a null workspace where the
 * sizes need one (P2P_E_ARG); f32 (P2P_E_DTYPE); k % 32, n % 8, a row stride % 8 or shorter than its
 * row, a pointer off 16 bytes (bias: 2), and sizes p2p_linear_split answers 0 for (P2P_E_ALIGN: the
 * caller runs its own GEMM). */
enum { P2P_LINEAR_BIAS = 0, P2P_LINEAR_GEGLU = 1, P2P_LINEAR_RESIDUAL = 2 };

typedef struct {
  const void* x;        /* [m, k], rows x_row_stride apart                                      */
  const void* weight;   /* [n, k] dense; P2P_LINEAR_GEGLU: [2 n, k]                             */
  const void* bias;     /* [n] ([2 n]) or NULL                                                  */
  const void* res;      /* P2P_LINEAR_RESIDUAL: [m, n], rows res_row_stride apart; else unused  */
  void* y;              /* [m, n] dense                                                         */
  void* p_out;          /* P2P_LINEAR_GEGLU: [m, 2 n] dense or NULL; else unused                */
  float* workspace;     /* p2p_linear_workspace_floats() f32; may be NULL where that is 0       */
  int64_t x_row_stride, res_row_stride;
  int32_t m, k, n;      /* n: output columns                                                    */
  int32_t form;         /* P2P_LINEAR_*                                                         */
  int32_t dtype;        /* P2P_DTYPE_BF16 / P2P_DTYPE_F16: every tensor but workspace           */
} p2p_linear_args;

int p2p_linear(const p2p_linear_args* a, p2p_stream_t stream);
/* Workgroups along k per output tile for these sizes (a function of the sizes only): 1 = one launch,
 * > 1 = the split form with its reduce launch, 0 = not served (a shape measured slower than the GEMM
 * it would replace), or the P2P_E_* code p2p_linear answers for the sizes. */
int p2p_linear_split(int32_t form, int32_t m, int32_t k, int32_t n);
/* f32 elements p2p_linear needs behind `workspace` (0 without a split), or the P2P_E_* code. */
int64_t p2p_linear_workspace_floats(int32_t form, int32_t m, int32_t k, int32_t n);

/* GEGLU: out[m, j] = in[m, j] * gelu(in[m, d + j]), j < d, gelu the exact erf form (F.gelu's
 * default).  Row strides in elements, multiples of 8 (as d), in_row_stride >= 2 d. */
typedef struct {
  const void* in;
  void* out;
  int64_t in_row_stride, out_row_stride;
  int32_t rows, d;
  int32_t dtype;
} p2p_geglu_args;

int p2p_geglu(const p2p_geglu_args* a, p2p_stream_t stream);

/* The glue's backward with respect to its tensors (p2p_amd/unet_grad.py; additive to ABI 16), under
 * the contract above.  New here: every reduction is taken inside one sample, in an order that
 * (channels, hw, groups) fix, so a sample's result bits depend neither on n nor on the other
 * samples (an all-zero dy of one sample gives that sample an exactly zero dx).
 *
 * p2p_group_norm_bwd: dx of p2p_group_norm -- not the gradients of gamma, beta or the per-channel
 * adds.  With xh = ((x + chan_add + chan_bias) - mean) * rstd and z = xh * gamma + beta:
 *   g = dy * act'(z) (SiLU'(z) = s (1 + z (1 - s)), s = sigmoid(z)),  gh = g * gamma,
 *   m1 = mean of gh, m2 = mean of gh * xh over the (n, group) slab,  dx = rstd * (gh - m1 - xh * m2).
 * z and g are recomputed from x and dy; {mean, rstd} are read from `stats`, the head of the
 * forward's workspace.  Slabs of 262,144 elements or more (the forward's split statistics) are
 * P2P_E_ARG. */
typedef struct {
  const void* x;            /* the forward's x, chan_add, chan_add_stride, chan_bias, gamma, beta */
  const void* chan_add;
  int64_t chan_add_stride;
  const void* chan_bias;
  const void* gamma;
  const void* beta;
  const void* dy;           /* [n, channels, hw], or [n, hw, channels] where the forward stored tokens */
  const float* stats;       /* {mean, rstd} per (n, group), as the forward left them: n * groups * 2 f32 */
  void* dx;                 /* [n, channels, hw]                                            */
  float* workspace;         /* p2p_group_norm_bwd_workspace_floats() f32                    */
  int32_t n, channels, hw, groups;
  int32_t act;              /* P2P_ACT_*, the forward's                                     */
  int32_t dy_layout;        /* P2P_LAYOUT_*, the forward's y_layout                         */
  int32_t dtype;            /* P2P_DTYPE_BF16 / P2P_DTYPE_F16: every tensor but stats and workspace */
} p2p_group_norm_bwd_args;

int p2p_group_norm_bwd(const p2p_group_norm_bwd_args* a, p2p_stream_t stream);
/* f32 elements p2p_group_norm_bwd needs behind `workspace` (a function of the sizes only, the same
 * for both layouts of dy), or P2P_E_ARG. */
int64_t p2p_group_norm_bwd_workspace_floats(int32_t n, int32_t channels, int32_t hw, int32_t groups);

/* GEGLU backward: din[m, j] = dout[m, j] * gelu(gate), din[m, d + j] = dout[m, j] * in[m, j] *
 * (Phi(gate) + gate * phi(gate)), gate = in[m, d + j], the exact erf form.  `in` as the forward's
 * (row stride a multiple of 8, >= 2 d); dout [rows, d] and din [rows, 2 d] are dense. */
typedef struct {
  const void* in;
  const void* dout;
  void* din;
  int64_t in_row_stride;
  int32_t rows, d;
  int32_t dtype;
} p2p_geglu_bwd_args;

int p2p_geglu_bwd(const p2p_geglu_bwd_args* a, p2p_stream_t stream);

/* dst[n, hw, channels] = src[n, channels, hw]: the gradient of p2p_bias_residual's token-major b
 * (that of a, and both of the NCHW form, are dout itself).  hw % 8 == 0 and channels % 8 == 0. */
typedef struct {
  const void* src;
  void* dst;
  int32_t n, channels, hw;
  int32_t dtype;
} p2p_nchw_to_tokens_args;

int p2p_nchw_to_tokens(const p2p_nchw_to_tokens_args* a, p2p_stream_t stream);

/* The U-Net's time path (p2p_amd/unet.py UNet2DConditionModel.forward; additive to ABI 16), under
 * the glue's contract: 16-bit weights and results, f32 accumulation in a fixed order, one rounding.
 *
 * p2p_time_embed: emb[n, :] = W2 . silu(W1 . [cos(t_n f_i), sin(t_n f_i)] + b1) + b2, the sinusoid
 * of timestep_embedding (f_i = exp(-ln(10000) i / half), half = in_channels / 2, cosines first) with
 * accurate cosf / sinf / expf, and TimestepEmbedding's two layers.  Nothing is rounded before emb:
 * linear_1's output stays f32, in `workspace`.  Two launches.  Rejected before any launch: a null
 * pointer, n outside [1, P2P_MAX_BATCH], in_channels or d outside [1, 2048], a timestep_stride
 * other than 0 or 1 (P2P_E_ARG); in_channels % 8 or d % 8, w1 / w2 / workspace / emb off 16 bytes,
 * timesteps off 8, a bias off 2 (P2P_E_ALIGN). */
typedef struct {
  const int64_t* timesteps;  /* n of them, or one for every row (timestep_stride = 0)          */
  int64_t timestep_stride;   /* 1 or 0                                                          */
  const void* w1;            /* [d, in_channels]                                                */
  const void* b1;            /* [d]                                                             */
  const void* w2;            /* [d, d]                                                          */
  const void* b2;            /* [d]                                                             */
  float* workspace;          /* n * d f32                                                       */
  void* emb;                 /* [n, d]                                                          */
  int32_t n, in_channels, d;
  int32_t dtype;
} p2p_time_embed_args;

int p2p_time_embed(const p2p_time_embed_args* a, p2p_stream_t stream);

/* p2p_time_proj: out_r[n, C_r] = W_r[C_r, d] . silu(emb[n, :]) + b_r for r < segments, in one launch:
 * the 22 time_emb_proj(F.silu(emb)) of the resnets.  `table` is device memory, 4 int64 per segment:
 * {W_r, b_r (addresses), s_r, C_r}: out_r starts n * s_r elements into `out` (s_r = the widths in
 * front of it for packed outputs), so one table serves every n; the weights are read where they
 * are.  W_r is 16-byte aligned and dense, as is every out_r ([n, C_r]): the caller answers for
 * the table's contents, which the host cannot see.  tiles = sum over r of ceil(C_r /
 * P2P_TIME_PROJ_TILE), the launch's workgroups (a larger count is harmless, a smaller one leaves
 * the last channels unwritten).  Rejected before the launch: a null pointer, n outside
 * [1, P2P_MAX_BATCH], d outside [1, 2048], segments < 1, tiles < 1 (P2P_E_ARG); d % 8, emb off 16
 * bytes, table off 8, out off 2 (P2P_E_ALIGN). */
#define P2P_TIME_PROJ_TILE 16
typedef struct {
  const void* emb;           /* [n, d]                                                          */
  const int64_t* table;      /* [segments, 4], device                                           */
  void* out;                 /* the arena the table's offsets count from                        */
  int32_t n, d, segments, tiles;
  int32_t dtype;
} p2p_time_proj_args;

int p2p_time_proj(const p2p_time_proj_args* a, p2p_stream_t stream);

/* The image ends of the pipeline (additive to ABI 16; p2p_amd/ptp_utils.py latent2image /
 * image2latent).  Three channels.  dtype: P2P_DTYPE_F32 / BF16 / F16, anything else is
 * P2P_E_DTYPE.  Both take height * width % 4 == 0 only (four pixels per thread, no scalar tail)
 * and answer P2P_E_ALIGN otherwise, as for a float pointer off 16 bytes or a byte pointer off 4:
 * the caller then converts some other way. */

/* out[n, y, x, c] = uint8(clamp(x[n, c, y, x] / 2 + 0.5, 0, 1) * 255), truncating: the reference's
 * latent2image arithmetic in f32, every operation rounded on its own, so the bytes equal
 * (((x.float() / 2 + 0.5).clamp(0, 1)) * 255).to(torch.uint8). */
typedef struct {
  const void* x;   /* [n, 3, height, width], dense */
  uint8_t* out;    /* [n, height, width, 3]        */
  int32_t n, height, width;
  int32_t dtype;   /* of x                         */
} p2p_image_u8_args;

int p2p_image_u8(const p2p_image_u8_args* a, p2p_stream_t stream);

/* out[n, c, y, x] = img[n, y, x, c] / 127.5 - 1, computed in f32 and rounded once to dtype. */
typedef struct {
  const uint8_t* img; /* [n, height, width, 3], dense */
  void* out;          /* [n, 3, height, width]        */
  int32_t n, height, width;
  int32_t dtype;      /* of out                       */
} p2p_image_to_model_args;

int p2p_image_to_model(const p2p_image_to_model_args* a, p2p_stream_t stream);

/* The CLIP text encoder (p2p_amd/text_encoder.py; ptp_utils.py:151,156 call it through
 * model.text_encoder), additive to ABI 16.  The three entry points below take 16-bit tensors only
 * (P2P_DTYPE_BF16 / P2P_DTYPE_F16, anything else is P2P_E_DTYPE), compute in f32 with one rounding
 * at the store, and reduce in a fixed order: bit-identical from launch to launch. */

/* Causal self-attention over the prompt tokens: O = softmax(causal(Q K^T * scale)) V, token i
 * attending to tokens <= i.  There is no padding mask.  The tokens x tokens matrix is never
 * written.  Rejected before anything is launched: n_query != n_key (P2P_E_ARG), more than
 * P2P_MAX_KEYS_CROSS tokens (P2P_E_KEYS), head_dim != 64 (P2P_E_HEAD_DIM), f32 tensors or
 * compute = P2P_COMPUTE_F32 (P2P_E_DTYPE), a pointer or stride off 16 bytes (P2P_E_ALIGN).
 * bf16 inputs run on bf16 MFMAs, fp16 inputs on f16 MFMAs. */
int p2p_causal_attn_fwd(const p2p_attn_tensors* t, p2p_stream_t stream);

/* nn.LayerNorm over rows of `channels` elements with the residual add in front of it:
 *   s = x + add + add_bias          (f32, left to right), rounded once to dtype
 *   sum_out = s                     (nullable; may alias x: the residual stream updated in place)
 *   y = (s - mean) * rstd * gamma + beta
 * with the mean and the centred, biased variance (both f32, as p2p_group_norm) taken from the
 * ROUNDED s -- the values the next reader of sum_out sees -- so the residual stream and its
 * normalised copy stay consistent.  Dense tensors, 16-byte aligned pointers; channels % 8 == 0
 * (else P2P_E_ALIGN) and channels <= 2048 (else P2P_E_ARG). */
typedef struct {
  const void* x;         /* [rows, channels]                                  */
  const void* add;       /* nullable [rows, channels]: a GEMM's output        */
  const void* add_bias;  /* nullable [channels]: that GEMM's bias             */
  const void* gamma;     /* [channels]                                        */
  const void* beta;      /* [channels]                                        */
  void* sum_out;         /* nullable [rows, channels]                         */
  void* y;               /* [rows, channels]                                  */
  int32_t rows, channels;
  float eps;
  int32_t dtype;         /* P2P_DTYPE_BF16 / P2P_DTYPE_F16: every tensor      */
} p2p_layer_norm_args;

int p2p_layer_norm(const p2p_layer_norm_args* a, p2p_stream_t stream);

/* Bias + quick-GELU behind a GEMM run without its bias: out[m, j] = h * sigmoid(1.702 h),
 * h = in[m, j] + bias[j], j < d.  Row strides in elements, multiples of 8 (as d), >= d; out may
 * be in. */
typedef struct {
  const void* in;
  const void* bias;  /* [d] */
  void* out;
  int64_t in_row_stride, out_row_stride;
  int32_t rows, d;
  int32_t dtype;
} p2p_bias_act_args;

int p2p_bias_quick_gelu(const p2p_bias_act_args* a, p2p_stream_t stream);

/* The LDMBert text encoder of LDM-256 (p2p_amd/ldm_bert.py; ptp_utils.py:98-126 call it through
 * model.bert), additive to ABI 16: the two entry points below beside p2p_layer_norm, under the
 * same rules (16-bit tensors, f32 arithmetic, one rounding at the store, a fixed reduction order). */

/* Bidirectional self-attention over the prompt tokens: O = softmax(Q K^T * scale) V, with the
 * operands, limits and rejections of p2p_causal_attn_fwd.  key_counts: NULL -- every entry attends
 * to all n_key tokens (the reference passes no attention mask) -- or a device array of n_batch
 * int32 counts (4-byte aligned, else P2P_E_ALIGN): entry n attends to keys < key_counts[n] only
 * (right padding), and all n_query rows are still computed and stored.  A key at or past the
 * count contributes exactly 0 and is never read from memory.  The counts live on the device, so a
 * count outside [1, n_key] cannot be seen, let alone rejected, by the host: the kernel clamps it
 * into [1, n_key], and no row is ever empty. */
int p2p_text_attn_fwd(const p2p_attn_tensors* t, const int32_t* key_counts, p2p_stream_t stream);

/* Bias + exact (erf) GELU behind a GEMM run without its bias: out[m, j] = 0.5 h (1 + erf(h / sqrt 2)),
 * h = in[m, j] + bias[j], j < d.  Arguments, vector widths, in-place rule and rejections as
 * p2p_bias_quick_gelu. */
int p2p_bias_gelu(const p2p_bias_act_args* a, p2p_stream_t stream);

/* The attention-map figures (main.py:293-350; p2p_amd/controllers.py aggregate_attention_device,
 * cross_attention_panels, show_self_attention_comp), additive to ABI 16. */

#define P2P_MAX_AGG_LAYERS 16

/* aggregate_attention (main.py:293-307) for one prompt, straight from AttentionStore's running
 * sums: out[p, k] = (sum over layers l, heads h of stores[l][select * heads[l] + h, p, k] / steps)
 * / (number of terms).  The arithmetic is fixed: every term is an IEEE f32 division by
 * (float)steps, the terms are added in f32 one after another, layer-major and head-minor (the order
 * main.py:305 concatenates them), and the sum is divided once by the term count.  Only the
 * selected prompt's slabs are read.  Four-element vector accesses: P * K % 4 != 0, or a store or
 * out off 16 bytes, is P2P_E_ALIGN.  n_layers outside [1, P2P_MAX_AGG_LAYERS], select outside
 * [0, n_prompts), steps < 1, a heads[l] < 1 or a null pointer is P2P_E_ARG. */
typedef struct {
  const float* stores[P2P_MAX_AGG_LAYERS]; /* [n_prompts * heads[l], P, K] f32, dense, prompt-major */
  int32_t heads[P2P_MAX_AGG_LAYERS];
  int32_t n_layers, n_prompts, select;
  int32_t P, K;
  int32_t steps;                           /* AttentionStore.cur_step */
  float* out;                              /* [P, K] */
} p2p_maps_aggregate_args;

int p2p_maps_aggregate(const p2p_maps_aggregate_args* a, p2p_stream_t stream);

/* n maps of res x res f32 values as n grey RGB uint8 panels of S x S pixels, normalised and
 * upscaled as the reference's NumPy + PIL lines do it (main.py:320-324, :342-348), byte for byte.
 * Element (panel i, pixel p) is in[i * panel_stride + p * pixel_stride] (strides in elements): the
 * columns of a cross map [res^2, K] are panel_stride 1, pixel_stride K; rows [n, res^2] are
 * panel_stride res^2, pixel_stride 1.  Pixel (y, x) of panel i goes to the three bytes at
 * out + i * out_panel_stride + y * out_row_stride + 3 x (strides in bytes), so a row of panels can
 * be written straight into a wider canvas.
 *   P2P_PANEL_MAX:    y = (255 * x) / max x, truncated to uint8        (show_cross_attention)
 *   P2P_PANEL_MINMAX: x' = x - min x, y = (255 * x') / max x', truncated (show_self_attention_comp)
 * every operation rounded to f32 on its own.  A panel whose divisor is 0, or that holds a NaN,
 * comes out all zero (the reference's result there is undefined).
 * The resize is PIL's 8-bit bicubic (a = -0.5): per output pixel P2P_RESIZE_TAPS taps, normalised
 * and rounded to 22-bit fixed point, the accumulator starting at 2^21, shifted and clamped; the
 * horizontal pass is rounded to uint8 before the vertical one.  coeffs / bounds: the tap table
 * int32 [S][P2P_RESIZE_TAPS] and {first input pixel, tap count} int32 [S][2] of a res -> S resize,
 * built on the host (p2p_amd/_hip.py resize_coeffs); entries that point past the panel are clamped.
 * 1 <= res <= P2P_PANEL_MAX_RES, res <= S <= P2P_PANEL_MAX_SIDE, S % 4 == 0 (at these sizes no
 * output pixel has more taps), out_row_stride >= 3 S, a known mode, n >= 1 and no null pointer:
 * else P2P_E_ARG.  in / coeffs / bounds / out and both byte strides on 4 bytes: else P2P_E_ALIGN. */
#define P2P_RESIZE_TAPS 5
#define P2P_PANEL_MAX_RES 64
#define P2P_PANEL_MAX_SIDE 512
enum { P2P_PANEL_MAX = 0, P2P_PANEL_MINMAX = 1 };

typedef struct {
  const float* in;
  int64_t panel_stride, pixel_stride;      /* elements */
  const int32_t* coeffs;                   /* [S][P2P_RESIZE_TAPS] */
  const int32_t* bounds;                   /* [S][2] */
  uint8_t* out;
  int64_t out_row_stride, out_panel_stride; /* bytes */
  int32_t res, n, S, mode;
} p2p_map_panels_args;

int p2p_map_panels(const p2p_map_panels_args* a, p2p_stream_t stream);

/* Batched null-text inversion (null_text.py:574-606 for B images in one U-Net call; p2p_amd/
 * null_text.py NullInversion.invert_batch), additive to ABI 16: new symbols only.  Both entry points
 * take B images of one size, keep one flag byte per image on the device (active: nonzero = still
 * optimising) and never involve the host, so they can sit in a captured graph. */

/* The guided DDIM prev_step, the per-image MSE against the inverted trajectory and its gradient
 * with respect to eps_u, in one launch (null_text.py:588-591 and the backward of those lines).
 * Per element, in f32 on the widened inputs, with c = coef[0..3] = sqrt(1 - a_t), sqrt(a_t),
 * sqrt(a_prev), sqrt(1 - a_prev) (DDIMScheduler.prev_coeffs, read from DEVICE memory so that a
 * graph captured once is refilled per DDIM step):
 *   eps  = eps_u + guidance * (eps_c - eps_u)
 *   prev = c2 * ((x - c0 * eps) / c1) + c3 * eps
 *   r    = prev - target
 *   loss[b] = mean(r^2) over image b's n elements
 *   grad_eps_u = (2 / n) * (1 - guidance) * (c3 - c2 * c0 / c1) * r
 * The scalar in front of r is formed in f64 and rounded to f32; the f32 product is rounded once to
 * the eps dtype.  The squares are summed in f64 in a fixed order, without atomics: image b's loss
 * and gradient bits depend on its own data only, not on B nor on its place in the batch, and are
 * the same from launch to launch.  Where active[b] == 0 the gradient is exact (+0) zeros; the loss
 * is written all the same.
 * Rejected before anything is launched: a null pointer, B <= 0 or n <= 0 (P2P_E_ARG); an eps_dtype
 * other than P2P_DTYPE_F32 / P2P_DTYPE_BF16 (P2P_E_DTYPE: fp16 too, as the attention backward this
 * gradient feeds refuses it); B > 65535 (P2P_E_BATCH); n % 4 != 0, or eps_u / eps_c / x / target /
 * coef / grad_eps_u off 16 bytes, or loss off 4 (P2P_E_ALIGN). */
typedef struct {
  const void* eps_u;      /* [B, n] in eps_dtype                                        */
  const void* eps_c;      /* [B, n] in eps_dtype                                        */
  int32_t eps_dtype;      /* P2P_DTYPE_F32 / P2P_DTYPE_BF16                             */
  float guidance;
  const float* x;         /* [B, n] the current latent                                  */
  const float* target;    /* [B, n] the inverted trajectory's previous latent           */
  const float* coef;      /* 4 f32, device                                              */
  const uint8_t* active;  /* [B], device                                                */
  float* loss;            /* [B] out                                                    */
  void* grad_eps_u;       /* [B, n] out, in eps_dtype                                   */
  int32_t B, n;
} P2PNullLossArgs;

int p2p_null_loss(const P2PNullLossArgs* a, p2p_stream_t stream);

/* One Adam step per image, gated, then the early stop of null_text.py:597.  For every image whose
 * flag is set AT LAUNCH, torch.optim.Adam's update (t = step[b] + 1):
 *   m <- beta1 m + (1 - beta1) g,   v <- beta2 v + (1 - beta2) g^2
 *   p <- p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   step[b] += 1,  steps_run[b] += 1
 * and then active[b] &= !(loss[b] < threshold[b]), a strict < in f32: the update of the step whose
 * loss met the threshold IS applied (the reference breaks after optimizer.step()).  Nothing of an
 * image whose flag is clear at launch is written: its param, both moments, step and steps_run keep
 * their bits.  The bias corrections and 1 - beta are formed in f64, as torch forms them in Python
 * floats, and then used as f32 scalars; beta1, beta2 and eps are therefore doubles (0.999f is not
 * 0.999: 1 - beta2^t would be off by 1e-5 of its value).
 * The flags and step counts are read by every workgroup of the update, so the update does not
 * write them: the entry point launches a second, one-thread-per-image kernel behind it on the same
 * stream, which advances the counts and clears the flags (no ping-pong buffers).
 * Rejected before anything is launched: a null pointer, B <= 0, m <= 0, a beta outside [0, 1) or a
 * negative eps (P2P_E_ARG); B > 65535 (P2P_E_BATCH); m % 4 != 0, param / grad / exp_avg /
 * exp_avg_sq off 16 bytes, or lr / step / loss / threshold / steps_run off 4 (P2P_E_ALIGN). */
typedef struct {
  float* param;            /* [B, m] in/out                                             */
  const float* grad;       /* [B, m]                                                    */
  float* exp_avg;          /* [B, m] in/out                                             */
  float* exp_avg_sq;       /* [B, m] in/out                                             */
  const float* lr;         /* device scalar                                             */
  int32_t* step;           /* [B] in/out: Adam's step count, reset per DDIM step        */
  uint8_t* active;         /* [B] in/out                                                */
  const float* loss;       /* [B], as p2p_null_loss wrote it                            */
  const float* threshold;  /* [B]: early_stop_epsilon_b + i * 2e-5, refilled per step   */
  int32_t* steps_run;      /* [B] in/out: updates applied since the caller zeroed it    */
  int32_t B, m;
  double beta1, beta2, eps; /* torch's defaults: 0.9, 0.999, 1e-8                       */
} P2PNullAdamArgs;

int p2p_null_adam(const P2PNullAdamArgs* a, p2p_stream_t stream);

/* Measurement only (ABI 15; bench.py's roofline clock, not part of the reference's interface):
 * n_workgroups one-wave workgroups each read the shader-cycle counter and the constant 100 MHz
 * counter, spin until `ticks` (1..1e6) of the 100 MHz counter have passed, and read both again:
 * out[2 w] = shader cycles, out[2 w + 1] = 100 MHz ticks of workgroup w, so the shader clock is
 * out[2 w] / out[2 w + 1] x 100 MHz.  Consecutive workgroups run on different XCDs.  out: device
 * memory, 2 x n_workgroups (1..1024) u64. */
int p2p_clock_probe(uint64_t* out, int32_t n_workgroups, int32_t ticks, p2p_stream_t stream);

/* Measurement only (ABI 15): kernel timing events (hipEvent_t, created by the caller) for the
 * next p2p_* calls of the calling thread -- their kernels are launched with hipExtLaunchKernel,
 * the first one recording `start`, each one `stop` (the last kernel's stands), from the kernels'
 * own dispatch timestamps.  Clear with (NULL, NULL).  Always returns 0. */
int p2p_set_launch_events(void* start, void* stop);

/* Build/runtime information.  p2p_source_hash: content hash of the HIP sources the library
 * was built from (p2p_amd/_srchash.py), so a host can refuse a stale prebuilt binary. */
int p2p_abi_version(void);
const char* p2p_source_hash(void);
const char* p2p_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif /* P2P_HIP_H */
