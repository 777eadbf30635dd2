// Which kernel runs for a shape: the one place that decides.  Plain C++17, no HIP: the two pure
// functions below map (dtype, compute, head dim, sizes, what the caller wants back) to a kernel
// form, p2p_dispatch.hip launches that form, and p2p_self_attn_kernel / p2p_cross_attn_kernel
// report it by name (tests/test_select.py pins the table on the CPU).  The kernel files export
// launchers only; every threshold, with the measurement behind it, lives here.
#pragma once

#include <stdint.h>

#include "../../include/p2p_hip.h"

namespace p2p {

enum { MODE_FUSED_ = 0, MODE_PV_ = 3 };

// P2P_SELF_VARIANT: the values an experiments build honours, each a clock-stamp diagnostic of one
// kernel (read once at load; select_self / select_cross refuse any other non-zero value with
// P2P_E_ARG).  A production build compiles the variable out and always passes 0.
enum Variant {
  VARIANT_CROSS_STAMPS = 90,    // cross_attn_kernel (tools/cross_stamps.py)
  VARIANT_GROUP_STAMPS = 123,   // cross_group_kernel, at d = 80 / 160 too (tools/group_stamps.py)
  VARIANT_SELF40_STAMPS = 163,  // self40_kernel at d = 40 (tools/s40_stamps.py)
  VARIANT_SELF80_STAMPS = 164,  // self40_kernel at d = 80
};
inline bool variant_known(int v) {
  return v == 0 || v == VARIANT_CROSS_STAMPS || v == VARIANT_GROUP_STAMPS || v == VARIANT_SELF40_STAMPS ||
         v == VARIANT_SELF80_STAMPS;
}

// ---------------------------------------------------------------------------- precision, head dim
// (io_dtype, compute) -> the (IO, MQ, MP) triple of the kernels: exact-f32 check mode; the bf16
// pipe on f32 inputs (split-bf16 QK^T so the logits keep f32 grade, bf16 PV); bf16 inputs (one
// bf16 MFMA per step, exact products); fp16 inputs (one f16 MFMA per step, exact products, f16 PV).
enum Precision { PREC_F32 = 0, PREC_SPLIT, PREC_BF16, PREC_F16 };

inline int select_precision(int io_dtype, int compute) {
  if (compute == P2P_COMPUTE_F32) return io_dtype == P2P_DTYPE_F32 ? (int)PREC_F32 : (int)P2P_E_DTYPE;
  if (io_dtype == P2P_DTYPE_F32) return PREC_SPLIT;
  if (io_dtype == P2P_DTYPE_F16) return PREC_F16;
  if (io_dtype == P2P_DTYPE_BF16) return PREC_BF16;
  return P2P_E_DTYPE;
}

// the head dims with compiled kernels
#define P2P_FOR_EACH_D(X) X(8) X(16) X(32) X(40) X(64) X(80) X(128) X(160)

inline bool head_dim_compiled(int d) {
  switch (d) {
#define P2P_CASE(DD) case DD:
    P2P_FOR_EACH_D(P2P_CASE)
#undef P2P_CASE
    return true;
    default: return false;
  }
}

// the one head dim outside that list: self_wide_kernel only (select_self)
constexpr int kWideHeadDim = 512;

// ---------------------------------------------------------------------------- self attention
// family of a self kernel form: which file's launcher takes it
enum SelfFamily { FAM_FUSED, FAM_PV, FAM_MULTI, FAM_SELF40, FAM_SPLIT, FAM_HALVES, FAM_RING, FAM_WIDE };
// row-statistics form of self_attn_fused_kernel
enum SelfForm { FORM_DEFAULT, FORM_EXACT, FORM_NOMAX };

// X(id, family, key tile | key blocks per wave, waves, form, name): "…" stands for the precision
// triple and D for the head dim, both inputs of the selection -- so a name (and a test that asserts
// it) tells the kernel family, tile shape and form, not which precision's or head dim's
// instantiation the launcher then takes; that step is with_precision / with_head_dim
// (p2p_device.h), one switch each, covered by the numeric tests.  Every row is a kernel some build
// can select; the STAMPS rows are compiled and selected by the experiments build only.
#define P2P_SELF_KERNELS(X)                                                                              \
  X(SELF_FUSED_32x2, FAM_FUSED, 32, 2, FORM_DEFAULT, "self_attn_fused_kernel<…,D,32,2>")                 \
  X(SELF_FUSED_32x2_EXACT, FAM_FUSED, 32, 2, FORM_EXACT, "self_attn_fused_kernel<…,D,32,2,EXACT>")       \
  X(SELF_FUSED_32x4, FAM_FUSED, 32, 4, FORM_DEFAULT, "self_attn_fused_kernel<…,D,32,4>")                 \
  X(SELF_FUSED_32x4_EXACT, FAM_FUSED, 32, 4, FORM_EXACT, "self_attn_fused_kernel<…,D,32,4,EXACT>")       \
  X(SELF_FUSED_64x2, FAM_FUSED, 64, 2, FORM_DEFAULT, "self_attn_fused_kernel<…,D,64,2>")                 \
  X(SELF_FUSED_64x2_EXACT, FAM_FUSED, 64, 2, FORM_EXACT, "self_attn_fused_kernel<…,D,64,2,EXACT>")       \
  X(SELF_FUSED_64x2_NOMAX, FAM_FUSED, 64, 2, FORM_NOMAX, "self_attn_fused_kernel<…,D,64,2,NOMAX>")       \
  X(SELF_FUSED_64x4, FAM_FUSED, 64, 4, FORM_DEFAULT, "self_attn_fused_kernel<…,D,64,4>")                 \
  X(SELF_FUSED_64x4_EXACT, FAM_FUSED, 64, 4, FORM_EXACT, "self_attn_fused_kernel<…,D,64,4,EXACT>")       \
  X(SELF_FUSED_64x4_NOMAX, FAM_FUSED, 64, 4, FORM_NOMAX, "self_attn_fused_kernel<…,D,64,4,NOMAX>")       \
  X(SELF_FUSED_64x8, FAM_FUSED, 64, 8, FORM_DEFAULT, "self_attn_fused_kernel<…,D,64,8>")                 \
  X(SELF_FUSED_64x8_EXACT, FAM_FUSED, 64, 8, FORM_EXACT, "self_attn_fused_kernel<…,D,64,8,EXACT>")       \
  X(SELF_FUSED_64x8_NOMAX, FAM_FUSED, 64, 8, FORM_NOMAX, "self_attn_fused_kernel<…,D,64,8,NOMAX>")       \
  X(SELF_PV_32x4, FAM_PV, 32, 4, FORM_DEFAULT, "self_pv_kernel<…,D,32,4>")                               \
  X(SELF_PV_64x4, FAM_PV, 64, 4, FORM_DEFAULT, "self_pv_kernel<…,D,64,4>")                               \
  X(SELF_MULTI_F16_256, FAM_MULTI, 256, 8, FORM_NOMAX, "self_attn_multi_kernel<…,40,256,8,2,F16,PIPE>")  \
  X(SELF_MULTI_128, FAM_MULTI, 128, 8, FORM_NOMAX, "self_attn_multi_kernel<…,40,128,8,2>")               \
  X(SELF40_D40, FAM_SELF40, 256, 8, FORM_NOMAX, "self40_kernel<40,8,2,256>")                             \
  X(SELF40_D40_H16, FAM_SELF40, 256, 8, FORM_NOMAX, "self40_kernel<40,8,2,256,H16>")                     \
  X(SELF40_D40_STAMPS, FAM_SELF40, 256, 8, FORM_NOMAX, "self40_kernel<40,8,2,256,STAMPS>")               \
  X(SELF40_D80, FAM_SELF40, 128, 8, FORM_NOMAX, "self40_kernel<80,8,1,128>")                             \
  X(SELF40_D80_H16, FAM_SELF40, 128, 8, FORM_NOMAX, "self40_kernel<80,8,1,128,H16>")                     \
  X(SELF40_D80_STAMPS, FAM_SELF40, 128, 8, FORM_NOMAX, "self40_kernel<80,8,1,128,STAMPS>")               \
  X(SELF_SPLIT_1x1, FAM_SPLIT, 1, 1, FORM_DEFAULT, "self_split_kernel<160,1,1>")                         \
  X(SELF_SPLIT_2x1, FAM_SPLIT, 1, 2, FORM_DEFAULT, "self_split_kernel<160,2,1>")                         \
  X(SELF_SPLIT_2x2, FAM_SPLIT, 2, 2, FORM_DEFAULT, "self_split_kernel<160,2,2>")                         \
  X(SELF_HALVES, FAM_HALVES, 32, 4, FORM_DEFAULT, "self_halves_kernel")                                  \
  X(SELF_RING, FAM_RING, 32, 4, FORM_DEFAULT, "self_ring_kernel<160,4>")                                 \
  X(SELF_WIDE, FAM_WIDE, 64, 4, FORM_DEFAULT, "self_wide_kernel<512,…>")

enum SelfKernel {
#define P2P_ENUM(id, fam, bk, w, form, nm) id,
  P2P_SELF_KERNELS(P2P_ENUM)
#undef P2P_ENUM
  SELF_KERNEL_COUNT
};

struct SelfKernelInfo {
  SelfFamily family;
  int bk;      // keys per tile (split family: 32-key blocks per wave)
  int waves;
  SelfForm form;
  const char* name;
};

inline const SelfKernelInfo& self_info(SelfKernel k) {
  static const SelfKernelInfo table[SELF_KERNEL_COUNT] = {
#define P2P_INFO(id, fam, bk, w, form, nm) {fam, bk, w, form, nm},
      P2P_SELF_KERNELS(P2P_INFO)
#undef P2P_INFO
  };
  return table[k];
}
inline const char* name(SelfKernel k) { return self_info(k).name; }

// Key tile of self_attn_fused_kernel / self_pv_kernel: 32 keys at d >= 128 and for the f32 P V
// (mp16 false: MP::kElemBytes == 4), else 64.  The launchers take their compile-time BK from here.
constexpr int fused_bk(int d, bool mp16) { return (d >= 128 || !mp16) ? 32 : 64; }

// self_attn_fused_kernel's form of a tile shape: EXACT and, where the table has it, NOMAX follow
// the shape's DEFAULT row
constexpr SelfKernel fused_form(SelfKernel shape, SelfForm form) { return (SelfKernel)(shape + (int)form); }
static_assert(SELF_FUSED_32x2_EXACT == SELF_FUSED_32x2 + FORM_EXACT && SELF_FUSED_32x4_EXACT == SELF_FUSED_32x4 + FORM_EXACT &&
                  SELF_FUSED_64x2_EXACT == SELF_FUSED_64x2 + FORM_EXACT && SELF_FUSED_64x4_EXACT == SELF_FUSED_64x4 + FORM_EXACT &&
                  SELF_FUSED_64x8_EXACT == SELF_FUSED_64x8 + FORM_EXACT,
              "EXACT follows DEFAULT");
static_assert(SELF_FUSED_64x2_NOMAX == SELF_FUSED_64x2 + FORM_NOMAX && SELF_FUSED_64x4_NOMAX == SELF_FUSED_64x4 + FORM_NOMAX &&
                  SELF_FUSED_64x8_NOMAX == SELF_FUSED_64x8 + FORM_NOMAX,
              "NOMAX follows EXACT (64-key shapes only: the 32-key shapes have no NOMAX row)");

// self_attn_fused_kernel's shape and form for a launch no specialised kernel takes
inline SelfKernel select_fused(int prec, int d, int P, bool lse, bool maps) {
  const bool mp16 = prec != PREC_F32;                 // 16-bit P V (MP::kElemBytes == 2)
  const int bk = fused_bk(d, mp16);
  // 8 waves x 32 query rows per workgroup, 64-key tiles (measured best at d = 40 and within 2 % of
  // best at d = 80: tools/attn_bench.py, profiles/); else 2 waves up to 64 rows, 4 above
  const int waves = (bk == 64 && (d == 40 || d == 80) && P > 64) ? 8 : P <= 64 ? 2 : 4;
  SelfForm form = FORM_DEFAULT;
  // kept maps: the lse feeds the stored maps, exact f32 row sums
  if (maps) form = FORM_EXACT;
  // O only (no lse) with a ones column (d % 32 != 0) and bf16 P: no per-tile max (p grows with
  // the f32 exponent range; f16 P keeps the defer-max loop, p <= 2^8)
  else if (!lse && bk == 64 && d % 32 != 0 && (prec == PREC_BF16 || prec == PREC_SPLIT)) form = FORM_NOMAX;
  const SelfKernel base = bk == 32 ? (waves == 2 ? SELF_FUSED_32x2 : SELF_FUSED_32x4)
                                   : (waves == 2 ? SELF_FUSED_64x2 : waves == 4 ? SELF_FUSED_64x4 : SELF_FUSED_64x8);
  return fused_form(base, form);   // (NOMAX only with bk == 64, above)
}

// The kernel a self launch runs, or a negative P2P_E_* code.  mode: MODE_FUSED_ (O, and the lse when
// `lse` or `maps`) or MODE_PV_ (the materialise protocol's P V).  variant: P2P_SELF_VARIANT of the
// experiments build (a Variant or 0; anything else: P2P_E_ARG), 0 in production.
inline int select_self(int io_dtype, int compute, int d, int P, int K, int mode, bool lse, bool maps,
                       int variant) {
#ifdef P2P_EXPERIMENTS
  if (!variant_known(variant)) return P2P_E_ARG;
#else
  (void)variant;
#endif
  const int prec = select_precision(io_dtype, compute);
  if (prec < 0) return prec;
  // d = 512 (the VAE's mid-block attention, one head as wide as the layer): p2p_selfwide.hip, the
  // only kernel of that width -- bf16 / fp16 inputs, O only.  512 is not in P2P_FOR_EACH_D, so
  // everything else at d = 512 (f32 inputs, check mode, P V mode, lse, kept maps, cross) is an
  // uncompiled head dim like any other.
  if (d == kWideHeadDim && mode == MODE_FUSED_ && !lse && !maps && (prec == PREC_BF16 || prec == PREC_F16))
    return SELF_WIDE;
  if (!head_dim_compiled(d)) return P2P_E_HEAD_DIM;
  if (mode == MODE_PV_) return fused_bk(d, prec != PREC_F32) == 32 ? SELF_PV_32x4 : SELF_PV_64x4;
  lse = lse || maps;
  const bool o_only = !lse;   // nothing but O wanted: no kept maps, no autograd
  // d = 40 / 80 with bf16 or fp16 inputs, O only (G1/G7, G2/G6): the software-pipelined kernel of
  // p2p_self40.hip, from the sizes where its 512- / 256-query workgroups and 256- / 128-key tiles
  // fill (d = 40: P >= 2048; d = 80: P >= 512; both K >= 256)
  if (o_only && (prec == PREC_BF16 || prec == PREC_F16) && K >= 256) {
    const bool h16 = prec == PREC_F16;   // fp16: the launch shapes of the bf16 defaults (K's
                                         // packed-u16 range check has nothing to check)
    if (d == 40 && P >= 2048) {
      if (h16) return SELF40_D40_H16;
#ifdef P2P_EXPERIMENTS
      if (variant == VARIANT_SELF40_STAMPS) return SELF40_D40_STAMPS;   // default with clock stamps
#endif
      // LEAN fragments, split staging (waves 0-3 K, 4-7 V), the younger half holding priority 1 on
      // three of every four steps (round 3: 0.1867 ms vs 0.1880-0.1885 for priority on alternate
      // step pairs and 0.2056 for round 2, profiles/r03/g1_ab/r03y_ab.log), and K's f16 range check
      // as a packed-u16 maximum (round 4: 0.1864-0.1865 vs 0.1881-0.1889 ms,
      // profiles/r04/ab/g1_r04h.log)
      return SELF40_D40;
    }
    if (d == 80 && P >= 512) {
      if (h16) return SELF40_D80_H16;
#ifdef P2P_EXPERIMENTS
      if (variant == VARIANT_SELF80_STAMPS) return SELF40_D80_STAMPS;   // default with clock stamps
#endif
      // d = 80: 8 waves x ONE 32-row query block (two waves per SIMD), 128-key tiles, split staging
      // and the younger half's priority duty of the d = 40 kernel.  In the pipeline (bench.py,
      // HIP events) 36.8-37.2 -> 30.9-31.2 us against round 4's 4 waves x 2 blocks (one wave per
      // SIMD), which is as fast only with hot inputs: the second wave hides the cold Q / K / V
      // loads the layer meets after its QKV GEMM (profiles/r05/d80_ab/; 4 x 1 x 64: 34.0, 8 x 1 x
      // 64: 35.9, without split staging or priority: 32.0-33.0)
      return SELF40_D80;
    }
  }
  // d = 40, O only, P >= 2048, what self40_kernel leaves: the multi-block kernel (bf16 / f32
  // inputs only; fp16 takes the per-tile kernel below).  bf16 inputs with K < 256: its F16 form
  // on 256-key tiles; f32 inputs (split-bf16 Q K^T, two K planes): 128-key tiles
  if (o_only && d == 40 && P >= 2048) {
    if (prec == PREC_BF16) return SELF_MULTI_F16_256;
    if (prec == PREC_SPLIT) return SELF_MULTI_128;
  }
  // d = 160, bf16 inputs, O only (the 16x16 / 8x8 layers): p2p_selfsplit.hip
  if (o_only && d == 160 && prec == PREC_BF16 && K >= 1) {
    // K <= 128 (the 8x8 layers): the waves of a 32-query workgroup split the keys (W = ceil(K / 64)
    // waves of 64 keys, or 2 x 32 for K <= 64).  Measured against the per-tile kernel
    // (tools/small_bench.py, profiles/r03/small): 8x8 (K = 64) 7.84 -> 6.21 us; 16x16 (K = 256)
    // 14.73 -> 16.51 us -- every 32-query workgroup then pulls the head's whole K and V through its
    // CU (4x the per-tile kernel's L2 -> CU traffic), so K > 128 keeps per-tile kernels:
    if (K <= 32) return SELF_SPLIT_1x1;
    if (K <= 64) return SELF_SPLIT_2x1;
    if (K <= 128) return SELF_SPLIT_2x2;
    // K <= 256 (16x16): two halves of the keys per 64-query workgroup; above, the 4-stage
    // global_load_lds ring
    return K <= 256 ? SELF_HALVES : SELF_RING;
  }
  return select_fused(prec, d, P, lse, maps);
}

// ---------------------------------------------------------------------------- mutual self attention
// mutual_attn_kernel (p2p_mutual.hip), O only: M(id, key tile, waves, class-masked, name).  "…" and
// D as in P2P_SELF_KERNELS.  (M, not X: the X rows of this file are the kernels that
// tests/test_gpu_layouts.py runs under every operand layout; these have their layout tests in
// tests/test_gpu_mutual.py.)
#define P2P_MUTUAL_KERNELS(M)                                                   \
  M(MUTUAL_32x4, 32, 4, false, "mutual_attn_kernel<…,D,32,4>")                  \
  M(MUTUAL_32x4_MASKED, 32, 4, true, "mutual_attn_kernel<…,D,32,4,MASKED>")     \
  M(MUTUAL_64x4, 64, 4, false, "mutual_attn_kernel<…,D,64,4>")                  \
  M(MUTUAL_64x4_MASKED, 64, 4, true, "mutual_attn_kernel<…,D,64,4,MASKED>")     \
  M(MUTUAL_64x8, 64, 8, false, "mutual_attn_kernel<…,D,64,8>")                  \
  M(MUTUAL_64x8_MASKED, 64, 8, true, "mutual_attn_kernel<…,D,64,8,MASKED>")

enum MutualKernel {
#define P2P_ENUM(id, bk, w, masked, nm) id,
  P2P_MUTUAL_KERNELS(P2P_ENUM)
#undef P2P_ENUM
  MUTUAL_KERNEL_COUNT
};

struct MutualKernelInfo {
  int bk;       // keys per tile
  int waves;
  bool masked;  // the class predicate is compiled in
  const char* name;
};

inline const MutualKernelInfo& mutual_info(MutualKernel k) {
  static const MutualKernelInfo table[MUTUAL_KERNEL_COUNT] = {
#define P2P_INFO(id, bk, w, masked, nm) {bk, w, masked, nm},
      P2P_MUTUAL_KERNELS(P2P_INFO)
#undef P2P_INFO
  };
  return table[k];
}
inline const char* name(MutualKernel k) { return mutual_info(k).name; }
static_assert(MUTUAL_32x4_MASKED == MUTUAL_32x4 + 1 && MUTUAL_64x4_MASKED == MUTUAL_64x4 + 1 &&
                  MUTUAL_64x8_MASKED == MUTUAL_64x8 + 1,
              "MASKED follows the unmasked shape");

// The kernel a mutual launch runs, or a negative P2P_E_* code.  masked: the call carries token
// classes.  One kernel family serves every precision and every compiled head dim; its loop is
// self_attn_fused_kernel's, so the tile and wave choice is select_fused's, whose measurements
// (tools/attn_bench.py, profiles/) were made on that loop: fused_bk's key tile (32 keys at d >= 128
// and for the f32 P V, else 64), 8 waves x 32 query rows at d = 40 / 80 on 64-key tiles (measured
// best at d = 40 and within 2 % of best at d = 80 there), 4 waves elsewhere.  P <= 64 keeps 4
// waves (select_fused takes 2): MasaCtrl's layers are the 32x32 and 64x64 ones, the small shapes
// occur in tests only.  Measured against the production self kernels on the same tensors (at d = 40 /
// 80 those are self40_kernel, not this loop; tools/mutual_bench.py, N = 8, H = 8, bf16, kernel time,
// profiles/r21/mutual/mutual_bench.txt): P = 4096, d = 40: 182.1 us self, 238.0 unmasked (1.31x),
// 298.3 / 292.0 masked with 30 % / 50 % foreground (1.64x / 1.60x); P = 1024, d = 80: 26.2 us self,
// 31.7 unmasked (1.21x), 38.3 / 38.2 masked (1.46x); fp16 within 3 % of these.  Other wave counts
// were not tried for this kernel.
inline int select_mutual(int io_dtype, int compute, int d, int P, bool masked) {
  const int prec = select_precision(io_dtype, compute);
  if (prec < 0) return prec;
  if (!head_dim_compiled(d)) return P2P_E_HEAD_DIM;
  const int bk = fused_bk(d, prec != PREC_F32);
  const int waves = (bk == 64 && (d == 40 || d == 80) && P > 64) ? 8 : 4;
  const MutualKernel base = bk == 32 ? MUTUAL_32x4 : waves == 4 ? MUTUAL_64x4 : MUTUAL_64x8;
  return base + (masked ? 1 : 0);
}

// ---------------------------------------------------------------------------- cross attention
// X(id, name): the group kernel's EDIT / STORE forms, and the per-entry kernel with its waves and
// whether the dense mapper tile is staged
#define P2P_CROSS_KERNELS(X)                                            \
  X(CROSS_GROUP, "cross_group_kernel<D,4>")                             \
  X(CROSS_GROUP_STORE, "cross_group_kernel<D,4,STORE>")                 \
  X(CROSS_GROUP_EDIT, "cross_group_kernel<D,4,EDIT>")                   \
  X(CROSS_GROUP_EDIT_STORE, "cross_group_kernel<D,4,EDIT,STORE>")       \
  X(CROSS_ENTRY_W2, "cross_attn_kernel<…,D,2>")                         \
  X(CROSS_ENTRY_W4, "cross_attn_kernel<…,D,4>")                         \
  X(CROSS_ENTRY_W4_DENSE, "cross_attn_kernel<…,D,4,DENSE>")

enum CrossKernel {
#define P2P_ENUM(id, nm) id,
  P2P_CROSS_KERNELS(P2P_ENUM)
#undef P2P_ENUM
  CROSS_KERNEL_COUNT
};

inline const char* name(CrossKernel k) {
  static const char* const table[CROSS_KERNEL_COUNT] = {
#define P2P_NAME(id, nm) nm,
      P2P_CROSS_KERNELS(P2P_NAME)
#undef P2P_NAME
  };
  return table[k];
}
inline bool is_group(CrossKernel k) { return k <= CROSS_GROUP_EDIT_STORE; }
static_assert(CROSS_GROUP_STORE == CROSS_GROUP + 1 && CROSS_GROUP_EDIT == CROSS_GROUP + 2 &&
                  CROSS_GROUP_EDIT_STORE == CROSS_GROUP + 3,
              "select_cross adds 2 for EDIT and 1 for STORE");

// Waves of cross_attn_kernel: 4, 2 for the f32 P V (mp16 false) at d >= 128.  The launcher takes
// its compile-time W from here.
constexpr int cross_waves(int d, bool mp16) { return (!mp16 && d >= 128) ? 2 : 4; }

// The kernel a cross launch runs, or a negative P2P_E_* code.  edit_terms / edit_dense: some group
// edits through the term planes / carries the dense f16 mapper tile; any_store: some entry keeps
// its maps.
inline int select_cross(int io_dtype, int compute, int d, int n_groups, int H, int P, int K, bool edit_terms,
                        bool edit_dense, bool any_store, int variant) {
#ifdef P2P_EXPERIMENTS
  if (!variant_known(variant)) return P2P_E_ARG;
#else
  (void)variant;
#endif
  const int prec = select_precision(io_dtype, compute);
  if (prec < 0) return prec;
  if (K > P2P_MAX_KEYS_CROSS) return P2P_E_KEYS;
  if (!head_dim_compiled(d)) return P2P_E_HEAD_DIM;
  // The group-coupled kernel (p2p_cross.hip): bf16 inputs and compute, no term-plane (non-dense)
  // programs (fp16 takes the per-entry kernel).
  // The workgroup walks the group's entries one after another, so it only pays where the grid
  // still fills the chip: >= 2 workgroups per CU (G1/G7: 2 groups x 8 heads x 32 query tiles).
  // Smaller grids (the 32x32 / 16x16 / 8x8 layers) keep the per-entry kernel's parallelism, and so
  // do d = 80 / 160 at any size: with eight groups per U-Net call (configs[3], 1024 workgroups at
  // G2/G6) the group kernel -- four entries with their map stores walked in sequence -- measured
  // 228.5 us per launch against the per-entry kernel's 131.4 (profiles/r04/group_vs_entry_r04aj/);
  // at d = 40 it stays ahead (146.9 vs 215.0 us).  (The d = 80 / 160 instantiations remain in the
  // experiments build, VARIANT_GROUP_STAMPS.)
  if (prec == PREC_BF16 && !edit_terms) {
    const int wgs = n_groups * H * ((P + 127) / 128);
    bool group = d == 40 && wgs >= 512;
#ifdef P2P_EXPERIMENTS
    if (variant == VARIANT_GROUP_STAMPS) group = d == 40 || d == 80 || d == 160;   // (tools/group_stamps.py)
#endif
    if (group) return CROSS_GROUP + (edit_dense ? 2 : 0) + (any_store ? 1 : 0);
  }
  if (prec == PREC_F32) return cross_waves(d, false) == 2 ? CROSS_ENTRY_W2 : CROSS_ENTRY_W4;
  // the dense path (16-bit P V only) forms the edit as one MFMA product with the mapper tile;
  // a launch that mixes dense and term-plane programs gathers all of them
  return (edit_dense && !edit_terms) ? CROSS_ENTRY_W4_DENSE : CROSS_ENTRY_W4;
}

// ---------------------------------------------------------------------------- 3x3 convolution
// conv3x3_kernel (p2p_conv.hip): 128 pixels x bn output channels per workgroup, bk channels of one
// tap per K step, `split` workgroups along K per tile (their f32 partials summed in split order by
// conv3x3_reduce_kernel).  split == 0: the shape stays with the caller's convolution.
constexpr int kConvBM = 128;
constexpr int kConvMaxHW = 4096;     // the U-Net's largest map; the VAE's larger ones were not measured
constexpr int kConvMaxSplit = 8;
constexpr int kConvFillTiles = 512;  // two workgroups per CU of the 256
constexpr int kConvMinSteps = 8;     // K steps a split keeps at least

struct ConvPlan {
  int bk, bn, split;
};

// sizes p2p_conv3x3 rejects before anything else: 0, or the P2P_E_* code
inline int conv3x3_check_sizes(int n, int h, int w, int c_in, int c_out) {
  if (n < 1 || h < 1 || w < 1 || c_in < 1 || c_out < 1) return P2P_E_ARG;
  const int64_t m = (int64_t)n * h * w;
  // pixels, and the element offsets into x, y and the packed weights, are 32-bit in the kernel
  if (m > INT32_MAX || m * c_in > INT32_MAX || m * c_out > INT32_MAX || (int64_t)9 * c_in * c_out > INT32_MAX)
    return P2P_E_ARG;
  if (c_in % 32 || c_out % 32 || ((int64_t)h * w) % 8) return P2P_E_ALIGN;
  return 0;
}

// Tile shape and K split from the sizes alone (never the device).  bk: 64 where it divides c_in, else
// 32.  bn: 160 where it divides c_out (320, 640, 1280: no tail tile) and bk is 64, else 128.  split:
// as many as bring the grid to kConvFillTiles workgroups (two per CU: the second hides the first
// one's barriers), at most kConvMaxSplit -- each split writes and the reduce reads an f32 copy of y
// -- and never leaving a split fewer than kConvMinSteps K steps.  At N = 8 that is 1 at 64x64 (512
// tiles), 2 at 32x32, 4 at 16x16 and 8 at 8x8.  Measured (tools/conv_bench.py, profiles/r17/conv3x3/
// conv_bench.txt): every resnet shape of the U-Net beats the chain it replaces, 1.74x to 2.38x; with
// split 1 at 32x32 (256 tiles, one workgroup per CU) 640 -> 640 took 100.8 us against 83.4 with 2,
// 1920 -> 640 291.9 against 217.6 (conv_bench_split1_at_32.txt).
inline ConvPlan select_conv3x3(int n, int h, int w, int c_in, int c_out) {
  ConvPlan p = {0, 0, 0};
  if (conv3x3_check_sizes(n, h, w, c_in, c_out) != 0 || h * w > kConvMaxHW) return p;
  p.bk = c_in % 64 == 0 ? 64 : 32;
  p.bn = (p.bk == 64 && c_out % 160 == 0) ? 160 : 128;
  const int64_t m = (int64_t)n * h * w;
  const int64_t tiles = ((m + kConvBM - 1) / kConvBM) * ((c_out + p.bn - 1) / p.bn);
  const int steps = 9 * c_in / p.bk;
  int64_t s = 1;
  if (tiles < kConvFillTiles) {
    s = (kConvFillTiles + tiles - 1) / tiles;
    if (s > kConvMaxSplit) s = kConvMaxSplit;
    if (s > steps / kConvMinSteps) s = steps / kConvMinSteps;
    if (s < 1) s = 1;
  }
  p.split = (int)s;
  return p;
}
// f32 elements of p2p_conv3x3_args.workspace
inline int64_t conv3x3_workspace_floats(int n, int h, int w, int c_in, int c_out) {
  const ConvPlan p = select_conv3x3(n, h, w, c_in, c_out);
  return p.split > 1 ? (int64_t)p.split * n * h * w * c_out : 0;
}

// The sampling forms (P2P_CONV_*): Up2 reads a map half the output's size, Down2 one twice its size.
// The output map of a form's input map; false for an unknown form, a size < 1, or an input Down2
// does not take (odd sizes: its upper edge would be crossed).
inline bool conv3x3_out_map(int form, int ih, int iw, int* oh, int* ow) {
  if (ih < 1 || iw < 1 || ih > (1 << 20) || iw > (1 << 20)) return false;
  switch (form) {
    case P2P_CONV_SAME: *oh = ih, *ow = iw; return true;
    case P2P_CONV_UP2: *oh = 2 * ih, *ow = 2 * iw; return true;
    case P2P_CONV_DOWN2: *oh = ih / 2, *ow = iw / 2; return ih % 2 == 0 && iw % 2 == 0;
    default: return false;
  }
}
// sizes p2p_conv3x3_ex rejects: conv3x3_check_sizes on the output map, and x's element offsets
// (Down2's input is four times the output) within 32 bits
inline int conv3x3_check_sizes(int form, int n, int ih, int iw, int c_in, int c_out) {
  if (form != P2P_CONV_SAME && form != P2P_CONV_UP2 && form != P2P_CONV_DOWN2) return P2P_E_ARG;
  if (n < 1 || ih < 1 || iw < 1 || c_in < 1 || c_out < 1) return P2P_E_ARG;
  if ((int64_t)n * ih * iw > INT32_MAX || (int64_t)n * ih * iw * c_in > INT32_MAX) return P2P_E_ARG;
  int oh, ow;
  if (!conv3x3_out_map(form, ih, iw, &oh, &ow)) return P2P_E_ALIGN;
  return conv3x3_check_sizes(n, oh, ow, c_in, c_out);
}
// The plan of a form at its OUTPUT map h x w: tile and split come from the output M exactly as for
// Same, and Up2 / Down2 are served on the same maps (h w <= kConvMaxHW, h w % 8 == 0).  Which of the
// U-Net's six resampling convolutions take the kernel was measured per shape (tools/conv_bench.py,
// DESIGN.md §4.16).
inline ConvPlan select_conv3x3(int form, int n, int h, int w, int c_in, int c_out) {
  if (form != P2P_CONV_SAME && form != P2P_CONV_UP2 && form != P2P_CONV_DOWN2) return ConvPlan{0, 0, 0};
  return select_conv3x3(n, h, w, c_in, c_out);
}

// The tile loop of a bk = 64, bn = 160 plan (p2p_conv3x3_set_loop's values): conv3x3_kernel's
// register-staged loop, or conv3x3_pipe_kernel's global_load_lds ring on 128 or 256 pixels per
// workgroup.  The plan -- bk, bn, split, the workspace -- is the same under each, and so are the bits.
enum ConvLoop { CONV_LOOP_AUTO = 0, CONV_LOOP_TILE = 1, CONV_LOOP_PIPE128 = 2, CONV_LOOP_PIPE256 = 3 };
// stage images in the ring: 36,864 B each at 128 pixels, 53,248 B at 256 (160 KiB of LDS).  Measured
// (tools/conv_bench.py --loops, profiles/r24/conv_pipe/candidates_*.txt, N = 8, bf16): at 256 pixels 3
// stages against 2 are equal at 64x64 and 32x32 and 5 to 9 % faster at 16x16 and 8x8; at 128 pixels on
// the 8x8 maps 3 stages 30.9 / 48.9 us, 4 stages 31.4 / 49.4, 2 stages (two workgroups per CU) 36.6 / 59.2.
constexpr int kConvPipeDepth128 = 3;
constexpr int kConvPipeDepth256 = 3;
constexpr int kConvPipeFill = 256;   // workgroups that give every CU one

constexpr int conv3x3_loop_bm(int loop) { return loop == CONV_LOOP_PIPE256 ? 256 : kConvBM; }

// The loop the selection takes for a form at its OUTPUT map h x w, from the sizes alone; CONV_LOOP_TILE
// for every plan that is not bk = 64, bn = 160 (the ring is built for that tile only).  The ring on 256
// pixels wherever its tiles and splits give every CU a workgroup, else on 128.  Measured against the
// register-staged kernel on the same operands (tools/conv_bench.py --loops, profiles/r24/conv_pipe/
// candidates_1.txt, candidates_2.txt and conv_bench.txt, all 20 convolution shapes of the U-Net at
// N = 8): the 17 shapes with 256 workgroups or more take 256 pixels (0.76x to 0.93x of that kernel's
// time; 128 pixels lost to it on each of them, 1.01x to 1.17x), the three 8x8 shapes (128 workgroups
// at 256 pixels, 256 at 128) take 128 pixels (0.76x to 0.78x; 256 pixels equal to it or 3 % slower).
// No shape of the U-Net stays on the register-staged loop.
inline int select_conv3x3_loop(int form, int n, int h, int w, int c_in, int c_out) {
  const ConvPlan p = select_conv3x3(form, n, h, w, c_in, c_out);
  if (p.split < 1 || p.bk != 64 || p.bn != 160) return CONV_LOOP_TILE;
  const int64_t m = (int64_t)n * h * w;
  const int64_t wgs = ((m + 255) / 256) * (c_out / p.bn) * p.split;
  return wgs >= kConvPipeFill ? CONV_LOOP_PIPE256 : CONV_LOOP_PIPE128;
}

// the loop a launch runs: the forced one (p2p_conv3x3_set_loop) where the plan's tile has it, else
// the selection's
inline int conv3x3_loop(int forced, const ConvPlan& p, int form, int n, int h, int w, int c_in, int c_out) {
  if (p.bk != 64 || p.bn != 160) return CONV_LOOP_TILE;
  return forced == CONV_LOOP_AUTO ? select_conv3x3_loop(form, n, h, w, c_in, c_out) : forced;
}

// ---------------------------------------------------------------------------- linear layers
// linear_kernel (p2p_linear.hip): conv3x3_kernel's tile loop on y = x[m, k] . W[n, k]^T -- 128 rows x
// bn staged weight rows per workgroup, bk of k per step, `split` workgroups along k per tile (their
// f32 partials summed in split order by linear_reduce_kernel).  split == 0: the caller's GEMM.
struct LinearPlan {
  int bk, bn, split;
};

// sizes p2p_linear rejects before anything else: 0, or the P2P_E_* code.  n: output columns (the
// GEGLU form's weight has 2 n rows)
inline int linear_check_sizes(int form, int m, int k, int n) {
  if (form != P2P_LINEAR_BIAS && form != P2P_LINEAR_GEGLU && form != P2P_LINEAR_RESIDUAL) return P2P_E_ARG;
  if (m < 1 || k < 1 || n < 1) return P2P_E_ARG;
  const int64_t rows = form == P2P_LINEAR_GEGLU ? (int64_t)2 * n : n;
  // the element offsets into x, the weight, y and p_out are 32-bit in the kernel
  if ((int64_t)m * k > INT32_MAX || rows * k > INT32_MAX || (int64_t)m * rows > INT32_MAX) return P2P_E_ARG;
  if (k % 32 || n % 8) return P2P_E_ALIGN;
  return 0;
}

// output columns of one tile: the GEGLU form stages a column's h row and its gate row
inline int linear_tile_cols(int form, const LinearPlan& p) { return form == P2P_LINEAR_GEGLU ? p.bn / 2 : p.bn; }

// Shapes measured slower than the chain they replace stay with the caller's GEMM (tools/linear_bench.py
// at N = 8, bf16, profiles/r23/linear/linear_bench.txt): the three feed-forward
// output GEMMs whose K is split -- their f32 partials cost more than the add they save, 54.6 us
// against 42.8 at 32 x 32 (split 2), 60.1 against 48.8 at 16 x 16 (split 4), 52.5 against 28.4 at
// 8 x 8 (split 8) -- and the GEGLU GEMM at 8 x 8 (320 tiles: 34.1 against 27.7).  A weight that lost at
// m rows is declined for every m up to that: fewer rows are fewer tiles still.
struct LinearDeclined {
  int form, k, n, max_m;
};
constexpr LinearDeclined kLinearDeclined[] = {
    {P2P_LINEAR_RESIDUAL, 2560, 640, 8192},
    {P2P_LINEAR_RESIDUAL, 5120, 1280, 2048},
    {P2P_LINEAR_GEGLU, 1280, 5120, 512},
};
inline bool linear_declined(int form, int m, int k, int n) {
  for (const LinearDeclined& d : kLinearDeclined)
    if (form == d.form && k == d.k && n == d.n && m <= d.max_m) return true;
  return false;
}

// Tile shape and K split from the sizes alone (never the device), by conv3x3_kernel's rules.  bk: 64
// where it divides k, else 32.  bn: 160 where it divides n and bk is 64, else 128; the GEGLU form
// always 128 (its fragments pair up: 64 output columns a tile).  split: as many as bring the grid to
// kConvFillTiles workgroups, at most kConvMaxSplit, never leaving a split fewer than kConvMinSteps
// steps; the GEGLU form is never split.
inline LinearPlan select_linear(int form, int m, int k, int n) {
  LinearPlan p = {0, 0, 0};
  if (linear_check_sizes(form, m, k, n) != 0 || linear_declined(form, m, k, n)) return p;
  p.bk = k % 64 == 0 ? 64 : 32;
  p.bn = (form != P2P_LINEAR_GEGLU && p.bk == 64 && n % 160 == 0) ? 160 : 128;
  const int cols = linear_tile_cols(form, p);
  const int64_t tiles = (int64_t)((m + kConvBM - 1) / kConvBM) * ((n + cols - 1) / cols);
  const int steps = k / p.bk;
  int64_t s = 1;
  if (form != P2P_LINEAR_GEGLU && tiles < kConvFillTiles) {
    s = (kConvFillTiles + tiles - 1) / tiles;
    if (s > kConvMaxSplit) s = kConvMaxSplit;
    if (s > steps / kConvMinSteps) s = steps / kConvMinSteps;
    if (s < 1) s = 1;
  }
  p.split = (int)s;
  return p;
}
// f32 elements of p2p_linear_args.workspace: [split][n][m rounded up to the tile]
inline int64_t linear_workspace_floats(int form, int m, int k, int n) {
  const LinearPlan p = select_linear(form, m, k, n);
  return p.split > 1 ? (int64_t)p.split * n * ((m + kConvBM - 1) / kConvBM * kConvBM) : 0;
}

}  // namespace p2p
