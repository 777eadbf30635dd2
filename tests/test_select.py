"""Which kernel runs for a shape (csrc/p2p_select.h), pinned on the CPU through the library's query
entry points p2p_self_attn_kernel / p2p_cross_attn_kernel: they validate and select exactly as the
forward calls do and launch nothing, so no GPU is needed.  The expected names are DESIGN.md §4's,
written from the dispatch code of the commit that introduced the table -- a change of a threshold
or of a ladder's order fails here instead of passing every numeric test on another kernel."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

from p2p_amd import _hip

from test_gpu_kernels import CROSS_GROUP_CASES

F32, BF16, F16 = _hip.P2P_DTYPE_F32, _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16
C16, C32 = _hip.P2P_COMPUTE_BF16, _hip.P2P_COMPUTE_F32


def _tensors(io, compute, d, P, K, H=8, N=8):
    t = _hip.AttnTensors()
    t.q = t.k = t.v = t.o = 4096                       # never dereferenced: nothing is launched
    t.q_row_stride = t.k_row_stride = t.v_row_stride = t.o_row_stride = H * d
    t.q_batch_stride = t.k_batch_stride = t.v_batch_stride = t.o_batch_stride = H * d * max(P, K)
    t.n_batch, t.n_query, t.n_key, t.n_heads, t.head_dim = N, P, K, H, d
    t.io_dtype, t.compute, t.scale = io, compute, d ** -0.5
    return t


def fused(bk, waves, form=""):
    return "self_attn_fused_kernel<…,D,%d,%d%s>" % (bk, waves, "," + form if form else "")


SELF_ROWS = [  # (id, io, compute, d, P, K, maps kept, lse wanted, kernel)
    ("g1", BF16, C16, 40, 4096, 4096, 0, 0, "self40_kernel<40,8,2,256>"),
    ("d40_p2048", BF16, C16, 40, 2048, 256, 0, 0, "self40_kernel<40,8,2,256>"),              # both thresholds, at them
    ("d40_k200", BF16, C16, 40, 2048, 200, 0, 0, "self_attn_multi_kernel<…,40,256,8,2,F16,PIPE>"),
    ("d40_k255", BF16, C16, 40, 4096, 255, 0, 0, "self_attn_multi_kernel<…,40,256,8,2,F16,PIPE>"),
    ("d40_p2047", BF16, C16, 40, 2047, 2047, 0, 0, fused(64, 8, "NOMAX")),
    ("d40_p65", BF16, C16, 40, 65, 65, 0, 0, fused(64, 8, "NOMAX")),
    ("d40_p64", BF16, C16, 40, 64, 64, 0, 0, fused(64, 2, "NOMAX")),
    ("d40_maps", BF16, C16, 40, 4096, 4096, 1, 0, fused(64, 8, "EXACT")),
    ("d40_lse", BF16, C16, 40, 4096, 4096, 0, 1, fused(64, 8)),
    ("g2", BF16, C16, 80, 1024, 1024, 0, 0, "self40_kernel<80,8,1,128>"),
    ("d80_p512", BF16, C16, 80, 512, 256, 0, 0, "self40_kernel<80,8,1,128>"),
    ("d80_p511", BF16, C16, 80, 511, 511, 0, 0, fused(64, 8, "NOMAX")),
    ("d80_k255", BF16, C16, 80, 1024, 255, 0, 0, fused(64, 8, "NOMAX")),
    ("d80_maps", BF16, C16, 80, 1024, 1024, 1, 0, fused(64, 8, "EXACT")),
    ("d160_k20", BF16, C16, 160, 20, 20, 0, 0, "self_split_kernel<160,1,1>"),
    ("d160_k32", BF16, C16, 160, 32, 32, 0, 0, "self_split_kernel<160,1,1>"),
    ("d160_k33", BF16, C16, 160, 33, 33, 0, 0, "self_split_kernel<160,2,1>"),
    ("d160_k64", BF16, C16, 160, 64, 64, 0, 0, "self_split_kernel<160,2,1>"),
    ("d160_k65", BF16, C16, 160, 65, 65, 0, 0, "self_split_kernel<160,2,2>"),
    ("d160_k128", BF16, C16, 160, 128, 128, 0, 0, "self_split_kernel<160,2,2>"),
    ("d160_k129", BF16, C16, 160, 129, 129, 0, 0, "self_halves_kernel"),
    ("d160_k256", BF16, C16, 160, 256, 256, 0, 0, "self_halves_kernel"),
    ("d160_k257", BF16, C16, 160, 257, 257, 0, 0, "self_ring_kernel<160,4>"),
    ("d160_k300", BF16, C16, 160, 300, 300, 0, 0, "self_ring_kernel<160,4>"),
    ("d160_maps", BF16, C16, 160, 256, 256, 1, 0, fused(32, 4, "EXACT")),
    ("d160_lse", BF16, C16, 160, 64, 64, 0, 1, fused(32, 2)),
    ("d64", BF16, C16, 64, 1024, 1024, 0, 0, fused(64, 4)),                                   # no ones column: no NOMAX
    ("f16_d40", F16, C16, 40, 4096, 4096, 0, 0, "self40_kernel<40,8,2,256,H16>"),
    ("f16_d40_k200", F16, C16, 40, 2048, 200, 0, 0, fused(64, 8)),                            # no fp16 multi kernel
    ("f16_d80", F16, C16, 80, 1024, 1024, 0, 0, "self40_kernel<80,8,1,128,H16>"),
    ("f16_d80_p511", F16, C16, 80, 511, 511, 0, 0, fused(64, 8)),                             # defer-max, never NOMAX
    ("f16_d160", F16, C16, 160, 256, 256, 0, 0, fused(32, 4)),
    ("f16_d160_k64", F16, C16, 160, 64, 64, 0, 0, fused(32, 2)),
    ("f16_lse", F16, C16, 40, 4096, 4096, 0, 1, None),                                        # no fp16 autograd pair
    ("f32in_d40", F32, C16, 40, 4096, 4096, 0, 0, "self_attn_multi_kernel<…,40,128,8,2>"),
    ("f32in_d40_p2047", F32, C16, 40, 2047, 2047, 0, 0, fused(64, 8, "NOMAX")),
    ("f32in_d80", F32, C16, 80, 1024, 1024, 0, 0, fused(64, 8, "NOMAX")),
    ("f32in_d160", F32, C16, 160, 256, 256, 0, 0, fused(32, 4)),
    ("f32_d40", F32, C32, 40, 4096, 4096, 0, 0, fused(32, 4)),
    ("f32_d40_p64", F32, C32, 40, 64, 64, 0, 0, fused(32, 2)),
    ("f32_maps", F32, C32, 80, 1024, 1024, 1, 0, fused(32, 4, "EXACT")),
    ("f32_lse", F32, C32, 40, 4096, 4096, 0, 1, None),                                        # autograd: bf16 pipe only
    ("f32_compute_bf16_tensors", BF16, C32, 40, 4096, 4096, 0, 0, None),
    ("f32_compute_f16_tensors", F16, C32, 40, 4096, 4096, 0, 0, None),
    ("d44", BF16, C16, 44, 4096, 4096, 0, 0, None),
    ("d48", BF16, C16, 48, 4096, 4096, 0, 0, None),
]


@pytest.mark.parametrize("row", SELF_ROWS, ids=lambda r: r[0])
def test_self_selection(row):
    _, io, compute, d, P, K, maps, lse, want = row
    assert _hip.self_attn_kernel(_tensors(io, compute, d, P, K), keeps_maps=maps, wants_lse=lse) == want


PROG = 4096          # a device pointer the query never follows
DENSE, TERMS = 1, 0  # p2p_group.flags: P2P_PROGRAM_F_DENSE or a term-plane program


def _groups(n_batch, n_cond, B, flags=None):
    """[uncond groups | cond groups] of B entries each, as the GPU tests batch them; the cond groups
    carry a program with `flags` (None: no program)."""
    n = n_batch // B
    G = (_hip.Group * n)()
    for g in range(n):
        G[g].first, G[g].count = g * B, B
        if flags is not None and g >= n - n_cond:
            G[g].program, G[g].alpha, G[g].flags, G[g].n_edits = PROG, PROG, flags, B - 1
    return G


def _cross(io, compute, d, P, K, H, n_groups, flags, any_store, B=4):
    N = 2 * B * n_groups
    return _hip.cross_attn_kernel(_tensors(io, compute, d, P, K, H, N), _groups(N, n_groups, B, flags), any_store)


@pytest.mark.parametrize("case", CROSS_GROUP_CASES, ids=lambda c: "P{}_d{}_K{}_H{}_g{}_{}".format(*c))
def test_cross_selection_group_cases(case):
    """test_cross_group_kernel_bf16's launches: dense Replace edits, the cond maps kept."""
    P, d, K, H, n_groups, kernel = case
    want = "cross_group_kernel<D,4,EDIT,STORE>" if kernel == "group" else "cross_attn_kernel<…,D,4,DENSE>"
    assert _cross(BF16, C16, d, P, K, H, n_groups, DENSE, True) == want


@pytest.mark.parametrize("geom", [(4096, 40, 1, "group"), (4096, 40, 2, "group"), (4000, 40, 1, "group"),
                                  (1024, 80, 1, "entry"), (256, 160, 8, "entry")],
                         ids=lambda g: "P{}_d{}_g{}_{}".format(*g))
def test_cross_selection_shared_kv_geometries(geom):
    """test_cross_shared_kv_hint's launches: plain steps and dense edit steps, nothing stored."""
    P, d, n_groups, kernel = geom
    plain, edit, stored = (("cross_group_kernel<D,4>", "cross_group_kernel<D,4,EDIT>", "cross_group_kernel<D,4,STORE>")
                           if kernel == "group" else
                           ("cross_attn_kernel<…,D,4>", "cross_attn_kernel<…,D,4,DENSE>", "cross_attn_kernel<…,D,4>"))
    assert _cross(BF16, C16, d, P, 77, 8, n_groups, None, False) == plain
    assert _cross(BF16, C16, d, P, 77, 8, n_groups, DENSE, False) == edit
    assert _cross(BF16, C16, d, P, 77, 8, n_groups, None, True) == stored


def test_cross_selection_other_rows():
    # a term-plane (non-dense) program: the per-entry kernel gathers, at any size
    assert _cross(BF16, C16, 40, 4096, 77, 8, 1, TERMS, True) == "cross_attn_kernel<…,D,4>"
    # fp16 and f32 inputs: no group kernel; the dense tile with any 16-bit P V
    assert _cross(F16, C16, 40, 4096, 77, 8, 1, DENSE, True) == "cross_attn_kernel<…,D,4,DENSE>"
    assert _cross(F16, C16, 40, 4096, 77, 8, 1, None, False) == "cross_attn_kernel<…,D,4>"
    assert _cross(F32, C16, 40, 4096, 77, 8, 1, DENSE, True) == "cross_attn_kernel<…,D,4,DENSE>"
    # exact f32: no dense tile, two waves from d = 128
    assert _cross(F32, C32, 160, 256, 77, 8, 1, DENSE, True) == "cross_attn_kernel<…,D,2>"
    assert _cross(F32, C32, 128, 256, 77, 8, 1, None, False) == "cross_attn_kernel<…,D,2>"
    assert _cross(F32, C32, 80, 1024, 77, 8, 1, DENSE, True) == "cross_attn_kernel<…,D,4>"
    # the workgroup bar of the group kernel, on both sides: 2 groups x 8 heads x ceil(P / 128)
    assert _cross(BF16, C16, 40, 3969, 77, 8, 1, None, False) == "cross_group_kernel<D,4>"
    assert _cross(BF16, C16, 40, 3968, 77, 8, 1, None, False) == "cross_attn_kernel<…,D,4>"
    # rejected by the forward call: rejected here
    assert _cross(BF16, C16, 40, 4096, 97, 8, 1, None, False) is None
    assert _cross(BF16, C32, 40, 4096, 77, 8, 1, None, False) is None
    assert _cross(BF16, C16, 44, 4096, 77, 8, 1, None, False) is None
    t = _tensors(BF16, C16, 40, 4096, 77, 8, 8)
    assert _hip.cross_attn_kernel(t, _groups(4, 0, 4), False) is None        # groups do not cover the batch


def test_select_header_is_host_only(tmp_path):
    """p2p_select.h compiles alone with g++: no HIP include reaches the selection."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    src = tmp_path / "select_only.cpp"
    src.write_text('#include "p2p_select.h"\n'
                   "int main() {\n"
                   "  const int s = p2p::select_self(P2P_DTYPE_BF16, P2P_COMPUTE_BF16, 40, 4096, 4096, p2p::MODE_FUSED_,\n"
                   "                                 false, false, 0);\n"
                   "  const int c = p2p::select_cross(P2P_DTYPE_BF16, P2P_COMPUTE_BF16, 40, 2, 8, 4096, 77, false, false,\n"
                   "                                  false, 0);\n"
                   "  return !(s == p2p::SELF40_D40 && c == p2p::CROSS_GROUP && p2p::name((p2p::SelfKernel)s) &&\n"
                   "           p2p::name((p2p::CrossKernel)c));\n"
                   "}\n")
    exe = tmp_path / "select_only"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    subprocess.run([str(exe)], check=True)


def test_experiments_variant_switch_is_closed(tmp_path):
    """An experiments build honours only the named P2P_SELF_VARIANT values: at the G1 shape 0 gives the
    default kernel and 163 its stamped form; a value that names nothing (17281 once chose a kernel
    that is gone) is P2P_E_ARG from select_self and select_cross, not the default kernel."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    src = tmp_path / "select_exp.cpp"
    src.write_text('#include "p2p_select.h"\n'
                   "static int self(int variant) {\n"
                   "  return p2p::select_self(P2P_DTYPE_BF16, P2P_COMPUTE_BF16, 40, 4096, 4096, p2p::MODE_FUSED_, false,\n"
                   "                          false, variant);\n"
                   "}\n"
                   "static int cross(int variant) {\n"
                   "  return p2p::select_cross(P2P_DTYPE_BF16, P2P_COMPUTE_BF16, 40, 2, 8, 4096, 77, false, false, false,\n"
                   "                           variant);\n"
                   "}\n"
                   "int main() {\n"
                   "  if (self(0) != p2p::SELF40_D40) return 1;\n"
                   "  if (self(163) != p2p::SELF40_D40_STAMPS) return 2;\n"
                   "  if (self(17281) != P2P_E_ARG) return 3;\n"
                   "  if (cross(0) != p2p::CROSS_GROUP) return 4;\n"
                   "  if (cross(5) != P2P_E_ARG) return 5;\n"
                   "  return 0;\n"
                   "}\n")
    exe = tmp_path / "select_exp"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-DP2P_EXPERIMENTS", "-I", csrc, str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)]).returncode == 0
