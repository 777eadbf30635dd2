"""tests/kernel_matrix.py reaches every compiled instantiation of conv3x3_kernel, conv3x3_pipe_kernel and
linear_kernel, and every bias / residual state of their two reduce kernels: proved on the CPU from what
csrc/p2p_select.h answers (compiled alone with g++), never from a Python copy of its rules.

A row's plan -- select_conv3x3 and conv3x3_loop with the row's forced loop, or select_linear -- maps
to the instantiation the ``launch_*`` chains take for it.  THIS is the one place that states the
mapping; a new template parameter or launch branch is added here and to the products below.

  csrc/p2p_conv.hip, launch_conv -> launch_conv_form -> launch_conv_tile / launch_conv_pipe:
    loop PIPE128 / PIPE256 -> conv3x3_pipe_kernel<F16, BM = conv3x3_loop_bm(loop), D, PARTIAL, FORM, BIAS>
    loop TILE              -> conv3x3_kernel<F16, BK = plan.bk, NF = plan.bn / 32, PARTIAL, FORM, BIAS>
    plan.split > 1         -> PARTIAL (BIAS false), then conv3x3_reduce_kernel<F16>, which adds the bias
                              where the call has one: modes "partial" and "partial, reduce adds bias"
    else                   -> BIAS = the call has a bias: modes "bias" and "no bias"
    conv key: (family, bk, bn, BM, form, mode)
  csrc/p2p_linear.hip, launch_linear_dtype -> launch_linear_geglu / launch_linear_tile:
    form GEGLU             -> linear_kernel<F16, plan.bk, 4, EPI_GEGLU_P if p_out else EPI_GEGLU>
    plan.split > 1         -> linear_kernel<F16, plan.bk, plan.bn / 32, EPI_PARTIAL>, then
                              linear_reduce_kernel<F16> with bias and res each present or null
    else                   -> EPI_RESIDUAL for the RESIDUAL form, EPI_BIAS for the BIAS form
    linear key: (bk, bn, epilogue); reduce key: (bias, residual)
  F16 (bf16 / f16) is not part of a key: the GPU tests run every row in both."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import kernel_matrix as km
from test_select_conv_pipe import UNET

MODES = ("no bias", "bias", "partial", "partial, reduce adds bias")
# (family, bk, bn, BM): launch_conv_form's five branches
CONV_TILE_SHAPES = [("conv3x3_kernel", 64, 128, 128), ("conv3x3_kernel", 32, 128, 128), ("conv3x3_kernel", 64, 160, 128),
                    ("conv3x3_pipe_kernel", 64, 160, 128), ("conv3x3_pipe_kernel", 64, 160, 256)]
CONV_KEYS = {(*t, form, mode) for t in CONV_TILE_SHAPES for form in (km.SAME, km.UP2, km.DOWN2) for mode in MODES}
# launch_linear_dtype's branches and launch_linear_tile's / launch_linear_geglu's epilogues
LINEAR_KEYS = {(bk, bn, epi) for bk, bn in [(64, 128), (32, 128), (64, 160)] for epi in ("EPI_BIAS", "EPI_RESIDUAL", "EPI_PARTIAL")} | \
              {(bk, 128, epi) for bk in (64, 32) for epi in ("EPI_GEGLU", "EPI_GEGLU_P")}
REDUCE_KEYS = {(bias, res) for bias in (False, True) for res in (False, True)}


def conv_key(plan, form, bias):
    bk, bn, split, loop, bm = plan
    family = "conv3x3_pipe_kernel" if loop in (km.LOOP_PIPE128, km.LOOP_PIPE256) else "conv3x3_kernel"
    mode = MODES[(2 if split > 1 else 0) + (1 if bias else 0)]
    return (family, bk, bn, bm, form, mode)


def conv_name(key):
    family, bk, bn, bm, form, mode = key
    tile = f"BM = {bm}" if family == "conv3x3_pipe_kernel" else f"BK = {bk}, NF = {bn // 32}"
    return f"{family}<{tile}, FORM = {km.FORM_NAMES[form]}>, {mode}"


def linear_key(plan, form, p_out):
    bk, bn, split, cols = plan
    if form == km.LIN_GEGLU:
        return (bk, bn, "EPI_GEGLU_P" if p_out else "EPI_GEGLU")
    return (bk, bn, "EPI_PARTIAL" if split > 1 else "EPI_RESIDUAL" if form == km.LIN_RESIDUAL else "EPI_BIAS")


def rows_class(m):
    return "one row" if m == 1 else "below half a tile" if m < 64 else "odd" if m % 2 else "a tile and a tail" if m > 128 else "?"


def unet_input_row(sizes):
    """test_select_conv_pipe.UNET's rows carry the OUTPUT map; the table's and the C API's the input map."""
    form, n, oh, ow, c_in, c_out = sizes
    h, w = {km.SAME: (oh, ow), km.UP2: (oh // 2, ow // 2), km.DOWN2: (2 * oh, 2 * ow)}[form]
    return (form, n, h, w, c_in, c_out)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """What the header answers for every row of the table and of UNET: (conv plans, linear plans, UNET
    plans); conv (bk, bn, split, loop, BM), linear (bk, bn, split, output columns of a tile)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    conv = [(*r[:6], r[7]) for r in km.CONV_ROWS] + [(*unet_input_row(s), km.LOOP_AUTO) for s, _ in UNET]
    calls = "".join("  conv(%d, %d, %d, %d, %d, %d, %d);\n" % c for c in conv)
    calls += "".join("  linear(%d, %d, %d, %d);\n" % r[:4] for r in km.LINEAR_ROWS)
    tmp = tmp_path_factory.mktemp("select_instances")
    src = tmp / "select_instances.cpp"
    src.write_text('#include <stdio.h>\n#include "p2p_select.h"\n'
                   "static void conv(int form, int n, int ih, int iw, int ci, int co, int forced) {\n"
                   "  int oh = 0, ow = 0;\n"
                   "  if (p2p::conv3x3_check_sizes(form, n, ih, iw, ci, co) != 0 || !p2p::conv3x3_out_map(form, ih, iw, &oh, &ow)) {\n"
                   '    printf("C 0 0 0 0 0\\n");\n'
                   "    return;\n"
                   "  }\n"
                   "  const p2p::ConvPlan p = p2p::select_conv3x3(form, n, oh, ow, ci, co);\n"
                   "  const int loop = p2p::conv3x3_loop(forced, p, form, n, oh, ow, ci, co);\n"
                   '  printf("C %d %d %d %d %d\\n", p.bk, p.bn, p.split, loop, p2p::conv3x3_loop_bm(loop));\n'
                   "}\n"
                   "static void linear(int form, int m, int k, int n) {\n"
                   "  const p2p::LinearPlan p = p2p::select_linear(form, m, k, n);\n"
                   '  printf("L %d %d %d %d\\n", p.bk, p.bn, p.split, p.split > 0 ? p2p::linear_tile_cols(form, p) : 0);\n'
                   "}\n"
                   "int main() {\n" + calls + "  return 0;\n}\n")
    exe = tmp / "select_instances"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    lines = [ln.split() for ln in out if ln]
    assert len(lines) == len(conv) + len(km.LINEAR_ROWS)
    assert all(ln[0] == "C" for ln in lines[:len(conv)]) and all(ln[0] == "L" for ln in lines[len(conv):])
    answers = [tuple(int(v) for v in ln[1:]) for ln in lines]
    assert all(a[2] >= 1 for a in answers), "the selection declines a row"
    n_table = len(km.CONV_ROWS)
    return answers[:n_table], answers[len(conv):], answers[n_table:len(conv)]


def test_conv_rows_are_the_full_product(plans):
    """One row per (kernel family, tile, form, mode), and no key without its row: taking any row out of the
    table leaves its instantiation (or the reduce's bias state behind it) unreached, and named here."""
    keys = [conv_key(p, r[0], r[6]) for p, r in zip(plans[0], km.CONV_ROWS)]
    missing, extra = CONV_KEYS - set(keys), set(keys) - CONV_KEYS
    assert not missing, "no row of kernel_matrix.CONV_ROWS reaches: " + "; ".join(sorted(map(conv_name, missing)))
    assert not extra, "rows outside the product (a new launch branch? add it to CONV_KEYS): " + "; ".join(sorted(map(conv_name, extra)))
    assert len(keys) == len(CONV_KEYS) == 60, "two rows reach the same instantiation in the same mode"
    # every row: n = 3 images and an 8 x 8 output map, on the loop it forces
    for (bk, bn, split, loop, bm), r in zip(plans[0], km.CONV_ROWS):
        assert r[1] == 3 and r[2:4] == km.CONV_INPUT_MAP[r[0]]
        assert loop == r[7], f"{km.conv_id(r)}: the plan does not take the forced loop"


def test_linear_rows_reach_every_epilogue_and_reduce_state(plans):
    keys = {linear_key(p, r[0], r[6]) for p, r in zip(plans[1], km.LINEAR_ROWS)}
    missing, extra = LINEAR_KEYS - keys, keys - LINEAR_KEYS
    assert not missing, "no row of kernel_matrix.LINEAR_ROWS reaches linear_kernel<bk, bn / 32, epilogue>: " + str(sorted(missing))
    assert not extra, "rows outside the product (a new launch branch? add it to LINEAR_KEYS): " + str(sorted(extra))
    reduce = {(r[4], r[0] == km.LIN_RESIDUAL) for p, r in zip(plans[1], km.LINEAR_ROWS) if p[2] > 1}
    assert reduce == REDUCE_KEYS, "linear_reduce_kernel (bias, residual) states without a row: " + str(sorted(REDUCE_KEYS - reduce))
    # both tile widths and a step count that the split does not divide: ranges of 8 and 9 steps
    uneven = {(p[0], p[1]) for p, r in zip(plans[1], km.LINEAR_ROWS) if p[2] > 1 and (r[2] // p[0]) % p[2]}
    assert uneven == {(64, 128), (32, 128), (64, 160)}, uneven


def test_every_linear_row_is_needed(plans):
    """The rows are the product of (plan with its column tiles, row count class, form, bias, layout, p_out)
    the table sets out to run, each once: taking any row out leaves one of them unreached, and named."""
    def case(p, r):
        form, m, k, n, bias, strided, p_out = r
        return ((p[0], p[1], p[2], -(-n // p[3])), rows_class(m), km.LIN_NAMES[form], bias, strided, p_out)
    got = [case(p, r) for p, r in zip(plans[1], km.LINEAR_ROWS)]
    full = [(64, 128, 1, 1), (64, 128, 2, 1), (32, 128, 1, 1), (32, 128, 2, 1), (64, 160, 1, 1), (64, 160, 2, 1)]
    small = [(64, 160, 1, 1), (64, 160, 2, 1), (64, 128, 2, 3)]
    shapes = [(p, "a tile and a tail") for p in full] + \
             [(p, c) for p in small for c in ("one row", "below half a tile", "odd")]
    want = {(p, c, form, bias, strided, False) for p, c in shapes for form in ("bias", "residual")
            for bias in (False, True) for strided in (False, True)}
    geglu = [((64, 128, 1, 2), "a tile and a tail"), ((32, 128, 1, 2), "a tile and a tail"), ((64, 128, 1, 1), "below half a tile")]
    want |= {(p, c, "geglu", bias, False, p_out) for p, c in geglu for bias in (False, True) for p_out in (False, True)}
    assert not want - set(got), "no row of kernel_matrix.LINEAR_ROWS runs: " + str(sorted(want - set(got)))
    assert not set(got) - want, "rows outside the product: " + str(sorted(set(got) - want))
    assert len(got) == len(want), "two rows run the same case"


def test_every_production_conv_is_in_the_table(plans):
    """Every 3x3 convolution of the U-Net at N = 8 (test_select_conv_pipe.UNET) runs an instantiation, in
    a mode, that the table runs at its small shape -- none is left to full-size runs.  The resnets call
    p2p_conv3x3 without a bias (the next kernel adds it); Upsample2D / Downsample2D pass theirs."""
    table = {conv_key(p, r[0], r[6]) for p, r in zip(plans[0], km.CONV_ROWS)}
    for p, (sizes, pinned) in zip(plans[2], UNET):
        assert (p[3], p[0], p[1], p[2]) == pinned, sizes
        key = conv_key(p, sizes[0], sizes[0] != km.SAME)
        assert key in table, f"U-Net convolution {sizes} runs {conv_name(key)}, which no row of the table reaches"
