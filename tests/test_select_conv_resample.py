"""The sampling forms of the convolution's selection (csrc/p2p_select.h): plan and workspace size of
conv3x3_kernel's Up2 and Down2 forms for the six resampling convolutions of the SD-v1.4 U-Net at
N = 8 and for the shapes of tests/test_gpu_conv_resample.py, pinned on the CPU -- the split through
p2p_conv3x3_ex_split, the tile through the header compiled alone with g++, which also checks that
the 5-argument select_conv3x3 rows of tests/test_select_conv.py still hold beside the new overload."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

from p2p_amd import _hip

from test_select_conv import ROWS as SAME_ROWS

SAME, UP2, DOWN2 = _hip.CONV_SAME, _hip.CONV_UP2, _hip.CONV_DOWN2

# (form, n, input h, input w, c_in, c_out) -> (bk, bn, split); split 0 = left to the caller's convolution
ROWS = [
    # the U-Net's Upsample2D and Downsample2D at N = 8
    ((UP2, 8, 8, 8, 1280, 1280), (64, 160, 4)), ((UP2, 8, 16, 16, 1280, 1280), (64, 160, 1)),
    ((UP2, 8, 32, 32, 640, 640), (64, 160, 1)),
    ((DOWN2, 8, 64, 64, 320, 320), (64, 160, 4)), ((DOWN2, 8, 32, 32, 640, 640), (64, 160, 8)),
    ((DOWN2, 8, 16, 16, 1280, 1280), (64, 160, 8)),
    # tests/test_gpu_conv_resample.py
    ((UP2, 3, 4, 4, 64, 64), (64, 128, 1)), ((UP2, 1, 4, 4, 64, 96), (64, 128, 1)), ((UP2, 2, 3, 4, 64, 64), (64, 128, 1)),
    ((UP2, 2, 4, 8, 64, 128), (64, 128, 1)), ((UP2, 2, 8, 4, 64, 128), (64, 128, 1)), ((UP2, 2, 8, 8, 96, 320), (32, 128, 3)),
    ((UP2, 2, 4, 4, 1280, 1280), (64, 160, 8)),
    ((DOWN2, 3, 16, 16, 64, 64), (64, 128, 1)), ((DOWN2, 1, 16, 16, 64, 96), (64, 128, 1)),
    ((DOWN2, 2, 16, 32, 64, 128), (64, 128, 1)), ((DOWN2, 2, 32, 16, 64, 128), (64, 128, 1)),
    ((DOWN2, 2, 32, 32, 96, 320), (32, 128, 3)), ((DOWN2, 2, 16, 16, 1280, 1280), (64, 160, 8)),
    ((SAME, 3, 8, 8, 64, 64), (64, 128, 1)), ((SAME, 2, 8, 8, 1280, 1280), (64, 160, 8)),
    ((UP2, 2, 8, 8, 64, 64), (64, 128, 1)), ((DOWN2, 2, 16, 16, 64, 64), (64, 128, 1)),       # the module tests
    # an output map above 64 x 64: not served; 64 x 64 itself is
    ((UP2, 1, 64, 64, 128, 128), (0, 0, 0)), ((UP2, 1, 32, 64, 128, 128), (0, 0, 0)), ((DOWN2, 1, 256, 256, 128, 128), (0, 0, 0)),
    ((UP2, 1, 32, 32, 512, 512), (64, 128, 4)), ((DOWN2, 1, 128, 128, 512, 512), (64, 128, 4)),
]
E_ARG, E_ALIGN = -1, -6
# sizes the entry answers with a code: odd input sizes for Down2, h_out w_out % 8 != 0, an unknown form
CODES = [
    ((DOWN2, 2, 15, 16, 64, 64), E_ALIGN), ((DOWN2, 2, 16, 15, 64, 64), E_ALIGN), ((DOWN2, 2, 7, 7, 64, 64), E_ALIGN),
    ((UP2, 2, 1, 1, 64, 64), E_ALIGN), ((UP2, 2, 3, 3, 64, 64), E_ALIGN), ((DOWN2, 2, 6, 6, 64, 64), E_ALIGN),
    ((DOWN2, 2, 2, 2, 64, 64), E_ALIGN),
    ((3, 2, 8, 8, 64, 64), E_ARG), ((-1, 2, 8, 8, 64, 64), E_ARG),
]


def out_map(form, h, w):
    return {SAME: (h, w), UP2: (2 * h, 2 * w), DOWN2: (h // 2, w // 2)}[form]


@pytest.mark.parametrize("sizes,plan", ROWS, ids=lambda v: "x".join(map(str, v)))
def test_split_and_workspace(sizes, plan):
    form, n, h, w, c_in, c_out = sizes
    assert _hip.conv3x3_ex_split(*sizes) == plan[2]
    oh, ow = out_map(form, h, w)
    want_ws = plan[2] * n * oh * ow * c_out if plan[2] > 1 else 0
    assert _hip.lib().p2p_conv3x3_ex_workspace_floats(*sizes) == want_ws
    assert _hip.conv3x3_out_map(form, h, w) == (oh, ow)
    # tile and split come from the output M exactly as for the Same form
    assert plan[2] == _hip.conv3x3_split(n, oh, ow, c_in, c_out)


@pytest.mark.parametrize("sizes,code", CODES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_not_served_sizes(sizes, code):
    assert _hip.conv3x3_ex_split(*sizes) == code
    assert _hip.lib().p2p_conv3x3_ex_workspace_floats(*sizes) == code


def test_tiles_and_both_overloads(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    checks = ""
    for i, ((form, n, h, w, c_in, c_out), p) in enumerate(ROWS):
        oh, ow = out_map(form, h, w)
        checks += ("  if (!p2p::conv3x3_out_map(%d, %d, %d, &oh, &ow) || oh != %d || ow != %d) return %d;\n"
                   % (form, h, w, oh, ow, i + 1))
        checks += ("  if (!same(p2p::select_conv3x3(%d, %d, oh, ow, %d, %d), %d, %d, %d)) return %d;\n"
                   % (form, n, c_in, c_out, *p, i + 1))
    old = "".join("  if (!same(p2p::select_conv3x3(%d, %d, %d, %d, %d), %d, %d, %d)) return %d;\n" % (*s, *p, 100 + i)
                  for i, (s, p) in enumerate(SAME_ROWS))
    src = tmp_path / "select_conv_resample.cpp"
    src.write_text('#include "p2p_select.h"\n'
                   "static bool same(p2p::ConvPlan p, int bk, int bn, int split) {\n"
                   "  return p.bk == bk && p.bn == bn && p.split == split;\n"
                   "}\n"
                   "int main() {\n"
                   "  int oh = 0, ow = 0;\n" + checks + old +
                   "  if (p2p::conv3x3_out_map(P2P_CONV_DOWN2, 15, 16, &oh, &ow)) return 201;\n"
                   "  if (p2p::conv3x3_out_map(7, 16, 16, &oh, &ow)) return 202;\n"
                   "  if (p2p::select_conv3x3(7, 2, 8, 8, 64, 64).split != 0) return 203;\n"
                   "  if (p2p::conv3x3_check_sizes(P2P_CONV_DOWN2, 2, 15, 16, 64, 64) != P2P_E_ALIGN) return 204;\n"
                   "  if (p2p::conv3x3_check_sizes(P2P_CONV_UP2, 2, 3, 3, 64, 64) != P2P_E_ALIGN) return 205;\n"
                   "  if (p2p::conv3x3_check_sizes(7, 2, 8, 8, 64, 64) != P2P_E_ARG) return 206;\n"
                   "  if (p2p::conv3x3_check_sizes(P2P_CONV_DOWN2, 8192, 128, 128, 64, 64) != P2P_E_ARG) return 207;\n"
                   "  return 0;\n"
                   "}\n")
    exe = tmp_path / "select_conv_resample"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
