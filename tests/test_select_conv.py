"""select_conv3x3 (csrc/p2p_select.h): the tile shape and K split of conv3x3_kernel for every resnet
shape of the SD-v1.4 U-Net at N = 8 and for the shapes of tests/test_gpu_conv.py, pinned on the CPU
-- the split through p2p_conv3x3_split, the tile through the header compiled alone with g++ (which
also shows that the header stays host-only)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

from p2p_amd import _hip

# (n, h, w, c_in, c_out) -> (bk, bn, split); split 0 = left to the caller's convolution
ROWS = [
    # the U-Net's resnets at N = 8
    ((8, 64, 64, 320, 320), (64, 160, 1)), ((8, 64, 64, 640, 320), (64, 160, 1)), ((8, 64, 64, 960, 320), (64, 160, 1)),
    ((8, 32, 32, 320, 640), (64, 160, 2)), ((8, 32, 32, 640, 640), (64, 160, 2)), ((8, 32, 32, 960, 640), (64, 160, 2)),
    ((8, 32, 32, 1280, 640), (64, 160, 2)), ((8, 32, 32, 1920, 640), (64, 160, 2)),
    ((8, 16, 16, 640, 1280), (64, 160, 4)), ((8, 16, 16, 1280, 1280), (64, 160, 4)),
    ((8, 16, 16, 1920, 1280), (64, 160, 4)), ((8, 16, 16, 2560, 1280), (64, 160, 4)),
    ((8, 8, 8, 1280, 1280), (64, 160, 8)), ((8, 8, 8, 2560, 1280), (64, 160, 8)),
    # tests/test_gpu_conv.py
    ((3, 8, 8, 64, 64), (64, 128, 1)), ((1, 8, 8, 64, 96), (64, 128, 1)),
    ((2, 8, 16, 64, 128), (64, 128, 1)), ((2, 16, 8, 64, 128), (64, 128, 1)),
    ((2, 16, 16, 96, 320), (32, 128, 3)),
    ((2, 8, 8, 1280, 1280), (64, 160, 8)), ((1, 16, 16, 2560, 1280), (64, 160, 8)),
    ((2, 16, 16, 64, 128), (64, 128, 1)), ((2, 16, 16, 128, 128), (64, 128, 2)),     # the module tests' ResnetBlock2D
    # a map above 64 x 64 (the VAE's): not served
    ((1, 128, 128, 128, 128), (0, 0, 0)), ((1, 64, 128, 512, 512), (0, 0, 0)),
    # 64 x 64 itself is
    ((1, 64, 64, 512, 512), (64, 128, 4)),
]


@pytest.mark.parametrize("sizes,plan", ROWS, ids=lambda v: "x".join(map(str, v)))
def test_split(sizes, plan):
    assert _hip.conv3x3_split(*sizes) == plan[2]
    want_ws = plan[2] * sizes[0] * sizes[1] * sizes[2] * sizes[4] if plan[2] > 1 else 0
    assert _hip.lib().p2p_conv3x3_workspace_floats(*sizes) == want_ws


def test_tiles_and_header_is_host_only(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    checks = "".join("  if (!same(p2p::select_conv3x3(%d, %d, %d, %d, %d), %d, %d, %d)) return %d;\n" % (*s, *p, i + 1)
                     for i, (s, p) in enumerate(ROWS))
    src = tmp_path / "select_conv.cpp"
    src.write_text('#include "p2p_select.h"\n'
                   "static bool same(p2p::ConvPlan p, int bk, int bn, int split) {\n"
                   "  return p.bk == bk && p.bn == bn && p.split == split;\n"
                   "}\n"
                   "int main() {\n" + checks +
                   "  if (p2p::conv3x3_check_sizes(2, 8, 8, 48, 64) != P2P_E_ALIGN) return 101;\n"
                   "  if (p2p::conv3x3_check_sizes(65536, 256, 256, 64, 64) != P2P_E_ARG) return 102;\n"
                   "  return 0;\n"
                   "}\n")
    exe = tmp_path / "select_conv"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
