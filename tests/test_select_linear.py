"""select_linear (csrc/p2p_select.h): the tile shape and K split of linear_kernel for the two GEMMs of
the U-Net's four feed-forward geometries at N = 8 and for the shapes of tests/test_gpu_linear.py and
tests/test_gpu_linear_modules.py, pinned on the CPU -- the split through p2p_linear_split, the tile
through the header compiled alone with g++ (which also shows that the header stays host-only)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

from p2p_amd import _hip

BIAS, GEGLU, RES = _hip.LINEAR_BIAS, _hip.LINEAR_GEGLU, _hip.LINEAR_RESIDUAL

# (form, m, k, n) -> (bk, bn, split); n: output columns; split 0 = left to the caller's GEMM
ROWS = [
    # the feed-forwards at N = 8: ff.net[0] (GEGLU, [M, C] -> [M, 4 C]) and ff.net[2] + residual ([M, 4 C] -> [M, C])
    ((GEGLU, 32768, 320, 1280), (64, 128, 1)), ((RES, 32768, 1280, 320), (64, 160, 1)),
    # (the K-split output GEMMs and the 8 x 8 GEGLU GEMM measured slower than hipBLASLt's chain: declined)
    ((GEGLU, 8192, 640, 2560), (64, 128, 1)), ((RES, 8192, 2560, 640), (0, 0, 0)),
    ((GEGLU, 2048, 1280, 5120), (64, 128, 1)), ((RES, 2048, 5120, 1280), (0, 0, 0)),
    ((GEGLU, 512, 1280, 5120), (0, 0, 0)), ((RES, 512, 5120, 1280), (0, 0, 0)),
    # a declined weight is declined up to the rows it was measured at, and served above them
    ((RES, 4096, 2560, 640), (0, 0, 0)), ((RES, 16384, 2560, 640), (64, 160, 1)), ((GEGLU, 640, 1280, 5120), (64, 128, 1)),
    # tests/test_gpu_linear.py
    ((BIAS, 136, 64, 96), (64, 128, 1)), ((RES, 136, 64, 96), (64, 128, 1)), ((GEGLU, 136, 64, 96), (64, 128, 1)),
    ((BIAS, 136, 96, 96), (32, 128, 1)), ((RES, 136, 96, 96), (32, 128, 1)), ((GEGLU, 136, 96, 96), (32, 128, 1)),
    ((BIAS, 136, 320, 320), (64, 160, 1)), ((RES, 136, 320, 320), (64, 160, 1)), ((GEGLU, 264, 320, 160), (64, 128, 1)),
    ((BIAS, 128, 2560, 160), (64, 160, 5)), ((RES, 128, 2560, 160), (64, 160, 5)),
    ((RES, 136, 1024, 96), (64, 128, 2)), ((RES, 136, 768, 96), (64, 128, 1)),
    # tests/test_gpu_linear_modules.py and tests/test_gpu_unet_grad_modules.py
    ((GEGLU, 128, 64, 256), (64, 128, 1)), ((RES, 128, 256, 64), (64, 128, 1)),
    ((GEGLU, 512, 128, 512), (64, 128, 1)), ((RES, 512, 512, 128), (64, 128, 1)),
    ((GEGLU, 512, 64, 256), (64, 128, 1)),
    # the GEGLU form is never split, however few its tiles
    ((GEGLU, 128, 2560, 64), (64, 128, 1)),
]


@pytest.mark.parametrize("sizes,plan", ROWS, ids=lambda v: "x".join(map(str, v)))
def test_split(sizes, plan):
    form, m, k, n = sizes
    assert _hip.linear_split(*sizes) == plan[2]
    want_ws = plan[2] * n * ((m + 127) // 128 * 128) if plan[2] > 1 else 0
    assert _hip.lib().p2p_linear_workspace_floats(*sizes) == want_ws


def test_tiles_and_header_is_host_only(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    checks = "".join("  if (!same(p2p::select_linear(%d, %d, %d, %d), %d, %d, %d)) return %d;\n" % (*s, *p, i + 1)
                     for i, (s, p) in enumerate(ROWS))
    src = tmp_path / "select_linear.cpp"
    src.write_text('#include "p2p_select.h"\n'
                   "static bool same(p2p::LinearPlan p, int bk, int bn, int split) {\n"
                   "  return p.bk == bk && p.bn == bn && p.split == split;\n"
                   "}\n"
                   "int main() {\n" + checks +
                   "  if (p2p::linear_check_sizes(P2P_LINEAR_BIAS, 128, 48, 64) != P2P_E_ALIGN) return 101;\n"
                   "  if (p2p::linear_check_sizes(P2P_LINEAR_GEGLU, 128, 64, 20) != P2P_E_ALIGN) return 102;\n"
                   "  if (p2p::linear_check_sizes(P2P_LINEAR_BIAS, 1 << 20, 4096, 64) != P2P_E_ARG) return 103;\n"
                   "  if (p2p::linear_check_sizes(7, 128, 64, 64) != P2P_E_ARG) return 104;\n"
                   "  if (p2p::select_linear(P2P_LINEAR_BIAS, 128, 48, 64).split != 0) return 105;\n"
                   "  return 0;\n"
                   "}\n")
    exe = tmp_path / "select_linear"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
