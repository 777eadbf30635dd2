"""select_conv3x3_loop (csrc/p2p_select.h): which tile loop each 3x3 convolution of the SD-v1.4 U-Net
at N = 8 takes -- the 14 resnet shapes and the 6 resampling convolutions -- pinned on the CPU through
the header compiled alone with g++ (which also shows that it stays host-only).  Plans that are not
64 channels a step and 160 output channels a tile keep the register-staged loop, forced or not, and
select_conv3x3 itself answers what it answered before for all of these."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SAME, UP2, DOWN2 = 0, 1, 2
TILE, PIPE128, PIPE256 = 1, 2, 3

# (form, n, OUTPUT h, w, c_in, c_out) -> (loop, bk, bn, split)
UNET = [
    ((SAME, 8, 64, 64, 320, 320), (PIPE256, 64, 160, 1)), ((SAME, 8, 64, 64, 640, 320), (PIPE256, 64, 160, 1)),
    ((SAME, 8, 64, 64, 960, 320), (PIPE256, 64, 160, 1)),
    ((SAME, 8, 32, 32, 320, 640), (PIPE256, 64, 160, 2)), ((SAME, 8, 32, 32, 640, 640), (PIPE256, 64, 160, 2)),
    ((SAME, 8, 32, 32, 960, 640), (PIPE256, 64, 160, 2)), ((SAME, 8, 32, 32, 1280, 640), (PIPE256, 64, 160, 2)),
    ((SAME, 8, 32, 32, 1920, 640), (PIPE256, 64, 160, 2)),
    ((SAME, 8, 16, 16, 640, 1280), (PIPE256, 64, 160, 4)), ((SAME, 8, 16, 16, 1280, 1280), (PIPE256, 64, 160, 4)),
    ((SAME, 8, 16, 16, 1920, 1280), (PIPE256, 64, 160, 4)), ((SAME, 8, 16, 16, 2560, 1280), (PIPE256, 64, 160, 4)),
    ((SAME, 8, 8, 8, 1280, 1280), (PIPE128, 64, 160, 8)), ((SAME, 8, 8, 8, 2560, 1280), (PIPE128, 64, 160, 8)),
    # Upsample2D at 8 -> 16, 16 -> 32, 32 -> 64 and Downsample2D at 64 -> 32, 32 -> 16, 16 -> 8
    ((UP2, 8, 16, 16, 1280, 1280), (PIPE256, 64, 160, 4)), ((UP2, 8, 32, 32, 1280, 1280), (PIPE256, 64, 160, 1)),
    ((UP2, 8, 64, 64, 640, 640), (PIPE256, 64, 160, 1)),
    ((DOWN2, 8, 32, 32, 320, 320), (PIPE256, 64, 160, 4)), ((DOWN2, 8, 16, 16, 640, 640), (PIPE256, 64, 160, 8)),
    ((DOWN2, 8, 8, 8, 1280, 1280), (PIPE128, 64, 160, 8)),
]
# plans with bn = 128 or bk = 32, and a map that is not served: the register-staged loop
OTHER = [
    ((SAME, 3, 8, 8, 64, 64), (TILE, 64, 128, 1)), ((SAME, 2, 16, 16, 96, 320), (TILE, 32, 128, 3)),
    ((SAME, 2, 16, 16, 160, 160), (TILE, 32, 128, 5)), ((UP2, 2, 16, 16, 96, 320), (TILE, 32, 128, 3)),
    ((DOWN2, 1, 64, 64, 512, 512), (TILE, 64, 128, 4)), ((SAME, 1, 128, 128, 320, 320), (TILE, 0, 0, 0)),
]


def test_loops_and_header_is_host_only(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    checks = ""
    for i, (s, p) in enumerate(UNET + OTHER):
        checks += "  if (!row(%d, %d, %d, %d, %d, %d, %d, %d, %d, %d)) return %d;\n" % (*s, *p, i + 1)
    src = tmp_path / "select_conv_pipe.cpp"
    src.write_text('#include "p2p_select.h"\n'
                   "static bool row(int form, int n, int h, int w, int ci, int co, int loop, int bk, int bn, int split) {\n"
                   "  const p2p::ConvPlan p = p2p::select_conv3x3(form, n, h, w, ci, co);\n"
                   "  if (p.bk != bk || p.bn != bn || p.split != split) return false;\n"
                   "  if (p2p::select_conv3x3_loop(form, n, h, w, ci, co) != loop) return false;\n"
                   "  // the launch's loop: the selection's by default, a forced one only on the ring's tile\n"
                   "  if (p2p::conv3x3_loop(p2p::CONV_LOOP_AUTO, p, form, n, h, w, ci, co) != loop) return false;\n"
                   "  const bool ring = bk == 64 && bn == 160;\n"
                   "  for (int f = 1; f <= 3; ++f)\n"
                   "    if (p2p::conv3x3_loop(f, p, form, n, h, w, ci, co) != (ring ? f : (int)p2p::CONV_LOOP_TILE)) return false;\n"
                   "  return true;\n"
                   "}\n"
                   "int main() {\n" + checks +
                   "  if (p2p::conv3x3_loop_bm(p2p::CONV_LOOP_TILE) != 128 || p2p::conv3x3_loop_bm(p2p::CONV_LOOP_PIPE128) != 128 ||\n"
                   "      p2p::conv3x3_loop_bm(p2p::CONV_LOOP_PIPE256) != 256) return 101;\n"
                   "  return 0;\n"
                   "}\n")
    exe = tmp_path / "select_conv_pipe"
    csrc = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0
