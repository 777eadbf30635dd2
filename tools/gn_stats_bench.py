"""GroupNorm on the VAE's norm shapes: this tree's library against another build of it (the parent
commit's, whose statistics run one workgroup per slab at every size), runs alternated.  Prints one
line per shape: the p2p_group_norm call (statistics + apply; the apply kernel is the same in both)
in microseconds, median of --iters, and whether the outputs agree.

    python tools/gn_stats_bench.py --other-lib /path/to/parent/libp2p_hip.so [--iters 20]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prompt-to-prompt_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from p2p_amd import _hip  # noqa: E402

# (what, N, C, H, W): the decoder's norms, 32 groups, from the mid block up; slab = C / 32 * H * W
SHAPES = [("512 ch @ 64^2", 1, 512, 64, 64), ("512 ch @ 128^2", 1, 512, 128, 128), ("256 ch @ 256^2", 1, 256, 256, 256),
          ("512 ch @ 256^2", 1, 512, 256, 256), ("128 ch @ 512^2", 1, 128, 512, 512), ("256 ch @ 512^2", 1, 256, 512, 512),
          ("128 ch @ 512^2, N = 4", 4, 128, 512, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", required=True)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gn_stats_bench needs a GPU")
    dev = torch.device("cuda:0")
    new = _hip.lib()
    _hip.check_source_hash()
    old = ctypes.CDLL(args.other_lib)
    old.p2p_group_norm.argtypes = [ctypes.POINTER(_hip.GroupNormArgs), ctypes.c_void_p]
    old.p2p_source_hash.restype = ctypes.c_char_p
    print(f"this tree {new.p2p_source_hash().decode()}  other {old.p2p_source_hash().decode()}  "
          f"bf16, silu, NCHW out, median of {args.iters} alternated calls, us per call (statistics + apply)")
    stream = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(0)
    for what, N, C, H, W in SHAPES:
        x = (torch.randn(N, C, H, W, device=dev, generator=g) * 2 + 0.5).to(torch.bfloat16)
        gamma = torch.randn(C, device=dev, generator=g).to(torch.bfloat16)
        beta = torch.randn(C, device=dev, generator=g).to(torch.bfloat16)
        ys = {}
        a = {}
        floats = int(new.p2p_group_norm_stats_floats(N, C, H * W, 32))
        for name in ("new", "old"):
            y = torch.empty_like(x)
            stats = torch.empty(floats, dtype=torch.float32, device=dev)
            s = _hip.GroupNormArgs()
            s.x, s.gamma, s.beta, s.y, s.stats = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), stats.data_ptr()
            s.n, s.channels, s.hw, s.groups = N, C, H * W, 32
            s.eps, s.act, s.y_layout, s.dtype = 1e-6, _hip.ACT_SILU, _hip.LAYOUT_NCHW, _hip.P2P_DTYPE_BF16
            ys[name], a[name] = (y, stats), s
        libs = {"new": new, "old": old}
        times = {"new": [], "old": []}
        for it in range(args.iters + 3):
            for name in ("new", "old"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = libs[name].p2p_group_norm(ctypes.byref(a[name]), stream)
                e1.record()
                e1.synchronize()
                assert rc == 0, (name, rc)
                if it >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        lo = {k: min(v) for k, v in times.items()}
        diff = (ys["new"][0].float() - ys["old"][0].float()).abs().max().item()
        slab = C // 32 * H * W
        print(f"{what:24s} slab {slab:8d}  this tree {med['new']:9.1f} (min {lo['new']:9.1f})   other {med['old']:9.1f} "
              f"(min {lo['old']:9.1f})   max |dy| {diff:.3e}")


if __name__ == "__main__":
    main()
