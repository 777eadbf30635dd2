"""The transformer blocks' feed-forward GEMMs at the four geometries the SD-v1.4 U-Net runs with
N = 8, in tools/conv_bench.py's method: the chain a block ran before linear_kernel (hipBLASLt's
F.linear + p2p_geglu for ff.net[0]; F.linear + torch's add for ff.net[2] and the residual) against
the p2p_linear launch that replaces it (GEGLU form; RESIDUAL form with its reduce launch where K is
split).  Every variant is captured into a HIP graph of --reps calls that rotate over enough operand
sets to exceed the 256 MB Infinity Cache, and the graph's replays are timed with events.  Random
operands, weights scaled by K^-1/2.  --repeat R measures every chain R times; a shape counts as
adopted only if every one of its medians beats every median of the chain it replaces.

Prints per GEMM: microseconds per call (median of --iters replays) of both chains, the p2p_linear
launch's TFLOP/s (the reduce included where there is one) and its fraction of the 2500 TFLOP/s dense
16-bit peak, the selection's K split and the verdict.  A shape the selection declines is measured on
hipBLASLt only.

    python tools/linear_bench.py [--iters 15] [--reps 32] [--dtype bf16|f16] [--n 8] [--repeat 3]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prompt-to-prompt_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_bench import PEAK_TFLOPS, graph_us  # noqa: E402
from p2p_amd import _hip  # noqa: E402

# (H = W, C, how many of the U-Net's 16 transformer blocks have the geometry): M = N H W tokens
SHAPES = [(64, 320, 5), (32, 640, 5), (16, 1280, 5), (8, 1280, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("linear_bench needs a GPU")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    _hip.lib()
    _hip.check_source_hash()
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{torch.cuda.get_device_name(0)}, {args.dtype}, N = {args.n}, graphs of {args.reps} calls, median of {args.iters} "
          f"replays, every chain {args.repeat} times")
    print("us per call: [before] F.linear + p2p_geglu (ff.net[0]) / F.linear + torch add (ff.net[2]) || [now] p2p_linear")

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, device=dev, generator=g) * scale).to(dtype)

    saved = 0.0
    with torch.no_grad():
        for res, C, count in SHAPES:
            M = args.n * res * res
            # ff.net[0]: [M, C] -> GEGLU -> [M, 4 C]; ff.net[2] + residual: [M, 4 C] -> [M, C]
            for name, form, K, N in (("geglu   ", _hip.LINEAR_GEGLU, C, 4 * C), ("residual", _hip.LINEAR_RESIDUAL, 4 * C, C)):
                geglu = form == _hip.LINEAR_GEGLU
                rows = 2 * N if geglu else N
                per_set = (M * K + rows * K + M * rows + M * N) * 2
                sets = min(16, max(2, math.ceil(600e6 / per_set)))
                xs = [rnd(M, K) for _ in range(sets)]
                ws = [rnd(rows, K, scale=K ** -0.5) for _ in range(sets)]
                bs = [rnd(rows) for _ in range(sets)]
                ss = [None if geglu else rnd(M, N) for _ in range(sets)]

                def before(i):
                    if geglu:
                        return _hip.geglu(F.linear(xs[i], ws[i], bs[i]))
                    return F.linear(xs[i], ws[i], bs[i]) + ss[i]

                def now(i):
                    out = _hip.linear(xs[i], ws[i], bs[i], form, res=ss[i])
                    assert out is not None
                    return out

                split = _hip.linear_split(form, M, K, N)
                gflop = 2.0 * M * K * rows / 1e9
                b_us = [graph_us(before, sets, args.reps, args.iters, dev) for _ in range(args.repeat)]
                line = (f"  {res:2d}^2 C={C:4d} {name} M={M:5d} K={K:4d} N={rows:5d} (x{count}) {gflop:6.1f} GFLOP  before " +
                        " ".join(f"{u:7.1f}" for u in b_us))
                if split >= 1:
                    n_us = [graph_us(now, sets, args.reps, args.iters, dev) for _ in range(args.repeat)]
                    med_b, med_n = sorted(b_us)[len(b_us) // 2], sorted(n_us)[len(n_us) // 2]
                    tf = gflop / med_n * 1e3
                    wins = max(n_us) < min(b_us)
                    line += (" || now " + " ".join(f"{u:7.1f}" for u in n_us) +
                             f" ({tf:5.0f} TF, {100 * tf / PEAK_TFLOPS:4.1f} % of peak)  split {split}  chain {med_b / med_n:.2f}x  "
                             f"{'wins' if wins else 'LOSES: every median must beat every median'}")
                    if wins:
                        saved += count * (med_b - med_n)
                else:
                    line += " || declined by the selection: stays on hipBLASLt"
                print(line, flush=True)
                del xs, ws, bs, ss
    print(f"sum over the winning feed-forward GEMMs of a U-Net call: {saved / 1e3:.3f} ms less per call")


if __name__ == "__main__":
    main()
