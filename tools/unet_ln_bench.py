"""The transformer blocks' LayerNorm (+ residual add) and the U-Net's time path, per launch, at the
shapes the SD-v1.4 U-Net runs with N = 8: p2p_layer_norm of this tree, the same entry point of
another build (--other-lib: the parent commit's, one wave per row at every width) and the torch
launches they replace.  Every variant is captured into a HIP graph of --reps calls that rotate over
enough operand sets to exceed the 256 MB Infinity Cache at the large shapes, and the graph's replays
are timed with events: an eager host-timed loop floors at the enqueue cost.  Prints one line per
shape and variant: microseconds per call (median of --iters replays), algorithmic bytes, TB/s.

    python tools/unet_ln_bench.py [--other-lib /path/to/libp2p_hip.so] [--iters 15] [--reps 32] [--dtype bf16|f16]
"""
import argparse
import ctypes
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prompt-to-prompt_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from p2p_amd import _hip, unet  # noqa: E402

# rows x C of the token tensors at 64^2, 32^2, 16^2 and 8^2, N = 8, and how many of the U-Net's 16
# blocks run there (x 3 norms each)
SHAPES = [(32768, 320, 5), (8192, 640, 5), (2048, 1280, 5), (512, 1280, 1)]


def graph_us(fn, sets, reps, iters, dev):
    """fn(i) enqueues one call on operand set i; microseconds per call from replays of a graph of reps calls."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for i in range(sets):
            fn(i)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for r in range(reps):
            fn(r % sets)
    times = []
    for it in range(iters + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        if it >= 2:
            times.append(e0.elapsed_time(e1) * 1e3 / reps)
    return sorted(times)[len(times) // 2]


def ln_call(lib, x, add, gamma, beta, s, y, stream):
    a = _hip.LayerNormArgs()
    a.x, a.gamma, a.beta, a.y = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr()
    if add is not None:
        a.add, a.sum_out = add.data_ptr(), s.data_ptr()
    a.rows, a.channels, a.eps, a.dtype = x.shape[0], x.shape[1], 1e-5, _hip._glue_dtype(x)
    rc = lib.p2p_layer_norm(ctypes.byref(a), stream)
    assert rc == 0, rc


def layer_norms(args, dev, dtype, libs):
    g = torch.Generator(device=dev).manual_seed(0)
    print("LayerNorm: us per call; bytes = x (+ add) read, y (+ sum) written")
    for rows, C, blocks in SHAPES:
        tensor = rows * C * 2
        sets = min(16, max(2, math.ceil(600e6 / (4 * tensor))))
        ops = [[torch.randn(rows, C, device=dev, generator=g).to(dtype) for _ in range(2)] +
               [torch.empty(rows, C, device=dev, dtype=dtype) for _ in range(2)] for _ in range(sets)]
        gamma, beta = torch.randn(C, device=dev, generator=g).to(dtype), torch.randn(C, device=dev, generator=g).to(dtype)

        def stream():
            return torch.cuda.current_stream(dev).cuda_stream

        variants = {}
        for name, lib in libs.items():
            variants[f"{name} plain"] = (2, lambda i, lib=lib: ln_call(lib, ops[i][0], None, gamma, beta, None, ops[i][3], stream()))
            variants[f"{name} add+sum"] = (4, lambda i, lib=lib: ln_call(lib, ops[i][0], ops[i][1], gamma, beta, ops[i][2],
                                                                       ops[i][3], stream()))
        variants["torch layer_norm"] = (2, lambda i: F.layer_norm(ops[i][0], (C,), gamma, beta, 1e-5))
        variants["torch add"] = (3, lambda i: torch.add(ops[i][0], ops[i][1], out=ops[i][2]))
        variants["torch add, layer_norm"] = (4, lambda i: F.layer_norm(torch.add(ops[i][0], ops[i][1], out=ops[i][2]), (C,),
                                                                       gamma, beta, 1e-5))
        for name, (passes, fn) in variants.items():
            us = graph_us(fn, sets, args.reps, args.iters, dev)
            mb = passes * tensor / 1e6
            # MB per us is TB/s
            print(f"  {rows:6d} x {C:4d} ({blocks} blocks)  {name:28s} {us:8.2f} us  {mb:7.1f} MB  {mb / us:6.2f} TB/s")
        del ops


def time_path(args, dev, dtype):
    print("time path: us per U-Net call (N timesteps -> emb -> the 22 projections)")
    torch.manual_seed(0)
    model = unet.UNet2DConditionModel().to(dev, dtype).eval()
    te, linears = model.time_embedding, model._time_linears
    table = _hip.TimeProjTable([(m.weight, m.bias) for m in linears])
    weights_mb = sum(m.weight.numel() for m in linears) * 2 / 1e6
    for N in (8, 64):
        t = torch.randint(0, 1000, (N,), device=dev)

        def torch_lines(i):
            emb = te(unet.timestep_embedding(t, 320).to(dtype))
            return [m(F.silu(emb)) for m in linears]

        def fused(i):
            emb = _hip.time_embed(t, te.linear_1.weight, te.linear_1.bias, te.linear_2.weight, te.linear_2.bias)
            return _hip.time_proj(emb, table)

        def embed_only(i):
            return _hip.time_embed(t, te.linear_1.weight, te.linear_1.bias, te.linear_2.weight, te.linear_2.bias)

        with torch.no_grad():
            rows = {name: graph_us(fn, 1, args.reps, args.iters, dev)
                    for name, fn in (("torch lines", torch_lines), ("p2p_time_embed + p2p_time_proj", fused),
                                     ("p2p_time_embed alone", embed_only))}
        for name, us in rows.items():
            print(f"  N = {N:2d}  {name:32s} {us:8.2f} us")
        proj_us = rows["p2p_time_embed + p2p_time_proj"] - rows["p2p_time_embed alone"]
        print(f"  N = {N:2d}  p2p_time_proj by difference: {proj_us:.2f} us for {weights_mb:.1f} MB of weights = "
              f"{weights_mb / proj_us:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unet_ln_bench needs a GPU")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    libs = {"this tree": _hip.lib()}
    _hip.check_source_hash()
    if args.other_lib:
        other = ctypes.CDLL(args.other_lib)
        other.p2p_layer_norm.argtypes = [ctypes.POINTER(_hip.LayerNormArgs), ctypes.c_void_p]
        other.p2p_source_hash.restype = ctypes.c_char_p
        libs["other"] = other
        print(f"this tree {libs['this tree'].p2p_source_hash().decode()}  other {other.p2p_source_hash().decode()}")
    print(f"{torch.cuda.get_device_name(0)}, {args.dtype}, graphs of {args.reps} calls, median of {args.iters} replays")
    layer_norms(args, dev, dtype, libs)
    time_path(args, dev, dtype)


if __name__ == "__main__":
    main()
