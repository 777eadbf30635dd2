"""The resnets' 3x3 convolutions at the shapes the SD-v1.4 U-Net runs with N = 8: the chain a
ResnetBlock2D ran before conv3x3_kernel (NCHW p2p_group_norm + SiLU, then MIOpen's convolution with
its transposes, zero-fill and cast) against the chain it runs now (token-major p2p_group_norm, then
p2p_conv3x3 and, where K is split, its reduce launch), and each convolution alone.  Every variant
is captured into a HIP graph of --reps calls that rotate over enough operand sets to exceed the
256 MB Infinity Cache, and the graph's replays are timed with events.  Random operands.  Prints one
line per shape: microseconds per call (median of --iters replays), the kernel's TFLOP/s and its
fraction of the 2500 TFLOP/s dense 16-bit peak, and the selection's K split.

Then the six resampling convolutions (Upsample2D, Downsample2D) in the same method: what the module
launched before (F.interpolate + MIOpen's convolution with its bias, or the stride-2 convolution with
its bias, and everything MIOpen adds) against p2p_nchw_to_tokens on the low-resolution map +
p2p_conv3x3_ex in the Up2 / Down2 form with the bias.  --repeat R measures every chain R times: the
spread between the medians of one row is the bar a difference has to clear.  --other-lib runs the
resnet rows' p2p_conv3x3 on another build of the library too (the parent commit's) in the same call.

--loops 1,2,3 times every served row's kernel alone under each value of p2p_conv3x3_set_loop (1 the
register-staged loop, 2 / 3 the global_load_lds ring on 128 / 256 pixels) --repeat times, on the
operands of the row, with microseconds per K step of a workgroup and the fraction of the dense peak;
--other-lib may be given several times, each as PATH or PATH:LOOP (a build with other ring depths,
under that switch value), and is then timed beside them on both kinds of row.  --alone skips the
chains and MIOpen.

    python tools/conv_bench.py [--iters 15] [--reps 32] [--dtype bf16|f16] [--n 8] [--repeat 1]
                               [--other-lib /path/to/libp2p_hip.so[:LOOP]]... [--loops 1,2,3] [--alone]
                               [--only resnet|resample]
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

from p2p_amd import _hip  # noqa: E402

PEAK_TFLOPS = 2500.0
# (H = W, C_in, C_out, how many of the U-Net's resnet convolutions have the shape)
SHAPES = [(64, 320, 320, 7), (64, 640, 320, 2), (64, 960, 320, 1),
          (32, 320, 640, 1), (32, 640, 640, 6), (32, 960, 640, 1), (32, 1280, 640, 1), (32, 1920, 640, 1),
          (16, 640, 1280, 1), (16, 1280, 1280, 6), (16, 1920, 1280, 1), (16, 2560, 1280, 2),
          (8, 1280, 1280, 11), (8, 2560, 1280, 3)]
# (form, input H = W, channels): the U-Net's three Upsample2D and three Downsample2D convolutions
RESAMPLE = [("up2", 8, 1280), ("up2", 16, 1280), ("up2", 32, 640),
            ("down2", 64, 320), ("down2", 32, 640), ("down2", 16, 1280)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--other-lib", action="append", default=[])
    ap.add_argument("--loops", default="")
    ap.add_argument("--alone", action="store_true")
    ap.add_argument("--only", choices=["resnet", "resample"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv_bench needs a GPU")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    _hip.lib()
    _hip.check_source_hash()
    N = args.n
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{torch.cuda.get_device_name(0)}, {args.dtype}, N = {N}, graphs of {args.reps} calls, median of {args.iters} replays")
    print("us per call: [before] NCHW norm + MIOpen conv | MIOpen conv alone || [now] token norm + p2p_conv3x3 | "
          "p2p_conv3x3 alone")
    saved = 0.0
    loops = [int(v) for v in args.loops.split(",") if v]
    others = []   # (label, library)
    for spec in args.other_lib:
        path, _, loop = spec.partition(":")
        lib = ctypes.CDLL(path)
        lib.p2p_conv3x3.argtypes = [ctypes.POINTER(_hip.Conv3x3Args), ctypes.c_void_p]
        lib.p2p_conv3x3_ex.argtypes = [ctypes.POINTER(_hip.Conv3x3ExArgs), ctypes.c_void_p]
        lib.p2p_conv3x3_workspace_floats.restype = ctypes.c_int64
        lib.p2p_conv3x3_workspace_floats.argtypes = [ctypes.c_int32] * 5
        lib.p2p_conv3x3_ex_workspace_floats.restype = ctypes.c_int64
        lib.p2p_conv3x3_ex_workspace_floats.argtypes = [ctypes.c_int32] * 6
        # (one path is one loaded library however often it is named: the value is set before each timing)
        others.append((os.path.basename(os.path.dirname(path)) + (f" loop {loop}" if loop else ""), lib, int(loop or 0)))
    other = others[0][1] if others else None

    def candidates(ours, theirs, gflop, steps):
        """One line per candidate: this build under each --loops value, then every --other-lib."""
        rows = []
        for loop in loops:
            _hip.conv3x3_set_loop(loop)
            try:
                rows.append((f"this build, loop {loop}", [graph_us(ours, *timing) for _ in range(args.repeat)]))
            finally:
                _hip.conv3x3_set_loop(0)
        for label, lib, loop in others:
            if hasattr(lib, "p2p_conv3x3_set_loop"):
                assert lib.p2p_conv3x3_set_loop(loop) == 0
            rows.append((label, [graph_us(lambda i: theirs(i, lib), *timing) for _ in range(args.repeat)]))
        for label, us in rows:
            best = min(us)
            print(f"      {label:28s} " + " ".join(f"{u:7.1f}" for u in us) +
                  f"   {best / steps:5.2f} us per K step ({steps} steps), {gflop / best * 1e3 / PEAK_TFLOPS * 100:4.1f} % of peak",
                  flush=True)
    with torch.no_grad():
        for res, cin, cout, count in ([] if args.only == "resample" else SHAPES):
            split = _hip.conv3x3_split(N, res, res, cin, cout)
            per_set = N * res * res * (2 * cin + cout) * 2 + 2 * 9 * cin * cout * 2
            sets = min(16, max(2, math.ceil(600e6 / per_set)))
            xs = [torch.randn(N, cin, res, res, device=dev, generator=g).to(dtype) for _ in range(sets)]
            ws = [(torch.randn(cout, cin, 3, 3, device=dev, generator=g) / math.sqrt(9 * cin)).to(dtype) for _ in range(sets)]
            gamma, beta = torch.randn(cin, device=dev, generator=g).to(dtype), torch.randn(cin, device=dev, generator=g).to(dtype)
            nchw = [_hip.group_norm(x, gamma, beta, 32, 1e-5, silu=True) for x in xs]
            toks = [_hip.group_norm(x, gamma, beta, 32, 1e-5, silu=True, tokens=True) for x in xs]
            packed = [_hip.conv3x3_pack(w) for w in ws]

            def before(i):
                return F.conv2d(_hip.group_norm(xs[i], gamma, beta, 32, 1e-5, silu=True), ws[i], None, 1, 1)

            def miopen(i):
                return F.conv2d(nchw[i], ws[i], None, 1, 1)

            def now(i):
                return _hip.conv3x3(_hip.group_norm(xs[i], gamma, beta, 32, 1e-5, silu=True, tokens=True), packed[i], res, res)

            def ours(i):
                return _hip.conv3x3(toks[i], packed[i], res, res)

            def theirs(i, other=other):   # p2p_conv3x3 of the other build on the same operands
                a = _hip.Conv3x3Args()
                y = toks[i].new_empty((N, cout, res, res))
                a.x, a.weight, a.y = toks[i].data_ptr(), packed[i].data_ptr(), y.data_ptr()
                n_ws = other.p2p_conv3x3_workspace_floats(N, res, res, cin, cout)
                if n_ws:
                    ws_ = torch.empty(n_ws, dtype=torch.float32, device=dev)
                    a.workspace = ws_.data_ptr()
                a.n, a.height, a.width, a.c_in, a.c_out = N, res, res, cin, cout
                a.dtype = _hip._glue_dtype(toks[i])
                rc = other.p2p_conv3x3(ctypes.byref(a), _hip._stream(dev))
                assert rc == 0, rc
                return y

            timing = (sets, args.reps, args.iters, dev)
            gflop = 2.0 * N * res * res * 9 * cin * cout / 1e9
            if args.alone:
                print(f"  {res:2d}^2 {cin:4d} -> {cout:4d} (x{count:2d}) {gflop:6.1f} GFLOP  split {split}", flush=True)
                if split >= 1:
                    candidates(ours, theirs, gflop, 9 * cin // 64 // split)
                del xs, ws, nchw, toks, packed
                continue
            variants = [before, miopen] + ([now, ours] if split >= 1 else [])
            us = [graph_us(fn, sets, args.reps, args.iters, dev) for fn in variants]
            line = (f"  {res:2d}^2 {cin:4d} -> {cout:4d} (x{count:2d}) {gflop:6.1f} GFLOP  before {us[0]:7.1f} | {us[1]:7.1f} "
                    f"({gflop / us[1] * 1e3:5.0f} TF)")
            if split >= 1:
                tf = gflop / us[3] * 1e3
                line += (f" || now {us[2]:7.1f} | {us[3]:7.1f} ({tf:5.0f} TF, {100 * tf / PEAK_TFLOPS:4.1f} % of peak)  "
                         f"split {split}  chain {us[0] / us[2]:.2f}x")
                saved += count * (us[0] - us[2])
            else:
                line += " || not served by the selection"
            if other is not None and split >= 1 and not loops:
                pairs = [(graph_us(ours, sets, args.reps, args.iters, dev), graph_us(theirs, sets, args.reps, args.iters, dev))
                         for _ in range(max(2, args.repeat))]
                line += ("  alone, this build / other build, repeated: " +
                         ", ".join(f"{a:.1f} / {b:.1f}" for a, b in pairs))
            print(line, flush=True)
            if loops and split >= 1:
                candidates(ours, theirs, gflop, 9 * cin // 64 // split)
            del xs, ws, nchw, toks, packed
    if args.only != "resample" and not args.alone:
        print(f"sum over the served convolutions of a U-Net call: {saved / 1e3:.2f} ms less per call")
    if args.only == "resnet":
        return

    print("the resampling convolutions, us per call: [before] F.interpolate + MIOpen conv + bias (down2: the stride-2 conv + "
          "bias) || [now] p2p_nchw_to_tokens + p2p_conv3x3_ex with the bias | p2p_conv3x3_ex alone")
    gained = 0.0
    with torch.no_grad():
        for form, res, ch in RESAMPLE:
            up = form == "up2"
            code = _hip.CONV_UP2 if up else _hip.CONV_DOWN2
            out = 2 * res if up else res // 2
            split = _hip.conv3x3_ex_split(code, N, res, res, ch, ch)
            per_set = N * (res * res + out * out) * ch * 2 * 2 + 2 * 9 * ch * ch * 2
            sets = min(16, max(2, math.ceil(600e6 / per_set)))
            xs = [torch.randn(N, ch, res, res, device=dev, generator=g).to(dtype) for _ in range(sets)]
            ws = [(torch.randn(ch, ch, 3, 3, device=dev, generator=g) / math.sqrt(9 * ch)).to(dtype) for _ in range(sets)]
            bs = [torch.randn(ch, device=dev, generator=g).to(dtype) for _ in range(sets)]
            toks = [_hip.nchw_to_tokens(x) for x in xs]
            packed = [_hip.conv3x3_pack(w) for w in ws]

            def before(i):
                if up:
                    return F.conv2d(F.interpolate(xs[i], scale_factor=2.0, mode="nearest"), ws[i], bs[i], 1, 1)
                return F.conv2d(xs[i], ws[i], bs[i], 2, 1)

            def now(i):
                return _hip.conv3x3_ex(_hip.conv_input_tokens(xs[i]), packed[i], bs[i], res, res, code)

            def ours(i):
                return _hip.conv3x3_ex(toks[i], packed[i], bs[i], res, res, code)

            def theirs(i, lib):   # p2p_conv3x3_ex of another build on the same operands
                a = _hip.Conv3x3ExArgs()
                y = toks[i].new_empty((N, ch, out, out))
                a.x, a.weight, a.bias, a.y = toks[i].data_ptr(), packed[i].data_ptr(), bs[i].data_ptr(), y.data_ptr()
                n_ws = lib.p2p_conv3x3_ex_workspace_floats(code, N, res, res, ch, ch)
                if n_ws:
                    ws_ = torch.empty(n_ws, dtype=torch.float32, device=dev)
                    a.workspace = ws_.data_ptr()
                a.n, a.in_height, a.in_width, a.c_in, a.c_out = N, res, res, ch, ch
                a.dtype, a.form = _hip._glue_dtype(toks[i]), code
                rc = lib.p2p_conv3x3_ex(ctypes.byref(a), _hip._stream(dev))
                assert rc == 0, rc
                return y

            timing = (sets, args.reps, args.iters, dev)
            gflop = 2.0 * N * out * out * 9 * ch * ch / 1e9
            if args.alone:
                print(f"  {form:5s} {res:2d}^2 -> {out:2d}^2 {ch:4d} -> {ch:4d} {gflop:6.1f} GFLOP  split {split}", flush=True)
                if split >= 1:
                    candidates(ours, theirs, gflop, 9 * ch // 64 // split)
                del xs, ws, bs, toks, packed
                continue
            b_us = [graph_us(before, sets, args.reps, args.iters, dev) for _ in range(args.repeat)]
            line = f"  {form:5s} {res:2d}^2 -> {out:2d}^2 {ch:4d} -> {ch:4d} {gflop:6.1f} GFLOP  before " + \
                " ".join(f"{u:7.1f}" for u in b_us)
            if split >= 1:
                n_us = [graph_us(now, sets, args.reps, args.iters, dev) for _ in range(args.repeat)]
                o_us = graph_us(ours, sets, args.reps, args.iters, dev)
                tf = gflop / o_us * 1e3
                line += (" || now " + " ".join(f"{u:7.1f}" for u in n_us) + f" | {o_us:7.1f} ({tf:5.0f} TF)  split {split}  "
                         f"chain {sorted(b_us)[len(b_us) // 2] / sorted(n_us)[len(n_us) // 2]:.2f}x")
                gained += sorted(b_us)[len(b_us) // 2] - sorted(n_us)[len(n_us) // 2]
            else:
                line += " || not served by the selection"
            print(line, flush=True)
            if loops and split >= 1:
                candidates(ours, theirs, gflop, 9 * ch // 64 // split)
            del xs, ws, bs, toks, packed
    if args.alone:
        return
    print(f"sum over the served resampling convolutions of a U-Net call: {gained / 1e3:.3f} ms less per call")


if __name__ == "__main__":
    main()
