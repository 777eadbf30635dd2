"""Check and time the G1/G7 self-attention kernel, one P2P_SELF_VARIANT per process (the experiments
build reads it once at load; the values that exist are p2p_select.h's Variant: 0 = the default
kernel, 163 = the same with clock stamps, 164 its d = 80 counterpart with G1AB_SHAPE=1024,80; the
library refuses any other).  Checks the kernel against a torch fp32 reference on
the same bf16 inputs (plain, peaky rows, a source-map remap, ragged P/K), then times the config-2
G1 launch (N = 8, H = 8, P = K = 4096, d = 40) with HIP events: median of 7 rounds x 50 launches.
Usage: P2P_EXPERIMENTS_LIB=1 P2P_SELF_VARIANT=v python tools/g1_ab.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from p2p_amd import _hip  # noqa: E402


def ref(q, k, v, H, qk_src=None):
    N, P, C = q.shape
    d = C // H
    qs = q if qk_src is None else q[qk_src]
    ks = k if qk_src is None else k[qk_src]
    qh = qs.float().reshape(N, P, H, d).permute(0, 2, 1, 3)
    kh = ks.float().reshape(N, -1, H, d).permute(0, 2, 1, 3)
    vh = v.float().reshape(N, -1, H, d).permute(0, 2, 1, 3)
    p = (qh @ kh.transpose(-1, -2) * d ** -0.5).softmax(-1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(N, P, C)


def check(N, P, K, d, H=8, qscale=1.0, qk_src=None, dtype=torch.bfloat16, big_head=None):
    g = torch.Generator(device="cuda").manual_seed(P * 7 + K)
    C = H * d
    q = (qscale * torch.randn(N, P, C, device="cuda", generator=g)).to(dtype)
    k = torch.randn(N, K, C, device="cuda", generator=g).to(dtype)
    if big_head is not None:   # one K element past the f16 range: that head's workgroups recompute exactly
        k[:, K // 3, big_head * d] = 1e5
    v = torch.randn(N, K, C, device="cuda", generator=g).to(dtype)
    o = torch.empty_like(q)
    _hip.self_attn(q, k, v, o, H, d ** -0.5, qk_src=qk_src)
    want = ref(q, k, v, H, qk_src)
    return (o.float() - want).abs().max().item() / v.float().abs().max().item()


def time_fn(fn, iters=50, warm=3):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    var = int(os.environ.get("P2P_SELF_VARIANT", "0"))
    P0, d0 = (int(x) for x in os.environ.get("G1AB_SHAPE", "4096,40").split(","))
    errs = {
        "g1": check(8, P0, P0, d0),
        "peaky16": check(2, P0, P0, d0, qscale=16.0),
        "remap": check(8, 1024, 1024, d0, qk_src=[0, 1, 2, 3, 4, 4, 4, 4]),
        "ragged": check(2, 1000, 777, d0),
        "f32in": check(2, 2048, 2048, d0, dtype=torch.float32),
        # an odd number of (entry, head, query tile) items and a ragged last key tile; a workgroup
        # holding items of two heads, one of them on the exact path (chained items: re-staging)
        "odd": check(1, 2560, 2000, d0, H=1),
        "exact_h0": check(1, 2560, 2048, d0, H=2, big_head=0),
        "exact_h1": check(1, 2560, 2048, d0, H=2, big_head=1),
    }
    ok = all(e < 2.0 ** -7 * 2 for e in errs.values())
    P, d = (int(x) for x in os.environ.get("G1AB_SHAPE", "4096,40").split(","))
    N, H = 8, 8
    C = H * d
    q = torch.randn(N, P, C, device="cuda").to(torch.bfloat16)
    k = torch.randn(N, P, C, device="cuda").to(torch.bfloat16)
    v = torch.randn(N, P, C, device="cuda").to(torch.bfloat16)
    o = torch.empty_like(q)
    fn = lambda: _hip.self_attn(q, k, v, o, H, d ** -0.5)  # noqa: E731
    t_end = time.time() + 1.0
    while time.time() < t_end:
        fn()
    torch.cuda.synchronize()
    rounds = [time_fn(fn) for _ in range(7)]
    ms = statistics.median(rounds)
    flop = 4.0 * P * P * C * N
    print(json.dumps({"variant": var, "ok": ok, "rel_err": {k_: round(e, 5) for k_, e in errs.items()},
                      "median_ms": round(ms, 4), "min_ms": round(min(rounds), 4),
                      "tflops": round(flop / ms / 1e9, 1), "frac_2p5": round(flop / ms / 1e9 / 2500, 4)}), flush=True)


if __name__ == "__main__":
    main()
