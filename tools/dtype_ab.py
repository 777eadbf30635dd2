"""bf16 against fp16 inputs, kernel time per launch, in one process (what DESIGN.md's "fp16 inputs"
table is filled from).  The two dtypes alternate (ROUNDS alternations of ITERS launches each, after a
warm-up of both), every launch timed by its own dispatch timestamps (p2p_set_launch_events), so the
host enqueue is not in the numbers.  Per geometry and dtype: the median over the alternations'
medians, and their spread (max - min) -- the noise a difference has to clear.
  self  G1 (P = K = 4096, d 40), G2 (1024, d 80), G3 (256, d 160), G4 (64, d 160), O only
  cross G1, G2, G3 (K = 77): [4 uncond | source + 3 edits] with the north-star Replace program, the
        cond half's maps accumulated into the store
N = 8, H = 8 throughout.  --baseline-lib PATH: also time the bf16 self launches through another
build of the library (same ABI structs; e.g. the parent commit's), interleaved in the same loop.
Usage: python tools/dtype_ab.py [--rounds 7] [--iters 20] [--baseline-lib PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from bench import FenceFreeEvent  # noqa: E402
from p2p_amd import _hip, programs, seq_aligner  # noqa: E402
from p2p_amd import pipeline as pl  # noqa: E402
from p2p_amd.tokenizer import default_tokenizer  # noqa: E402

SELF = [("self G1", 4096, 40), ("self G2", 1024, 80), ("self G3", 256, 160), ("self G4", 64, 160)]
CROSS = [("cross G1", 4096, 40), ("cross G2", 1024, 80), ("cross G3", 256, 160)]
N, H, K_CROSS, B = 8, 8, 77, 4


def timed(lib, fn, iters):
    """Kernel times (us) of `iters` calls of fn, each from its own dispatch timestamps."""
    pairs = []
    for _ in range(iters):
        s, e = FenceFreeEvent(flags=0), FenceFreeEvent(flags=0)
        lib.p2p_set_launch_events(s.ev, e.ev)
        fn()
        lib.p2p_set_launch_events(None, None)
        pairs.append((s, e))
    torch.cuda.synchronize()
    return [s.elapsed_time(e) * 1e3 for s, e in pairs]


def other_lib_self(path):
    """p2p_self_attn_fwd of another build of the library, called on the same argument struct."""
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.p2p_self_attn_fwd.argtypes = [ctypes.POINTER(_hip.AttnTensors), vp, vp, vp, i32, vp, vp]
    L.p2p_self_attn_fwd.restype = ctypes.c_int
    L.p2p_set_launch_events.argtypes = [vp, vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5
    lib = _hip.lib()
    _hip.check_source_hash()
    base = other_lib_self(args.baseline_lib) if args.baseline_lib else None
    tok = default_tokenizer()
    mapper = seq_aligner.get_replacement_mapper(pl.north_star_prompts(), tok)
    prog = programs.replace_program(mapper).to_device("cuda")
    alpha = torch.ones(B - 1, K_CROSS, device="cuda")
    clk = torch.zeros(8, 2, dtype=torch.int64, device="cuda")
    for name, P, d in SELF + CROSS:
        cross = name.startswith("cross")
        K, C = (K_CROSS if cross else P), H * d
        g = torch.Generator(device="cuda").manual_seed(P + d)
        f32 = [torch.randn(N, n, C, device="cuda", generator=g) for n in (P, K, K)]
        runs = {}
        for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            q, k, v = (t.to(dt) for t in f32)
            o = torch.empty_like(q)
            if cross:
                store = torch.zeros(B * H, P, K, device="cuda")
                groups = [(0, B, None, None), (B, B, prog, alpha)]
                slots = [-1] * B + [i * H for i in range(B)]
                runs[tag] = (lib, lambda q=q, k=k, v=v, o=o, store=store: _hip.cross_attn(
                    q, k, v, o, H, d ** -0.5, groups, store=store, store_slot=slots, accumulate=True))
            else:
                runs[tag] = (lib, lambda q=q, k=k, v=v, o=o: _hip.self_attn(q, k, v, o, H, d ** -0.5))
                if base is not None and tag == "bf16":
                    t = _hip.make_tensors(q, k, v, o, H, d ** -0.5, "bf16")
                    st = torch.cuda.current_stream().cuda_stream
                    runs["bf16 baseline lib"] = (base, lambda t=t, keep=(q, k, v, o): base.p2p_self_attn_fwd(
                        ctypes.byref(t), None, None, None, 0, None, st))
        for L, fn in runs.values():          # warm-up: code objects loaded, clocks up
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        meds = {tag: [] for tag in runs}
        for _ in range(args.rounds):
            for tag, (L, fn) in runs.items():
                meds[tag].append(statistics.median(timed(L, fn, args.iters)))
        _hip.clock_probe(clk, 1000)
        torch.cuda.synchronize()
        mhz = statistics.median((clk[:, 0].float() / clk[:, 1].float() * 100.0).tolist())
        row = {"geom": name, "P": P, "K": K, "d": d, "sclk_mhz": round(mhz)}
        for tag, m in meds.items():
            row[tag] = {"median_us": round(statistics.median(m), 2), "spread_us": round(max(m) - min(m), 2)}
        row["fp16_over_bf16"] = round(row["fp16"]["median_us"] / row["bf16"]["median_us"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
