"""Mutual self-attention (p2p_mutual_attn_fwd) against the production self kernel, kernel time per
launch, in one process (what DESIGN.md §4.19 is filled from).

Kernel part.  N = 8 (two CFG halves of 1 source + 3 edits: kv_src = [0, 0, 0, 0, 4, 4, 4, 4]), H = 8,
at (P = 4096, d = 40) and (P = 1024, d = 80), bf16 and fp16 inputs.  Cases, alternated (ROUNDS
alternations of ITERS launches each, after a warm-up of all), every launch timed by its own dispatch
timestamps (p2p_set_launch_events), so the host enqueue is not in the numbers:
  self            p2p_self_attn_fwd on the same tensors (the baseline: the tuned production kernel)
  mutual          p2p_mutual_attn_fwd, all 8 entries, no classes
  mutual fg30/50  the same with token classes: a centred square foreground of 30 % / 50 % of the tokens
  edits / sources the controller's split: the 6 edit entries on p2p_mutual_attn_fwd (fg30 classes),
                  the 2 source entries on p2p_self_attn_fwd (their sum is what a mutual layer costs)
Per case: the median over the alternations' medians and their spread (max - min).

Pipeline part (--groups K, default 3 timed groups per controller after one warm-up group each): a
50-step DDIM group of 1 source + 3 edits on the SD-shaped bf16 U-Net under make_mutual_controller
(unmasked, and mask-guided with ref_words) against the same group under a plain AttentionStore
(store_self_maps = False), runs alternated, wall clock around a synchronised run_edit_group.
Usage: python tools/mutual_bench.py [--rounds 7] [--iters 20] [--groups 3] [--skip-pipeline]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from bench import FenceFreeEvent  # noqa: E402
from p2p_amd import _hip, controllers  # noqa: E402
from p2p_amd import pipeline as pl  # noqa: E402

SHAPES = [("G1", 4096, 40), ("G2", 1024, 80)]
N, H = 8, 8
KV_SRC = [0, 0, 0, 0, 4, 4, 4, 4]
EDIT_SRC = [-1, 0, 0, 0, -1, 4, 4, 4]
PROMPTS = ["a photo of a squirrel sitting on a bench", "a photo of a squirrel jumping over a bench",
           "a photo of a squirrel running on a bench", "a photo of a squirrel standing on a bench"]


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


def centred_square(P, fraction):
    """uint8 [N, P]: class 1 on a centred square holding `fraction` of the side x side tokens."""
    side = int(round(P ** 0.5))
    w = int(round(side * fraction ** 0.5))
    lo = (side - w) // 2
    m = torch.zeros(side, side, dtype=torch.uint8)
    m[lo:lo + w, lo:lo + w] = 1
    return m.reshape(1, P).expand(N, P).contiguous().cuda(), float(m.float().mean())


def kernel_part(args, lib):
    for name, P, d in SHAPES:
        C = H * d
        g = torch.Generator(device="cuda").manual_seed(P + d)
        f32 = [torch.randn(N, P, C, device="cuda", generator=g) for _ in range(3)]
        for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            q, k, v = (t.to(dt) for t in f32)
            o = torch.empty_like(q)
            sc = d ** -0.5
            fg30, f30 = centred_square(P, 0.30)
            fg50, f50 = centred_square(P, 0.50)
            runs = {
                "self": lambda: _hip.self_attn(q, k, v, o, H, sc),
                "mutual": lambda: _hip.mutual_attn(q, k, v, o, H, sc, KV_SRC),
                "mutual fg30": lambda: _hip.mutual_attn(q, k, v, o, H, sc, KV_SRC, token_class=fg30),
                "mutual fg50": lambda: _hip.mutual_attn(q, k, v, o, H, sc, KV_SRC, token_class=fg50),
                "edits fg30": lambda: _hip.mutual_attn(q, k, v, o, H, sc, EDIT_SRC, token_class=fg30),
                "sources": lambda: _hip.self_attn(q[::4], k[::4], v[::4], o[::4], H, sc),
            }
            for fn in runs.values():          # warm-up: code objects loaded, clocks up
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            meds = {case: [] for case in runs}
            for _ in range(args.rounds):
                for case, fn in runs.items():
                    meds[case].append(statistics.median(timed(lib, fn, args.iters)))
            t = _hip.make_tensors(q, k, v, o, H, sc, "bf16")
            row = {"geom": name, "P": P, "d": d, "dtype": tag, "fg30_tokens": round(f30, 3), "fg50_tokens": round(f50, 3),
                   "self_kernel": _hip.self_attn_kernel(t), "mutual_kernel": _hip.mutual_attn_kernel(t, False),
                   "masked_kernel": _hip.mutual_attn_kernel(t, True)}
            for case, m in meds.items():
                row[case] = {"median_us": round(statistics.median(m), 2), "spread_us": round(max(m) - min(m), 2)}
            base = row["self"]["median_us"]
            for case in ("mutual", "mutual fg30", "mutual fg50"):
                row[case + " / self"] = round(row[case]["median_us"] / base, 3)
            row["(edits fg30 + sources) / self"] = round((row["edits fg30"]["median_us"] + row["sources"]["median_us"]) / base, 3)
            print(json.dumps(row), flush=True)


def pipeline_part(args):
    model = pl.SyntheticStableDiffusion(device="cuda", dtype=torch.bfloat16)
    words = ("squirrel",) * len(PROMPTS)

    def plain():
        ctrl = controllers.AttentionStore()
        ctrl.store_self_maps = False
        return ctrl
    makers = {"plain AttentionStore": plain,
              "mutual": lambda: pl.make_mutual_controller(PROMPTS, 50, device="cuda"),
              "mutual ref_words": lambda: pl.make_mutual_controller(PROMPTS, 50, ref_words=words, device="cuda")}

    def group(make, seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = pl.run_edit_group(model, PROMPTS, make(), pl.seed_latent(seed), num_steps=50)
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all()
        return time.perf_counter() - t0
    for make in makers.values():
        group(make, 0)                        # warm-up: library searches, code objects
    secs = {name: [] for name in makers}
    for i in range(args.groups):
        for name, make in makers.items():
            secs[name].append(group(make, 1 + i))
    row = {"pipeline": "50-step DDIM group, 1 source + 3 edits, bf16, eager loop", "timed_groups": args.groups}
    for name, s in secs.items():
        row[name] = {"groups_per_s": round(1.0 / statistics.median(s), 4), "median_s": round(statistics.median(s), 4),
                     "spread_s": round(max(s) - min(s), 4)}
    base = row["plain AttentionStore"]["groups_per_s"]
    for name in ("mutual", "mutual ref_words"):
        row[name + " / plain (groups/s)"] = round(row[name]["groups_per_s"] / base, 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--skip-pipeline", action="store_true")
    args = ap.parse_args()
    lib = _hip.lib()
    _hip.check_source_hash()
    kernel_part(args, lib)
    if not args.skip_pipeline:
        pipeline_part(args)


if __name__ == "__main__":
    main()
