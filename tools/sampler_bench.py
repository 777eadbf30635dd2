"""Edit-groups/s of the north-star group by sampler: ddim 50, pndm 50, dpm 25 and dpm 20.

The group is bench.py's: 1 source + 3 AttentionReplace edits with LocalBlend, bf16, through
pipeline.sweep_batch_runner(graphed=True) -- one group per call.  One process and one set of
weights; every configuration is warmed (the eager first batch and the capture, then one replay),
then the configurations are timed alternately, ``rounds`` times (host wall time around a
synchronised call).  Prints one JSON line per configuration (median, min, max seconds of a group;
edit-groups/s of the median), then a summary line: the ratio dpm 20 : ddim 50 against the ratio of
U-Net calls (2.5), the straight line seconds = fixed + per_call x calls through dpm 20 and dpm 25
(the per-group cost that does not scale with calls), and the two pieces of that cost which run
outside the graphs, timed on their own (text encoding + context copy, map reduction).

bench.py's headline stays defined on 50 DDIM steps; this tool only compares samplers.
Usage: python tools/sampler_bench.py [rounds]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from p2p_amd import _hip, config, controllers  # noqa: E402
from p2p_amd import pipeline as pl  # noqa: E402

CONFIGS = [("ddim", 50), ("pndm", 50), ("dpm", 25), ("dpm", 20)]


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def main(rounds=5):
    if rounds < 3:
        raise SystemExit("at least three alternated rounds")
    dev = torch.device("cuda", 0)
    config.set_compute("bf16")
    _hip.lib()
    _hip.check_source_hash()
    model = pl.SyntheticStableDiffusion(device=dev, dtype=torch.bfloat16)
    prompts = pl.north_star_prompts()
    runs = []
    for name, steps in CONFIGS:
        sched = pl.make_scheduler(name)
        runner = pl.sweep_batch_runner(model, prompts, steps, device=dev, graphed=True)
        model.scheduler = sched
        t_first, _ = wall(lambda: runner([10 ** 6]), dev)          # the eager batch + the capture
        t_replay, _ = wall(lambda: runner([10 ** 6 + 1]), dev)
        calls = len(sched.timesteps)
        print(json.dumps({"warm": f"{name} {steps}", "unet_calls": calls, "first_s": round(t_first, 3),
                          "replay_s": round(t_replay, 4)}), flush=True)
        runs.append((f"{name} {steps}", sched, runner, calls, []))
    seed = 0
    for _ in range(rounds):
        for _, sched, runner, _, times in runs:
            model.scheduler = sched
            dt, (lat, _) = wall(lambda: runner([seed]), dev)
            if not torch.isfinite(lat).all():
                raise SystemExit("non-finite latents")
            times.append(dt)
            seed += 1
    med = {}
    for label, _, _, calls, times in runs:
        med[label] = statistics.median(times)
        print(json.dumps({"config": label, "unet_calls": calls, "rounds": rounds, "median_s": round(med[label], 4),
                          "min_s": round(min(times), 4), "max_s": round(max(times), 4),
                          "edit_groups_per_s": round(1.0 / med[label], 3),
                          "ms_per_call": round(1e3 * med[label] / calls, 2)}), flush=True)
    # seconds = fixed + per_call * calls through the two DPM configurations
    per_call = (med["dpm 25"] - med["dpm 20"]) / 5
    fixed = med["dpm 20"] - 20 * per_call
    runner = runs[0][2]
    ctx_t = statistics.median(wall(lambda: runner._context(1), dev)[0] for _ in range(11))
    members = runner.plans[1]["members"]
    red_t = statistics.median(
        wall(lambda: controllers.reduce_maps(members[0], 16, ["up", "down"], True, len(prompts)), dev)[0]
        for _ in range(11))
    print(json.dumps({"summary": "dpm 20 : ddim 50", "speedup": round(med["ddim 50"] / med["dpm 20"], 3),
                      "unet_call_ratio": 2.5, "line_per_call_ms": round(1e3 * per_call, 2),
                      "line_fixed_ms": round(1e3 * fixed, 2), "text_encode_context_ms": round(1e3 * ctx_t, 2),
                      "reduce_maps_ms": round(1e3 * red_t, 2)}), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
