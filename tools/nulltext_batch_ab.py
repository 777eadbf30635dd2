"""Batched against single-image null-text inversion in one process: after a warm-up of every batch
size, `rounds` alternations of NullInversion.invert (one image) and NullInversion.invert_batch for
each batch size, full-size bf16 U-Net, 64x64 latents, early stop 1e-5.  One JSON line per timed run,
then one summary line per batch size (median inversions/s, its ratio to the same round's single-image
run, the spread of that ratio, Adam updates per image against the batch's maximum).
Usage: python tools/nulltext_batch_ab.py [ddim_steps] [inner_steps] [rounds] [batch sizes, comma-separated]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from p2p_amd import null_text  # noqa: E402
from p2p_amd import pipeline as pl  # noqa: E402


def main(steps=50, inner=10, rounds=3, batches=(1, 2, 4, 8)):
    dev = torch.device("cuda")
    model = pl.SyntheticStableDiffusion(device=dev, dtype=torch.bfloat16)
    x0 = torch.cat([torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(7 + b))
                    for b in range(max(batches))]).to(dev)
    prompts = ([pl.SOURCE] + list(pl.EDITS) * max(batches))[:max(batches)]

    def run(batch, n_steps, n_inner):
        inv = null_text.NullInversion(model, num_ddim_steps=n_steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if batch == 0:
            inv.invert(x0[:1], prompts[0], num_inner_steps=n_inner, early_stop_epsilon=1e-5)
            ran = [inv.inner_steps_run]
        else:
            inv.invert_batch(x0[:batch], prompts[:batch], num_inner_steps=n_inner, early_stop_epsilon=1e-5)
            ran = inv.inner_steps_run_per_image
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ran

    order = (0,) + tuple(batches)          # 0: the single-image invert
    for b in order:
        run(b, 2, 1)
    rate = {b: [] for b in order}
    steps_run = {}
    for r in range(rounds):
        for b in order:
            sec, ran = run(b, steps, inner)
            n = max(b, 1)
            rate[b].append(n / sec)
            steps_run[b] = ran
            print(json.dumps({"round": r, "path": "invert" if b == 0 else "invert_batch", "batch": n,
                              "seconds": round(sec, 3), "inversions_per_s": round(n / sec, 4),
                              "adam_steps_per_image": ran}), flush=True)
    for b in batches:
        ratios = [x / y for x, y in zip(rate[b], rate[0])]
        print(json.dumps({"summary": "invert_batch vs invert", "batch": b,
                          "inversions_per_s_median": round(statistics.median(rate[b]), 4),
                          "single_inversions_per_s_median": round(statistics.median(rate[0]), 4),
                          "ratio_median": round(statistics.median(ratios), 3),
                          "ratio_min": round(min(ratios), 3), "ratio_max": round(max(ratios), 3),
                          "adam_steps_per_image": steps_run[b], "adam_steps_batch_max": max(steps_run[b])}), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(*(int(x) for x in a[:3]), **({"batches": tuple(int(x) for x in a[3].split(","))} if len(a) > 3 else {}))
