"""Attention-map figure timing on a 4-prompt SD-shaped store (random running sums in the shapes
AttentionStore keeps: 8 heads; 16^2 cross x 5 layers, 32^2 self x 5 layers).  Prints one JSON line.

* aggregate: controllers.aggregate_attention_device (one p2p_maps_aggregate launch on the selected
  prompt's slabs) against controllers.aggregate_attention (get_average_attention's scaled copy of
  every stored map, then the concatenation, the sum and the copy to the host), at the 16^2 cross
  and the 32^2 self shape.  The device form is timed with its result left on the device and, as
  ``*_to_host``, with the copy that aggregate_attention ends in.
* panels: the 77 panels of show_cross_attention at 16^2 -> 256^2: one p2p_map_panels launch plus the
  copy of the 15 MB of pixels to the host, against the reference's per-token torch + PIL loop on the
  host copy of the aggregate.

Wall-clock times around a device synchronise (the host work is part of what is compared), warmed
up, the forms run in turn within every repeat; a timed window holds --reps calls of one form and
each figure is the median over --iters windows of the time per call.

    python tools/viz_bench.py [--iters 10] [--warmup 2] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prompt-to-prompt_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from p2p_amd import _hip, controllers  # noqa: E402

PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger",
           "a painting of a cat eating a burger", "a painting of a squirrel eating a lasagna"]
HEADS = 8


def sd_store(dev, steps=50):
    g = torch.Generator(device=dev).manual_seed(0)
    n = len(PROMPTS) * HEADS
    s = controllers.AttentionStore()
    s.attention_store = s.get_empty_store()

    def maps(P, K):
        return torch.rand(n, P, K, device=dev, generator=g) * steps

    s.attention_store["down_cross"] = [maps(1024, 77), maps(1024, 77), maps(256, 77), maps(256, 77)]
    s.attention_store["up_cross"] = [maps(256, 77)] * 3 + [maps(1024, 77)] * 3
    s.attention_store["mid_cross"] = [maps(64, 77)]
    s.attention_store["down_self"] = [maps(1024, 1024), maps(1024, 1024), maps(256, 256), maps(256, 256)]
    s.attention_store["up_self"] = [maps(256, 256)] * 3 + [maps(1024, 1024)] * 3
    s.attention_store["mid_self"] = [maps(64, 64)]
    s.cur_step = steps
    return s


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternated(fns, iters, warmup, reps):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ms[k].append(wall_ms(fn, reps))
    return {k: sorted(v)[len(v) // 2] for k, v in ms.items()}


def pil_panels(agg, n, size=256):
    out = []
    for i in range(n):
        image = agg[:, :, i]
        image = 255 * image / image.max()
        image = image.unsqueeze(-1).expand(*image.shape, 3).numpy().astype(np.uint8)
        out.append(np.array(Image.fromarray(image).resize((size, size))))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("viz_bench needs a GPU")
    dev = torch.device("cuda:0")
    _hip.lib()
    _hip.check_source_hash()
    store = sd_store(dev)
    where = ["up", "down"]
    out = {"tool": "viz_bench", "device": torch.cuda.get_device_name(0), "prompts": len(PROMPTS), "heads": HEADS,
           "iters": args.iters, "warmup": args.warmup, "reps": args.reps, "unit": "ms wall per call, median"}
    for name, res, is_cross in (("cross16", 16, True), ("self32", 32, False)):
        fns = {"device": lambda: controllers.aggregate_attention_device(store, res, where, is_cross, 1, PROMPTS),
               "device_to_host": lambda: controllers.aggregate_attention_device(store, res, where, is_cross, 1,
                                                                                PROMPTS).cpu(),
               "torch": lambda: controllers.aggregate_attention(store, res, where, is_cross, 1, PROMPTS)}
        for form, ms in alternated(fns, args.iters, args.warmup, args.reps).items():
            out[f"aggregate_{name}_{form}_ms"] = round(ms, 4)
        a = fns["device"]().cpu()
        b = fns["torch"]()
        out[f"aggregate_{name}_max_rel"] = float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())
    agg_dev = controllers.aggregate_attention_device(store, 16, where, True, 1, PROMPTS)
    agg = agg_dev.cpu()
    fns = {"kernel": lambda: _hip.map_panels(agg_dev, 77, 16, 256, _hip.PANEL_MAX, 1, 77).cpu().numpy(),
           "pil": lambda: pil_panels(agg, 77)}
    for form, ms in alternated(fns, args.iters, args.warmup, args.reps).items():
        out[f"panels77_{form}_ms"] = round(ms, 4)
    out["panels77_equal"] = bool(np.array_equal(fns["kernel"](), fns["pil"]()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
