"""Direct Inversion against null-text inversion, seconds per image on the synthetic bf16 SD-v1.4-shaped
U-Net, 64x64 latent: DirectInversion.invert (batch 1) or invert_batch (batch B) as a whole and split
into its two passes -- the serial inversion loop and the chunked offsets pass, graph captures
included, as a user's first call pays them -- then NullInversion.invert (invert_batch) at
[steps] x 10 on the same model, and the edit the offsets prepare.  One JSON line per figure.
Usage: python tools/direct_bench.py [steps] [steps_per_call] [B]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from p2p_amd import null_text, ptp_utils  # noqa: E402
from p2p_amd import pipeline as pl  # noqa: E402
from p2p_amd.direct_inversion import DirectInversion  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main(steps=50, steps_per_call=4, batch=1, inner=10):
    dev = torch.device("cuda")
    model = pl.SyntheticStableDiffusion(device=dev, dtype=torch.bfloat16)
    x0 = torch.cat([torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(7 + b)) for b in range(batch)])
    x0 = x0.to(dev)
    prompts = ([pl.SOURCE] + list(pl.EDITS) * batch)[:batch]
    base = {"ddim_steps": steps, "steps_per_call": steps_per_call, "batch": batch, "unet_dtype": "bf16",
            "latent": "64x64"}

    def fresh(n=steps):
        return DirectInversion(model, num_ddim_steps=n, steps_per_call=steps_per_call)

    # warm-up (kernels, allocator, hipBLASLt heuristics) of every batch size the passes run -- a full
    # call and the short tail; the scheduler is shared, so the timed instances are built afterwards
    fresh(min(steps, steps_per_call + steps % steps_per_call)).invert_batch(x0, prompts)
    out, t_all = timed(lambda: fresh().invert_batch(x0, prompts))
    assert len(out) == batch and all(torch.isfinite(o[2]).all() and o[2].shape[0] == steps for o in out)
    print(json.dumps({"config": "direct inversion, invert" + ("_batch" if batch > 1 else ""), **base,
                      "seconds": round(t_all, 3), "seconds_per_image": round(t_all / batch, 4)}), flush=True)
    inv = fresh()
    inv._init_prompts(prompts)
    ptp_utils.register_attention_control(model, None)
    traj, t_loop = timed(lambda: inv.ddim_loop(x0))
    offs, t_off = timed(lambda: inv.latent_offsets(traj))
    calls = -(-steps // steps_per_call)
    print(json.dumps({"config": "direct inversion, the two passes", **base,
                      "inversion_loop_seconds_per_image": round(t_loop / batch, 4),
                      "offsets_pass_seconds_per_image": round(t_off / batch, 4),
                      "unet_replays": f"{steps} of batch {batch} + {calls} of batch up to {2 * steps_per_call * batch}"}),
          flush=True)

    if batch == 1:
        null_text.NullInversion(model, num_ddim_steps=2).invert(x0, prompts[0], num_inner_steps=1)
        nt, t_null = timed(lambda: null_text.NullInversion(model, num_ddim_steps=steps).invert(
            x0, prompts[0], num_inner_steps=inner, early_stop_epsilon=1e-5))
    else:
        null_text.NullInversion(model, num_ddim_steps=2).invert_batch(x0, prompts, num_inner_steps=1)
        nt, t_null = timed(lambda: null_text.NullInversion(model, num_ddim_steps=steps).invert_batch(
            x0, prompts, num_inner_steps=inner, early_stop_epsilon=1e-5))
    print(json.dumps({"config": "null-text inversion, invert" + ("_batch" if batch > 1 else ""), **base,
                      "max_inner_steps": inner, "seconds": round(t_null, 3),
                      "seconds_per_image": round(t_null / batch, 4),
                      "null_text_over_direct": round(t_null / t_all, 2)}), flush=True)

    # the edit the offsets prepare: source + one replacement, AttentionReplace, on image 0
    pair = [prompts[0], pl.EDITS[0] if prompts[0] == pl.SOURCE else pl.SOURCE]
    _, x_T, off0 = out[0]

    def run_edit(n):
        ctrl = null_text.AttentionReplace(pair, n, 0.8, 0.4, device=dev)
        return ptp_utils.text2image_ldm_stable(model, pair, ctrl, num_inference_steps=n, latent=x_T,
                                               latent_offsets=off0[:n])[0]
    run_edit(2)
    lat, t_edit = timed(lambda: run_edit(steps))
    assert torch.isfinite(lat).all()
    print(json.dumps({"config": "P2P edit with the offsets", "prompts": 2, "ddim_steps": steps,
                      "seconds": round(t_edit, 3)}), flush=True)


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:4]))
