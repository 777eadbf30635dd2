"""The edit-friendly DDPM inversion against Direct Inversion, seconds per image on the synthetic bf16
SD-v1.4-shaped U-Net, 64x64 latent: DDPMInversion.invert (batch 1) or invert_batch (batch B) as a
whole and split into its two halves -- drawing the levels and the chunked noise-map pass, graph
captures included, as a user's first call pays them -- then DirectInversion.invert (invert_batch) on
the same model, and the edit the maps prepare.  One JSON line per figure.
Usage: python tools/ddpm_bench.py [steps] [steps_per_call] [B]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from p2p_amd import null_text, ptp_utils  # noqa: E402
from p2p_amd import pipeline as pl  # noqa: E402
from p2p_amd.ddpm_inversion import DDPMInversion  # noqa: E402
from p2p_amd.direct_inversion import DirectInversion  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main(steps=50, steps_per_call=4, batch=1):
    dev = torch.device("cuda")
    model = pl.SyntheticStableDiffusion(device=dev, dtype=torch.bfloat16)
    x0 = torch.cat([torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(7 + b)) for b in range(batch)])
    x0 = x0.to(dev)
    prompts = ([pl.SOURCE] + list(pl.EDITS) * batch)[:batch]
    base = {"ddim_steps": steps, "steps_per_call": steps_per_call, "batch": batch, "unet_dtype": "bf16",
            "latent": "64x64"}
    short = min(steps, steps_per_call + steps % steps_per_call)

    def seed():
        return torch.Generator().manual_seed(11)

    def fresh(n=steps):
        return DDPMInversion(model, num_ddim_steps=n, steps_per_call=steps_per_call)

    # warm-up (kernels, allocator, hipBLASLt heuristics) of every batch size the pass runs -- a full
    # call and the short tail; the scheduler is shared, so the timed instances are built afterwards
    fresh(short).invert_batch(x0, prompts, generator=seed())
    out, t_all = timed(lambda: fresh().invert_batch(x0, prompts, generator=seed()))
    assert len(out) == batch and all(torch.isfinite(o[2]).all() and o[2].shape[0] == steps for o in out)
    print(json.dumps({"config": "ddpm inversion, invert" + ("_batch" if batch > 1 else ""), **base,
                      "seconds": round(t_all, 3), "seconds_per_image": round(t_all / batch, 4)}), flush=True)
    inv = fresh()
    inv._init_prompts(prompts)
    ptp_utils.register_attention_control(model, None)
    levels, t_lev = timed(lambda: inv.noisy_levels(x0, seed()))
    maps, t_map = timed(lambda: inv.noise_maps(levels))
    calls = -(-steps // steps_per_call)
    print(json.dumps({"config": "ddpm inversion, the two halves", **base,
                      "levels_seconds_per_image": round(t_lev / batch, 4),
                      "noise_map_pass_seconds_per_image": round(t_map / batch, 4),
                      "unet_replays": f"{calls} of batch up to {2 * steps_per_call * batch}"}), flush=True)

    def direct(n=steps):
        return DirectInversion(model, num_ddim_steps=n, steps_per_call=steps_per_call)

    direct(short).invert_batch(x0, prompts)
    dout, t_dir = timed(lambda: direct().invert_batch(x0, prompts))
    assert len(dout) == batch
    print(json.dumps({"config": "direct inversion, invert" + ("_batch" if batch > 1 else ""), **base,
                      "seconds": round(t_dir, 3), "seconds_per_image": round(t_dir / batch, 4),
                      "direct_over_ddpm": round(t_dir / t_all, 2)}), flush=True)

    # the edit the maps prepare: source + one replacement, AttentionReplace, on image 0
    pair = [prompts[0], pl.EDITS[0] if prompts[0] == pl.SOURCE else pl.SOURCE]
    _, x_start, z0 = out[0]

    def run_edit(n):
        ctrl = null_text.AttentionReplace(pair, n, 0.8, 0.4, device=dev)
        return ptp_utils.text2image_ldm_stable(model, pair, ctrl, num_inference_steps=n, latent=x_start,
                                               latent_noise=z0[:n])[0]
    run_edit(2)
    lat, t_edit = timed(lambda: run_edit(steps))
    assert torch.isfinite(lat).all()
    print(json.dumps({"config": "P2P edit with the noise maps", "prompts": 2, "ddim_steps": steps,
                      "seconds": round(t_edit, 3)}), flush=True)


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:4]))
