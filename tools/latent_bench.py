"""LocalBlend + latent update launch timing (HIP events, median of repeats), configs[1] shape:
B = 4 prompts, 4 x 64 x 64 latents, bf16 eps, folded word sums [4, 2, 40, 256]:
  fused     : p2p_latent_step with blend sums (latent_blend_kernel: mask + blend + CFG + DDIM)
  two_step  : p2p_localblend mask (blend_finalize_kernel) + p2p_latent_step with the mask
  plain     : p2p_latent_step without a blend
  plms_*    : the same two one-launch / plain forms of p2p_plms_step at a call >= 4 (three stored eps
              read, the new one written)
then, one line per batch ([4, 4, 64, 64] and [32, 4, 64, 64]), p2p_dpm_step against p2p_plms_step in
alternated rounds (plms_vs_dpm).
Usage: python tools/latent_bench.py [iters] [bf16|f16|f32]   (the eps dtype, bf16 by default; run under rocprofv3 --kernel-trace --stats for kernel times)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402

from p2p_amd import _hip, controllers  # noqa: E402
from p2p_amd.ddim import DDIMScheduler  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main(iters=200, dtype=torch.bfloat16):
    dev = "cuda"
    B, H, L = 4, 8, 5
    g = torch.Generator(device=dev).manual_seed(0)
    eps = torch.randn(2 * B, 4, 64, 64, device=dev, generator=g).to(dtype)
    x = torch.randn(B, 4, 64, 64, device=dev, generator=g)
    out = torch.empty_like(x)
    s = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                      set_alpha_to_one=False)
    s.set_timesteps(50)
    coeffs = s.prev_coeffs(500)
    sums = torch.rand(B, 2, L * H, 256, device=dev, generator=g)
    maps = [torch.zeros(B * H, 256, 77, device=dev) for _ in range(L)]
    alpha = torch.ones(B, 77, device=dev)
    fm = controllers.FoldedBlendMask(maps, H, alpha, None, 0.3, 0.3, (64, 64), sums)
    mask = fm.materialize()
    r = {"fused_us": timed(lambda: _hip.latent_step(eps, x, out, coeffs, 7.5, None, 0, None, [fm.latent_entry()]), iters),
         "two_step_us": timed(lambda: _hip.latent_step(eps, x, out, coeffs, 7.5, fm.materialize()), iters),
         "mask_only_us": timed(lambda: fm.materialize(), iters),
         "plain_us": timed(lambda: _hip.latent_step(eps, x, out, coeffs, 7.5, None), iters)}
    from p2p_amd.pndm import PNDMScheduler
    p = PNDMScheduler()
    p.set_timesteps(50)
    for t in p.timesteps.tolist()[:5]:      # the state of call 5: three stored outputs are read
        p.step(torch.randn(B, 4, 64, 64, device=dev, generator=g), t, x)
    plan = p.plan_step(int(p.timesteps[5]))
    hist, slot = p.history(plan), p.history_slot(plan, x)
    r["plms_fused_us"] = timed(lambda: _hip.plms_step(eps, x, out, plan, 7.5, None, 0, None, [fm.latent_entry()],
                                                      hist=hist, hist_out=slot), iters)
    r["plms_plain_us"] = timed(lambda: _hip.plms_step(eps, x, out, plan, 7.5, None, hist=hist, hist_out=slot), iters)
    print(json.dumps({k: round(v, 2) for k, v in r.items()}), flush=True)
    for groups in (1, 8):
        print(json.dumps(plms_vs_dpm(dev, groups, iters, dtype=dtype)), flush=True)


def plms_vs_dpm(dev, groups, iters, rounds=5, dtype=torch.bfloat16):
    """p2p_dpm_step (a second-order call: one stored x0 read, the new one written) against
    p2p_plms_step (call 5: three stored eps read, the new one written) of the same build, on the
    batch of ``groups`` edit groups, plain and one-launch LocalBlend form: ``rounds`` alternated
    rounds of the four, median and range of the per-round means."""
    import statistics
    from p2p_amd.dpm import DPMSolverMultistepScheduler
    from p2p_amd.pndm import PNDMScheduler
    gs, H, L = 4, 8, 5
    B = groups * gs
    g = torch.Generator(device=dev).manual_seed(1)
    eps = torch.randn(2 * B, 4, 64, 64, device=dev, generator=g).to(dtype)
    x = torch.randn(B, 4, 64, 64, device=dev, generator=g)
    out = torch.empty_like(x)
    maps = [torch.zeros(gs * H, 256, 77, device=dev) for _ in range(L)]
    alpha = torch.ones(gs, 77, device=dev)
    blend = [controllers.FoldedBlendMask(maps, H, alpha, None, 0.3, 0.3, (64, 64),
                                         torch.rand(gs, 2, L * H, 256, device=dev, generator=g)).latent_entry()
             for _ in range(groups)]
    group_size = gs if groups > 1 else 0
    p, d = PNDMScheduler(), DPMSolverMultistepScheduler()
    p.set_timesteps(50)
    d.set_timesteps(20)
    for s, calls in ((p, 5), (d, 2)):
        for t in s.timesteps.tolist()[:calls]:
            s.step(torch.randn(B, 4, 64, 64, device=dev, generator=g), t, x)
    pp, dp = p.plan_step(int(p.timesteps[5])), d.plan_step(int(d.timesteps[2]))
    ph, ps, dh, ds = p.history(pp), p.history_slot(pp, x), d.history(dp), d.history_slot(dp, x)
    assert pp.n_hist == 3 and dp.n_hist == 1
    forms = {
        "plms_plain": lambda: _hip.plms_step(eps, x, out, pp, 7.5, None, hist=ph, hist_out=ps),
        "dpm_plain": lambda: _hip.dpm_step(eps, x, out, dp, 7.5, None, hist=dh, hist_out=ds),
        "plms_blend": lambda: _hip.plms_step(eps, x, out, pp, 7.5, None, group_size, None, blend, hist=ph, hist_out=ps),
        "dpm_blend": lambda: _hip.dpm_step(eps, x, out, dp, 7.5, None, group_size, None, blend, hist=dh, hist_out=ds),
    }
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            times[k].append(timed(fn, iters))
    res = {"shape": [B, 4, 64, 64], "rounds": rounds, "iters": iters}
    for k, v in times.items():
        res[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    return res


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200,
         {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[sys.argv[2] if len(sys.argv) > 2 else "bf16"])
