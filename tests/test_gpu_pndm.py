"""The fused PLMS latent step (p2p_plms_step: CFG combine + PNDMScheduler.step + LocalBlend blend)
against the eager scheduler on the same inputs, bit for bit, and the PLMS sampler through the
sampling loop and the graphed runner -- GPU.

The eager reference is ptp_utils.diffusion_step's unfused tail: the CFG combine in the U-Net's
output dtype, PNDMScheduler.step (checked on the CPU against a float64 restatement, the DDIM step
and its order of accuracy in tests/test_pndm.py) and LocalBlend's blend of null_text.py:68-70.
"""
from types import SimpleNamespace

import pytest
import torch

from p2p_amd import _hip, config, controllers, null_text, ptp_utils
from p2p_amd import pipeline as pl
from p2p_amd.pndm import PNDMScheduler

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5


def sched(n=50):
    s = PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", set_alpha_to_one=False,
                      skip_prk_steps=True, steps_offset=1)
    s.set_timesteps(n)
    return s


def eager_tail(s, eps, x, t, guidance, mask):
    """ptp_utils.py:72-75 unfused, with the blend of null_text.py:68-70 on a given mask."""
    if guidance is not None:
        eu, ec = eps.chunk(2)
        noise = eu + guidance * (ec - eu)
    else:
        noise = eps
    out = s.step(noise, t, x)["prev_sample"]
    if mask is not None:
        m = mask[:, None].to(out.dtype)
        out = out[:1] + m * (out - out[:1])
    return out


def drive(s, calls, shape, g, dev):
    """``calls`` eager calls on random model outputs: the scheduler in the state of call ``calls``.
    Returns the sample of that call."""
    x = torch.randn(*shape, device=dev, generator=g)
    for t in s.timesteps.tolist()[:calls]:
        x = s.step(torch.randn(*shape, device=dev, generator=g), t, x)["prev_sample"]
    return x


# ------------------------------------------------------------------ 1. bit-exact against the eager scheduler
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
def test_plms_step_bit_exact_every_call_form(cuda, dtype, B, with_mask):
    """Calls 0 .. 5 of one run (the five forms: first, corrector, 2-, 3- and 4-term), each through
    the kernel first (the plan changes no state) and then through the eager scheduler."""
    g = torch.Generator(device=cuda).manual_seed(B * 100 + with_mask)
    s = sched()
    x = torch.randn(B, 4, 64, 64, device=cuda, generator=g)
    forms = []
    for c, t in enumerate(s.timesteps.tolist()[:6]):
        eps = torch.randn(2 * B, 4, 64, 64, device=cuda, generator=g).to(dtype)
        mask = (torch.rand(B, 64, 64, device=cuda, generator=g) > 0.5).to(torch.uint8) if with_mask else None
        plan = s.plan_step(t)
        forms.append((plan.n_hist, plan.from_kept))
        src, hist = s.step_source(plan, x), s.history(plan)
        slot = s.history_slot(plan, x)
        assert (slot is None) == (c == 1)            # the corrector call stores nothing
        if slot is not None:
            slot.fill_(float("nan"))
        stored_before = [h.clone() for h in s.ets]
        got = _hip.plms_step(eps, src, torch.empty_like(x), plan, GUIDANCE, mask, hist=hist, hist_out=slot)
        want = eager_tail(s, eps, x, t, GUIDANCE, mask)
        assert want.dtype == torch.float32
        assert torch.equal(got, want), (c, (got - want).abs().max().item())
        if c == 1:
            assert len(s.ets) == len(stored_before) and all(torch.equal(a, b) for a, b in zip(s.ets, stored_before))
        else:
            assert torch.equal(slot, s.ets[-1]), c     # hist_out is the eager history entry
        x = want
    assert forms == [(0, False), (1, True), (1, False), (2, False), (3, False), (3, False)]


def test_plms_step_in_place_no_cfg_ragged(cuda):
    g = torch.Generator(device=cuda).manual_seed(7)
    shape = (3, 4, 31, 33)
    s = sched()
    x = torch.randn(*shape, device=cuda, generator=g)
    for c, t in enumerate(s.timesteps.tolist()[:6]):
        eps = torch.randn(*shape, device=cuda, generator=g)
        plan = s.plan_step(t)
        buf = s.step_source(plan, x).clone()
        slot = s.history_slot(plan, x)
        _hip.plms_step(eps, buf, buf, plan, None, None, hist=s.history(plan), hist_out=slot)   # out aliases x
        want = eager_tail(s, eps, x, t, None, None)
        assert torch.equal(buf, want), c
        assert slot is None or torch.equal(slot, s.ets[-1])
        x = want


# ------------------------------------------------------------------ 2. the one-launch LocalBlend form
@pytest.mark.parametrize("call", [5, 1], ids=["call5", "corrector"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("sub", [False, True], ids=["nosub", "substruct"])
@pytest.mark.parametrize("groups", [(True,), (True, False, True)], ids=["one_group", "three_groups"])
def test_plms_step_builds_folded_blend_mask(cuda, call, dtype, sub, groups):
    """p2p_plms_step with blend sums (one kernel per step) against the mask p2p_localblend
    (word_sums_ready) builds from the same sums, read by the mask form -- out and hist_out, bit for
    bit.  On the corrector call the source and the edits are all stepped from the kept sample."""
    gs, H, L = 4, 8, 5
    G = len(groups)
    B = G * gs
    g = torch.Generator(device=cuda).manual_seed(17 + G + 2 * sub)
    s = sched()
    x = drive(s, call, (B, 4, 64, 64), g, cuda)
    eps = torch.randn(2 * B, 4, 64, 64, device=cuda, generator=g).to(dtype)
    plan = s.plan_step(int(s.timesteps[call]))
    src, hist = s.step_source(plan, x), s.history(plan)
    assert plan.n_hist == (3 if call == 5 else 1) and plan.from_kept == (call == 1)
    maps = [torch.zeros(gs * H, 256, 77, device=cuda) for _ in range(L)]   # not read (word sums ready)
    alpha = torch.ones(gs, 77, device=cuda)
    subt = torch.ones(gs, 77, device=cuda) if sub else None
    blend, masks = [], []
    for gi, on in enumerate(groups):
        base = torch.rand(gs * 2, 1, 4, 4, device=cuda, generator=g) ** 3
        field = torch.nn.functional.interpolate(base, size=(16, 16), mode="bilinear", align_corners=False)
        sums = field.reshape(gs, 2, 1, 256) * (0.8 + 0.4 * torch.rand(gs, 2, L * H, 256, device=cuda, generator=g))
        sums = sums.contiguous()
        if not sub:
            sums[:, 1] = 0
        fm = controllers.FoldedBlendMask(maps, H, alpha, subt, 0.5, 0.45, (64, 64), sums)
        blend.append(fm.latent_entry() if on else None)
        masks.append(fm.materialize() if on else torch.zeros(gs, 64, 64, dtype=torch.uint8, device=cuda))
    h_got = torch.full_like(x, float("nan")) if plan.append else None
    h_want = torch.full_like(x, float("nan")) if plan.append else None
    got = _hip.plms_step(eps, src, torch.empty_like(x), plan, GUIDANCE, None, gs if G > 1 else 0, None, blend,
                         hist=hist, hist_out=h_got)
    gb = torch.tensor([1 if on else 0 for on in groups], dtype=torch.uint8, device=cuda)
    want = _hip.plms_step(eps, src, torch.empty_like(x), plan, GUIDANCE, torch.cat(masks), gs if G > 1 else 0,
                          gb if G > 1 else None, hist=hist, hist_out=h_want)
    frac = torch.cat(masks).float().mean().item()
    assert 0.05 < frac < 0.95, frac
    assert torch.equal(got, want), (got - want).abs().max().item()
    if plan.append:
        assert torch.equal(h_got, h_want) and torch.isfinite(h_got).all()
    # and the mask form is the eager tail (one group: the eager blend broadcasts prompt 0)
    if G == 1:
        assert torch.equal(want, eager_tail(s, eps, x, int(s.timesteps[call]), GUIDANCE, masks[0]))
    with pytest.raises(_hip.HipError):      # out may not alias x in the one-launch form
        _hip.plms_step(eps, src, src, plan, GUIDANCE, None, gs if G > 1 else 0, None, blend, hist=hist, hist_out=h_got)


# ------------------------------------------------------------------ 3. odd shapes
@pytest.mark.parametrize("hw", [(63, 63), (12, 12)], ids=["63x63", "12x12"])
def test_fused_step_odd_shapes_fall_back_to_mask_path(cuda, hw):
    gs, H, L = 4, 8, 5
    g = torch.Generator(device=cuda).manual_seed(5)
    maps = [torch.zeros(gs * H, 256, 77, device=cuda) for _ in range(L)]
    alpha = torch.ones(gs, 77, device=cuda)
    sums = (0.5 + torch.rand(gs, 2, L * H, 256, device=cuda, generator=g)).contiguous()
    sums[:, 1] = 0
    s = sched()
    x = drive(s, 5, (gs, 4, *hw), g, cuda)
    eps = torch.randn(2 * gs, 4, *hw, device=cuda, generator=g)
    t = int(s.timesteps[5])

    class Ctrl:
        def fused_step_mask(self):
            return True, lambda size: controllers.FoldedBlendMask(maps, H, alpha, None, 0.3, 0.3, size, sums)

    plan = s.plan_step(t)
    hist = s.history(plan)
    mask = controllers.FoldedBlendMask(maps, H, alpha, None, 0.3, 0.3, hw, sums).materialize()
    h_want = torch.empty_like(x)
    want = _hip.plms_step(eps, x, torch.empty_like(x), plan, GUIDANCE, mask, hist=hist, hist_out=h_want)
    eu, ec = eps.chunk(2)
    got = ptp_utils._fused_latent_step(SimpleNamespace(scheduler=s), Ctrl(), eps, eu, ec, x, t, GUIDANCE)
    assert torch.equal(got, want)
    assert s.counter == 6 and torch.equal(s.ets[-1], h_want)


# ------------------------------------------------------------------ 4-6. the loop and the graphs
STEPS = 6          # 7 U-Net calls: every call form occurs
SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128))     # head dims 8 and 16


def small_model(cuda, scheduler="pndm"):
    return pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, scheduler=scheduler, unet_config=SMALL_UNET)


def make_ctrl(prompts, cuda, fold=True):
    lb = null_text.LocalBlend(list(prompts), pl.BLEND_WORDS, th=(.3, .3), device=cuda)
    lb.start_blend = 2                       # blends from the third call on
    ctrl = null_text.AttentionReplace(list(prompts), STEPS, cross_replace_steps=.8, self_replace_steps=.4,
                                      local_blend=lb, device=cuda)
    ctrl.fold_local_blend = fold
    return ctrl


class StoresCorrectorOutput(PNDMScheduler):
    """Negative control: the corrector call's model output is stored (history [E0, E1]), so the
    later calls combine one output too many, one call early."""

    def plan_step(self, timestep):
        if self.counter < 2:
            return super().plan_step(timestep)
        self.counter += 1
        try:
            return super().plan_step(timestep)
        finally:
            self.counter -= 1

    def commit(self, plan, model_output_f32, sample):
        super().commit(plan._replace(append=True) if plan.from_kept else plan, model_output_f32, sample)


@pytest.fixture(scope="module")
def loop_runs(cuda):
    """The fused loop, the same loop with the fused latent step disabled, and the disabled loop
    with the negative-control scheduler: Replace + LocalBlend on the north-star prompts, bf16,
    reproducible convolutions (as test_cross_kv_cache_bit_identical sets them)."""
    prompts = pl.north_star_prompts()
    model = small_model(cuda)
    x_T = pl.seed_latent(5)
    fused_calls = []
    orig = ptp_utils._fused_latent_step

    def counting(*a, **k):
        out = orig(*a, **k)
        fused_calls.append(out is not None)
        return out

    def group():
        ctrl = make_ctrl(prompts, cuda, fold=False)
        with config.compute_mode("bf16"):
            lat = pl.run_edit_group(model, prompts, ctrl, x_T, num_steps=STEPS)
        return lat, ctrl

    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        group()                                         # warm-up: library kernel selection
        ptp_utils._fused_latent_step = counting
        fused, ctrl_f = group()
        ptp_utils._fused_latent_step = lambda *a, **k: None
        eager, ctrl_e = group()
        good = model.scheduler
        model.scheduler = StoresCorrectorOutput()
        wrong, _ = group()
        model.scheduler = good
    finally:
        ptp_utils._fused_latent_step = orig
        torch.backends.cudnn.enabled = det
    return dict(fused=fused, eager=eager, wrong=wrong, ctrl_f=ctrl_f, ctrl_e=ctrl_e, fused_calls=fused_calls)


def test_plms_loop_fused_equals_eager(loop_runs):
    r = loop_runs
    assert r["fused_calls"] == [True] * (STEPS + 1)          # the kernel really ran, at every call
    assert r["ctrl_f"].cur_step == STEPS + 1 and r["ctrl_e"].cur_step == STEPS + 1
    assert r["ctrl_f"].local_blend.counter == STEPS + 1 > r["ctrl_f"].local_blend.start_blend
    assert torch.isfinite(r["fused"]).all()
    assert (r["fused"][1:] != r["fused"][:1]).any()          # the edits moved the latents
    assert torch.equal(r["fused"], r["eager"]), (r["fused"] - r["eager"]).abs().max().item()


def test_plms_loop_negative_control(loop_runs):
    """A scheduler that stores the corrector's output does not reproduce the fused result."""
    r = loop_runs
    assert torch.isfinite(r["wrong"]).all()
    assert not torch.equal(r["wrong"], r["fused"])
    assert (r["wrong"] - r["fused"]).abs().max().item() > 1e-3


def test_plms_graphed_runner_bit_identical(cuda):
    """GraphedEditRunner with the PNDM scheduler: n + 1 graphs; a batch of new seeds and a replay of
    the first seeds are bit-identical to the eager runner, for one group and a GroupBatch of two."""
    prompts = pl.north_star_prompts()
    model = small_model(cuda)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"):
            eager = pl.edit_batch_runner(model, prompts, lambda: make_ctrl(prompts, cuda), STEPS)
            graphed = pl.edit_batch_runner(model, prompts, lambda: make_ctrl(prompts, cuda), STEPS, graphed=True)
            assert isinstance(graphed, pl.GraphedEditRunner)
            for G in (1, 2):
                first = [100 + g for g in range(G)]
                want0 = graphed(first)                # eager on the capture stream, then the capture
                plan = graphed.plans[G]
                assert len(plan["graphs"]) == STEPS + 1
                assert all(m.cur_step == STEPS + 1 for m in plan["members"])
                seeds = [200 + g for g in range(G)]
                for want, got in ((eager(seeds), graphed(seeds)), (want0, graphed(first))):
                    for w, g_ in zip(want, got):
                        assert w.shape == g_.shape
                        assert torch.equal(w, g_), (G, (w - g_).abs().max().item())
    finally:
        torch.backends.cudnn.enabled = det


def test_pipeline_scheduler_choice(cuda):
    from p2p_amd.ddim import DDIMScheduler
    assert isinstance(small_model(cuda, "ddim").scheduler, DDIMScheduler)
    m = small_model(cuda)
    assert isinstance(m.scheduler, PNDMScheduler) and m.scheduler.steps_offset == 1
    with pytest.raises(ValueError):
        small_model(cuda, "euler")
