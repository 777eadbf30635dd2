"""The fused DPM-Solver++ latent step (p2p_dpm_step: CFG combine + DPMSolverMultistepScheduler.step +
LocalBlend blend) against the eager scheduler on the same inputs, bit for bit, and the sampler
through the sampling loop, the graphed runner and a GroupBatch -- GPU.

The eager reference is ptp_utils.diffusion_step's unfused tail: the CFG combine in the U-Net's
output dtype, DPMSolverMultistepScheduler.step (checked on the CPU against the mathematics in
tests/test_dpm.py) and LocalBlend's blend of null_text.py:68-70.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

from p2p_amd import _hip, config, controllers, null_text, ptp_utils
from p2p_amd import pipeline as pl
from p2p_amd.dpm import DPMSolverMultistepScheduler

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5


def sched(n, **kw):
    s = DPMSolverMultistepScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", **kw)
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


# the three call forms in three calls: first (n_hist 0, stored), middle (n_hist 1, stored) and last
# (nothing stored: hist_out NULL) -- second-order without lower_order_final, first-order with it
FORMS = {False: [(0, True), (1, True), (1, False)], True: [(0, True), (1, True), (0, False)]}


# ------------------------------------------------------------------ 1. bit-exact against the eager scheduler
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("lof", [False, True], ids=["last2nd", "last1st"])
def test_dpm_step_bit_exact_every_call_form(cuda, dtype, B, with_mask, lof):
    """Each call through the kernel first (the plan changes no state), then through the eager
    scheduler; outputs pre-filled with NaN."""
    g = torch.Generator(device=cuda).manual_seed(B * 100 + with_mask + 2 * lof)
    s = sched(3, lower_order_final=lof)
    x = torch.randn(B, 4, 16, 16, device=cuda, generator=g)
    forms = []
    for c, t in enumerate(s.timesteps.tolist()):
        eps = torch.randn(2 * B, 4, 16, 16, device=cuda, generator=g).to(dtype)
        mask = (torch.rand(B, 16, 16, device=cuda, generator=g) > 0.5).to(torch.uint8) if with_mask else None
        plan = s.plan_step(t)
        forms.append((plan.n_hist, plan.store))
        hist, slot = s.history(plan), s.history_slot(plan, x)
        assert (slot is None) == (c == 2) and len(hist) == plan.n_hist
        if slot is not None:
            slot.fill_(float("nan"))
            assert all(slot.data_ptr() != h.data_ptr() for h in hist)
        out = torch.full_like(x, float("nan"))
        got = _hip.dpm_step(eps, x, out, plan, GUIDANCE, mask, hist=hist, hist_out=slot)
        want = eager_tail(s, eps, x, t, GUIDANCE, mask)
        assert want.dtype == torch.float32 and torch.isfinite(want).all()
        assert torch.equal(got, want), (c, (got - want).abs().max().item())
        if slot is not None:
            assert torch.equal(slot, s.m_prev), c      # hist_out is the eager history entry
        else:
            assert s.m_prev is None
        x = want
    assert forms == FORMS[lof]


def test_dpm_step_ragged_in_place_no_cfg(cuda):
    """[3, 5, 6, 10]: 900 elements (no multiple of a block's 1024 / of 256 threads), no CFG, out
    aliasing x; the same bits, and the guard elements around x and hist_out keep theirs."""
    g = torch.Generator(device=cuda).manual_seed(7)
    shape, n, pad = (3, 5, 6, 10), 900, 64
    for lof in (False, True):
        s = sched(3, lower_order_final=lof)
        x = torch.randn(*shape, device=cuda, generator=g)
        for c, t in enumerate(s.timesteps.tolist()):
            eps = torch.randn(*shape, device=cuda, generator=g)
            plan = s.plan_step(t)
            xbuf = torch.full((n + 2 * pad,), -7.0, device=cuda)
            hbuf = torch.full((n + 2 * pad,), -9.0, device=cuda)
            buf = xbuf[pad:pad + n].view(shape)
            buf.copy_(x)
            slot = hbuf[pad:pad + n].view(shape) if plan.store else None
            eps_before = eps.clone()
            _hip.dpm_step(eps, buf, buf, plan, None, None, hist=s.history(plan), hist_out=slot)   # out aliases x
            want = eager_tail(s, eps, x, t, None, None)
            assert torch.equal(buf, want), c
            assert (xbuf[:pad] == -7.0).all() and (xbuf[pad + n:] == -7.0).all()
            assert (hbuf[:pad] == -9.0).all() and (hbuf[pad + n:] == -9.0).all()
            assert torch.equal(eps, eps_before)
            if plan.store:
                assert torch.equal(slot, s.m_prev)
            else:
                assert (hbuf == -9.0).all()
            x = want


# ------------------------------------------------------------------ 2. the one-launch LocalBlend form
@pytest.mark.parametrize("call", [0, 2], ids=["first_order", "second_order"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("sub", [False, True], ids=["nosub", "substruct"])
@pytest.mark.parametrize("groups", [(True,), (True, False, True)], ids=["one_group", "three_groups"])
def test_dpm_step_builds_folded_blend_mask(cuda, call, dtype, sub, groups):
    """p2p_dpm_step with blend sums (one kernel per step) against the mask p2p_localblend
    (word_sums_ready) builds from the same sums, read by the mask form -- out and hist_out, bit for
    bit."""
    gs, H, L = 4, 8, 5
    G = len(groups)
    B = G * gs
    g = torch.Generator(device=cuda).manual_seed(17 + G + 2 * sub)
    s = sched(20)
    x = drive(s, call, (B, 4, 64, 64), g, cuda)
    eps = torch.randn(2 * B, 4, 64, 64, device=cuda, generator=g).to(dtype)
    t = int(s.timesteps[call])
    plan = s.plan_step(t)
    hist = s.history(plan)
    assert plan.n_hist == (1 if call else 0) and plan.store
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
    h_got, h_want = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    got = _hip.dpm_step(eps, x, torch.full_like(x, float("nan")), plan, GUIDANCE, None, gs if G > 1 else 0, None, blend,
                        hist=hist, hist_out=h_got)
    gb = torch.tensor([1 if on else 0 for on in groups], dtype=torch.uint8, device=cuda)
    want = _hip.dpm_step(eps, x, torch.full_like(x, float("nan")), plan, GUIDANCE, torch.cat(masks), gs if G > 1 else 0,
                         gb if G > 1 else None, hist=hist, hist_out=h_want)
    frac = torch.cat(masks).float().mean().item()
    assert 0.05 < frac < 0.95, frac
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert torch.equal(h_got, h_want) and torch.isfinite(h_got).all()
    # and the mask form is the eager tail (one group: the eager blend broadcasts prompt 0)
    if G == 1:
        assert torch.equal(want, eager_tail(s, eps, x, t, GUIDANCE, masks[0]))
        assert torch.equal(h_want, s.m_prev)
    with pytest.raises(_hip.HipError):      # out may not alias x in the one-launch form
        _hip.dpm_step(eps, x, x, plan, GUIDANCE, None, gs if G > 1 else 0, None, blend, hist=hist, hist_out=h_got)


# ------------------------------------------------------------------ 3. odd shapes
@pytest.mark.parametrize("hw", [(63, 63), (12, 12)], ids=["63x63", "12x12"])
def test_fused_step_odd_shapes_fall_back(cuda, hw):
    """Shapes the one-launch form does not take (H * W % 4, a latent smaller than the maps), through
    diffusion_step: the mask is built by p2p_localblend and read by the mask form, as for PLMS, and
    the result is the eager one (scheduler.step and the blend lines on the same mask)."""
    gs, H, L = 4, 8, 5
    g = torch.Generator(device=cuda).manual_seed(5)
    maps = [torch.zeros(gs * H, 256, 77, device=cuda) for _ in range(L)]
    alpha = torch.ones(gs, 77, device=cuda)
    base = torch.rand(gs * 2, 1, 4, 4, device=cuda, generator=g) ** 3        # a field with structure: a mask
    field = torch.nn.functional.interpolate(base, size=(16, 16), mode="bilinear", align_corners=False)
    sums = field.reshape(gs, 2, 1, 256) * (0.8 + 0.4 * torch.rand(gs, 2, L * H, 256, device=cuda, generator=g))
    sums = sums.contiguous()                                                 # that is neither empty nor full
    sums[:, 1] = 0
    s = sched(20)
    x = drive(s, 2, (gs, 4, *hw), g, cuda)
    eps = torch.randn(2 * gs, 4, *hw, device=cuda, generator=g)
    t = int(s.timesteps[2])
    launches = []

    class Ctrl:
        def fused_step_mask(self):
            return True, lambda size: controllers.FoldedBlendMask(maps, H, alpha, None, 0.5, 0.45, size, sums)

    class Obs:
        def before_aux(self, kind, nbytes):
            launches.append(kind)

    mask = controllers.FoldedBlendMask(maps, H, alpha, None, 0.5, 0.45, hw, sums).materialize()
    assert 0.02 < mask.float().mean().item() < 0.98
    eager = copy.deepcopy(s)
    want = eager_tail(eager, eps, x, t, GUIDANCE, mask)
    model = SimpleNamespace(scheduler=s, unet=lambda lat, tt, encoder_hidden_states=None: {"sample": eps})
    prev = _hip.LAUNCH_OBSERVER
    _hip.LAUNCH_OBSERVER = Obs()
    try:
        got = ptp_utils.diffusion_step(model, Ctrl(), x, None, t, GUIDANCE)
    finally:
        _hip.LAUNCH_OBSERVER = prev
    assert launches[-1] == "dpm_step" and "dpm_blend" not in launches      # the mask form, not the one launch
    assert torch.equal(got, want)
    assert s.counter == 3 and torch.equal(s.m_prev, eager.m_prev)


# ------------------------------------------------------------------ 4-6. the loop and the graphs
STEPS = 6
# LocalBlend reads down_cross[2:4] + up_cross[:3] as 16 x 16 maps, which they are on a 64 x 64
# latent only (on 32 x 32 the first three up maps are 8 x 8): the loop runs the narrow U-Net there
NARROW = dict(block_out_channels=(160, 320, 320, 320), heads=4)
SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128))     # head dims 8 and 16


def make_ctrl(prompts, cuda, fold=True):
    lb = null_text.LocalBlend(list(prompts), pl.BLEND_WORDS, th=(.3, .3), device=cuda)
    lb.start_blend = 2                       # blends from the third call on
    ctrl = null_text.AttentionReplace(list(prompts), STEPS, cross_replace_steps=.8, self_replace_steps=.4,
                                      local_blend=lb, device=cuda)
    ctrl.fold_local_blend = fold
    return ctrl


@pytest.fixture(scope="module")
def loop_runs(cuda):
    """The fused loop, the same loop with the fused latent step disabled (scheduler.step +
    step_callback), and the fused loop with solver_order=1: Replace + LocalBlend on the north-star
    prompts, bf16, reproducible convolutions (as test_gpu_pndm.py sets them)."""
    prompts = pl.north_star_prompts()
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, scheduler="dpm", unet_config=NARROW)
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
        return lat, controllers.reduce_maps(ctrl, 16, ["up", "down"], True, len(prompts)), ctrl

    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        group()                                         # warm-up: library kernel selection
        ptp_utils._fused_latent_step = counting
        fused, maps_f, ctrl_f = group()
        ptp_utils._fused_latent_step = lambda *a, **k: None
        eager, maps_e, ctrl_e = group()
        ptp_utils._fused_latent_step = orig
        good = model.scheduler
        model.scheduler = DPMSolverMultistepScheduler(solver_order=1)
        wrong, _, _ = group()
        model.scheduler = good
    finally:
        ptp_utils._fused_latent_step = orig
        torch.backends.cudnn.enabled = det
    return dict(fused=fused, eager=eager, wrong=wrong, maps_f=maps_f, maps_e=maps_e, ctrl_f=ctrl_f, ctrl_e=ctrl_e,
                fused_calls=fused_calls)


def test_dpm_loop_fused_equals_eager(loop_runs):
    r = loop_runs
    assert r["fused_calls"] == [True] * STEPS                # the kernel really ran, at every call
    assert r["ctrl_f"].cur_step == STEPS and r["ctrl_e"].cur_step == STEPS
    assert r["ctrl_f"].local_blend.counter == STEPS > r["ctrl_f"].local_blend.start_blend
    assert torch.isfinite(r["fused"]).all()
    assert (r["fused"][1:] != r["fused"][:1]).any()          # the edits moved the latents
    assert torch.equal(r["fused"], r["eager"]), (r["fused"] - r["eager"]).abs().max().item()
    assert torch.equal(r["maps_f"], r["maps_e"]) and r["maps_f"].abs().sum().item() > 0


def test_dpm_loop_negative_control(loop_runs):
    """The first-order solver does not reproduce the second-order result."""
    r = loop_runs
    assert torch.isfinite(r["wrong"]).all()
    assert not torch.equal(r["wrong"], r["fused"])
    assert (r["wrong"] - r["fused"]).abs().max().item() > 1e-3


def test_dpm_graphed_runner_bit_identical(cuda):
    """GraphedEditRunner with the DPM-Solver++ scheduler: n graphs; a batch of new seeds and a replay
    of the first seeds are bit-identical to the eager runner (for three groups: run_edit_groups with
    a GroupBatch, which needs nothing of its own for this scheduler)."""
    prompts = pl.north_star_prompts()
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, scheduler="dpm", unet_config=SMALL_UNET)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"):
            eager = pl.edit_batch_runner(model, prompts, lambda: make_ctrl(prompts, cuda), STEPS)
            graphed = pl.edit_batch_runner(model, prompts, lambda: make_ctrl(prompts, cuda), STEPS, graphed=True)
            assert isinstance(graphed, pl.GraphedEditRunner)
            for G in (1, 3):
                first = [100 + g for g in range(G)]
                want0 = graphed(first)                # eager on the capture stream, then the capture
                plan = graphed.plans[G]
                assert len(plan["graphs"]) == STEPS
                assert all(m.cur_step == STEPS for m in plan["members"])
                assert isinstance(plan["ctrl"], controllers.GroupBatch) == (G > 1)
                assert model.scheduler.counter == STEPS and tuple(model.scheduler._ring.shape) == (2, 4 * G, 4, 64, 64)
                seeds = [200 + g for g in range(G)]
                for want, got in ((eager(seeds), graphed(seeds)), (want0, graphed(first))):
                    for w, g_ in zip(want, got):
                        assert w.shape == g_.shape and torch.isfinite(w).all()
                        assert torch.equal(w, g_), (G, (w - g_).abs().max().item())
    finally:
        torch.backends.cudnn.enabled = det


def test_pipeline_scheduler_choice(cuda):
    from p2p_amd.ddim import DDIMScheduler
    m = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, scheduler="dpm", unet_config=SMALL_UNET)
    assert isinstance(m.scheduler, DPMSolverMultistepScheduler)
    assert m.scheduler.solver_order == 2 and m.scheduler.lower_order_final
    ldm_unet = dict(cross_attention_dim=1280, **SMALL_UNET)
    ldm = pl.SyntheticLatentDiffusion(device=cuda, dtype=torch.bfloat16, scheduler="dpm", unet_config=ldm_unet)
    assert isinstance(ldm.scheduler, DPMSolverMultistepScheduler)
    assert isinstance(pl.SyntheticLatentDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=ldm_unet).scheduler,
                      DDIMScheduler)
    with pytest.raises(ValueError, match="'ddim', 'pndm' or 'dpm'"):
        pl.SyntheticLatentDiffusion(device=cuda, scheduler="euler", unet_config=ldm_unet)
    for model in (m, ldm):
        with pytest.raises(TypeError, match="prev_step"):
            null_text.NullInversion(model)
    ddim = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=SMALL_UNET)
    assert null_text.NullInversion(ddim, num_ddim_steps=4).scheduler is ddim.scheduler
