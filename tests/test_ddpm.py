"""The edit-friendly DDPM inversion (p2p_amd/ddpm_inversion.py, DDIMScheduler.ddpm_coeffs / ddpm_step,
ptp_utils' latent_noise / first_step) and the argument checks of p2p_ddpm_step / p2p_ddpm_noise -- CPU.

The reference of every test is the restatement of the method written here, in float64 numpy for the
coefficients and in torch lines for the loops:

    sigma_i^2 = eta^2 (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)
    mu_i(x, e) = sqrt(a_prev) ((x - sqrt(1 - a_t) e) / sqrt(a_t)) + sqrt(1 - a_prev - sigma_i^2) e
    level[T] = z0, level[i] = sqrt(a_i) z0 + sqrt(1 - a_i) eps~_i (level[i+1] where sigma_i == 0)
    z_i = (level[i+1] - mu_i(level[i], e_i)) / sigma_i (0 where sigma_i == 0)
    edit: x <- mu_i(x, e) + sigma_i z_i, then step_callback

The U-Net's attention runs on the GPU only, so the model is the elementwise stub of tests/test_direct.py
(eps = tanh(x s(t)) + c(ctx), batch-invariant bit for bit); the same checks on a real tiny U-Net are in
tests/test_gpu_ddpm.py.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_direct import EDIT, SOURCE, MaskBlend, StubUNet, encode, restated_edit, stub_model, z_start

from p2p_amd import _hip, null_text, ptp_utils
from p2p_amd.ddpm_inversion import DDPMInversion

E_ARG, E_DTYPE, E_BATCH, E_ALIGN = -1, -3, -5, -6
GUIDANCE = 7.5
STEPS = 10


# ------------------------------------------------------------------ 1. header, binding, ABI
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    assert re.search(r"^int\s+p2p_ddpm_step\s*\(const p2p_ddpm_step_args\*", text, flags=re.M)
    assert re.search(r"^int\s+p2p_ddpm_noise\s*\(const p2p_ddpm_noise_args\*", text, flags=re.M)
    assert "#define P2P_ABI_VERSION 16" in text
    for name in ("p2p_ddpm_step", "p2p_ddpm_noise"):
        assert name in _hip.EXPORTED_SYMBOLS
        assert getattr(_hip.lib(), name) is not None
    assert _hip.lib().p2p_abi_version() == 16 == _hip.ABI_VERSION


def test_ddpm_step_args_are_the_latent_args_plus_sigma_and_noise():
    assert _hip.DdpmStepArgs._fields_[:-2] == _hip.LatentArgs._fields_
    assert [f[0] for f in _hip.DdpmStepArgs._fields_[-2:]] == ["sigma", "noise"]
    for name, _ in _hip.LatentArgs._fields_:
        assert getattr(_hip.DdpmStepArgs, name).offset == getattr(_hip.LatentArgs, name).offset
    # the C layout: a float right after blend_sub, the pointer on the next 8-byte boundary
    assert _hip.DdpmStepArgs.sigma.offset == _hip.LatentArgs.blend_sub.offset + 4
    assert _hip.DdpmStepArgs.noise.offset == -(-(_hip.DdpmStepArgs.sigma.offset + 4) // 8) * 8
    assert [f[0] for f in _hip.DdpmNoiseArgs._fields_] == ["eps", "eps_dtype", "guidance", "x", "target", "coef",
                                                          "noise", "R", "n"]


# ------------------------------------------------------------------ 2. rejections without a GPU
X, OUT, NZ = 1 << 20, 2 << 20, 3 << 20
ROW = 4 * 64 * 64 * 4            # bytes of one [4, 64, 64] f32 row


def _step(kw):
    a = _hip.DdpmStepArgs()
    a.eps, a.x, a.out, a.noise = 1 << 24, X, OUT, NZ
    a.eps_dtype, a.cfg, a.guidance = 1, 1, 7.5
    a.n_prompts, a.channels, a.height, a.width = 4, 4, 64, 64
    a.sqrt_beta_t, a.sqrt_alpha_t, a.sqrt_alpha_prev, a.sqrt_one_minus_alpha_prev = 0.8, 0.6, 0.65, 0.7
    a.sigma = 0.3
    for k, v in kw.items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


_FOLD = {("blend_sums", 0): 1 << 26, "blend_lh": 40, "blend_res": 16}


@pytest.mark.parametrize("kw,code", [
    (dict(noise=None), E_ARG),
    (dict(noise=X), E_ARG),                                  # noise is x
    (dict(noise=OUT), E_ARG),                                # ... or out
    (dict(noise=X + 4 * ROW - 16), E_ARG),                   # starts in x's last bytes
    (dict(noise=OUT - 16), E_ARG),                           # its one row ends inside out
    (dict(noise=X - 2 * ROW + 16, group_size=2), E_ARG),     # two groups: the second row reaches x
    (dict(noise=X - 16, out=X), E_ARG),                      # out aliasing x is served, a noise in them is not
    (dict(sigma=-1.0), E_ARG), (dict(sigma=float("nan")), E_ARG), (dict(sigma=float("inf")), E_ARG),
    (dict(sigma=-1.0, eps_dtype=7), E_ARG),                  # (the sigma rule comes before the dtype's ...
    (dict(sigma=0.0, eps_dtype=7), E_DTYPE),                 # ... and sigma = 0 passes it: legal, the last step)
    (dict(sigma=0.0, group_size=3), E_ARG),
    (dict(group_size=3), E_ARG),                             # n_prompts no multiple of group_size
    (dict(eps=None), E_ARG), (dict(x=None), E_ARG), (dict(out=None), E_ARG),     # what p2p_latent_step rejects
    (dict(n_prompts=0), E_ARG), (dict(channels=0), E_ARG), (dict(height=0), E_ARG), (dict(width=0), E_ARG),
    (dict(group_size=-1), E_ARG),
    (dict(eps_dtype=7), E_DTYPE),
    # the one-launch LocalBlend form: its own conditions; a misaligned pointer is P2P_E_ARG, as in the
    # other step forms
    ({**_FOLD, "mask": 512}, E_ARG),
    ({**_FOLD, "out": X}, E_ARG),
    ({**_FOLD, "height": 63, "width": 63}, E_ARG),
    ({**_FOLD, "x": X + 4}, E_ARG),
    ({**_FOLD, "noise": NZ + 4}, E_ARG),
    ({**_FOLD, "blend_res": 17}, E_ARG),
    ({("blend_sums", 3): 1 << 26, "blend_lh": 40, "blend_res": 16}, E_ARG),
    (dict(noise=None, eps_dtype=7), E_ARG),                  # two faults: a NULL noise is answered first
])
def test_ddpm_step_rejects(kw, code):
    """Every case returns before any launch (the pointers are not memory: a launch would fault).  That
    sigma = 0 is accepted is shown without a launch: with an unknown eps_dtype as well the answer is the
    dtype's code, where sigma = -1 answers P2P_E_ARG first; the launch itself is in tests/test_gpu_ddpm.py."""
    assert _hip.lib().p2p_ddpm_step(ctypes.byref(_step(kw)), None) == code


def _noise(**kw):
    a = _hip.DdpmNoiseArgs()
    a.eps, a.x, a.target, a.coef, a.noise = 1 << 24, X, OUT, 4096, NZ
    a.eps_dtype, a.guidance, a.R, a.n = 1, 7.5, 4, 4 * 64 * 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(eps=None), E_ARG), (dict(x=None), E_ARG), (dict(target=None), E_ARG), (dict(coef=None), E_ARG),
    (dict(noise=None), E_ARG), (dict(R=0), E_ARG), (dict(R=-1), E_ARG), (dict(n=0), E_ARG),
    (dict(eps_dtype=7), E_DTYPE),
    (dict(R=65536), E_BATCH),
    (dict(n=4 * 64 * 64 + 2), E_ALIGN),
    (dict(eps=(1 << 24) + 8), E_ALIGN), (dict(x=X + 4), E_ALIGN), (dict(target=OUT + 8), E_ALIGN),
    (dict(coef=4100), E_ALIGN), (dict(noise=NZ + 4), E_ALIGN),
])
def test_ddpm_noise_rejects(kw, code):
    assert _hip.lib().p2p_ddpm_noise(ctypes.byref(_noise(**kw)), None) == code


def test_null_args_are_rejected():
    assert _hip.lib().p2p_ddpm_step(None, None) == E_ARG
    assert _hip.lib().p2p_ddpm_noise(None, None) == E_ARG


# ------------------------------------------------------------------ 3. ddpm_coeffs
def restated_coeffs(sched, t, eta):
    """The five factors in float64 from the f32 alphas_cumprod, each rounded once to f32."""
    delta = 1000 // sched.num_inference_steps
    a_t = np.float64(sched.alphas_cumprod[t].item())
    a_prev = np.float64((sched.alphas_cumprod[t - delta] if t - delta >= 0 else sched.final_alpha_cumprod).item())
    var = np.float64(eta) ** 2 * (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
    five = [np.sqrt(1 - a_t), np.sqrt(a_t), np.sqrt(a_prev), np.sqrt(max(1 - a_prev - var, 0.0)), np.sqrt(var)]
    return tuple(float(np.float32(c)) for c in five), float(1 - a_prev - var)


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("T", [4, 10, 50, 100])
def test_ddpm_coeffs(T, eta):
    sched = stub_model().scheduler
    sched.set_timesteps(T)
    ts = [int(t) for t in sched.timesteps]
    least = math.inf
    for i, t in enumerate(ts):
        got = sched.ddpm_coeffs(t, eta)
        want, under_root = restated_coeffs(sched, t, eta)
        assert len(got) == 5 and all(isinstance(c, float) for c in got)
        assert got == want, (t, got, want)
        assert math.isfinite(got[3]) and got[3] >= 0 and under_root > 0
        assert (got[4] == 0.0) == (i == T - 1)              # sigma is 0 at the last step, and only there
        least = min(least, under_root)
    assert ts[-1] == 0 and sched.ddpm_coeffs(0, eta)[4] == 0.0
    # the sigma = 0 step is the deterministic one: its four factors are prev_coeffs' within one f32 ulp
    # (prev_coeffs rounds 1 - a to f32 before the root, ddpm_coeffs takes the root in double)
    for a, b in zip(sched.ddpm_coeffs(0, eta)[:4], sched.prev_coeffs(0)):
        assert abs(a - b) <= float(np.spacing(np.float32(max(a, b))))
    print(f"T = {T}, eta = {eta}: min (1 - a_prev - sigma^2) = {least:.3e}")


def test_ddpm_step_is_the_restated_lines():
    """ddpm_step = mu + sigma z with the product rounded before the sum, f32 and f64; at the last
    step (sigma = 0) the noise does not matter and x comes back (a_prev == a_t there)."""
    sched = stub_model().scheduler
    sched.set_timesteps(STEPS)
    g = torch.Generator().manual_seed(8)
    for dtype in (torch.float32, torch.float64):
        e, x, z = (torch.randn(2, 4, 8, 8, generator=g, dtype=dtype) for _ in range(3))
        (c0, c1, c2, c3, c4), _ = restated_coeffs(sched, 500, 1.0)
        c0, c1, c2, c3, c4 = (torch.tensor(c, dtype=torch.float32) for c in (c0, c1, c2, c3, c4))
        mu = c2 * ((x - c0 * e) / c1) + c3 * e
        assert torch.equal(sched.ddpm_mean(e, 500, x), mu)
        assert torch.equal(sched.ddpm_step(e, 500, x, z), mu + c4 * z)
        assert not torch.equal(sched.ddpm_step(e, 500, x, z), sched.ddpm_step(e, 500, x, z, eta=0.5))
        last = sched.ddpm_step(e, 0, x, z)
        assert torch.equal(last, sched.ddpm_step(e, 0, x, torch.zeros_like(z)))
        assert (last - x).abs().max().item() <= 8 * torch.finfo(dtype).eps * x.abs().max().item()
    assert torch.equal(sched.step(e, 500, x, eta=1.0)["prev_sample"], sched.prev_step(e, 500, x))   # step stays eta = 0


# ------------------------------------------------------------------ the restatement
def restated_levels(sched, z0, noise, eta=1.0):
    T = sched.num_inference_steps
    levels = [None] * T + [z0]
    for i in range(T - 1, -1, -1):
        (c0, c1, _, _, c4), _ = restated_coeffs(sched, int(sched.timesteps[i]), eta)
        levels[i] = levels[i + 1] if c4 == 0 else \
            torch.tensor(c1, dtype=torch.float32) * z0 + torch.tensor(c0, dtype=torch.float32) * noise[i]
    return levels


def restated_mu(sched, e, t, x, eta=1.0):
    c0, c1, c2, c3 = (torch.tensor(c, dtype=torch.float32) for c in restated_coeffs(sched, t, eta)[0][:4])
    return c2 * ((x - c0 * e) / c1) + c3 * e


def restated_inversion(model, z0, prompt, seed, steps=STEPS, g=GUIDANCE, eta=1.0):
    """The levels and the maps [steps, 1, 4, h, w], one U-Net row pair per step."""
    sched, unet = model.scheduler, StubUNet()
    sched.set_timesteps(steps)
    noise = torch.randn((steps, *z0.shape), generator=torch.Generator().manual_seed(seed), dtype=z0.dtype)
    levels = restated_levels(sched, z0, noise, eta)
    ctx = torch.cat([encode(model, [""]), encode(model, [prompt])])
    maps = []
    for i, t in enumerate(int(t) for t in sched.timesteps):
        sigma = restated_coeffs(sched, t, eta)[0][4]
        if sigma == 0:
            maps.append(torch.zeros_like(z0))
            continue
        eps_u, eps_c = unet(torch.cat([levels[i]] * 2), t, ctx)["sample"].chunk(2)
        mu = restated_mu(sched, eps_u + g * (eps_c - eps_u), t, levels[i], eta)
        maps.append((levels[i + 1] - mu) / torch.tensor(sigma, dtype=torch.float32))
    return levels, torch.stack(maps)


def restated_ddpm_edit(model, prompts, x_start, maps, first=0, callback=None, noise_after_blend=False, steps=STEPS,
                       g=GUIDANCE, eta=1.0):
    """x <- mu + sigma z, then the callback (LocalBlend's place).  noise_after_blend: the other order."""
    sched, unet = model.scheduler, StubUNet()
    sched.set_timesteps(steps)
    ctx = torch.cat([encode(model, [""] * len(prompts)), encode(model, prompts)])
    lat = x_start.expand(len(prompts), *x_start.shape[1:])
    callback = callback or (lambda x: x)
    for i, t in enumerate(int(t) for t in sched.timesteps):
        if i < first:
            continue
        eps_u, eps_c = unet(torch.cat([lat] * 2), t, ctx)["sample"].chunk(2)
        mu = restated_mu(sched, eps_u + g * (eps_c - eps_u), t, lat, eta)
        sz = torch.tensor(restated_coeffs(sched, t, eta)[0][4], dtype=torch.float32) * maps[i]
        lat = callback(mu) + sz if noise_after_blend else callback(mu + sz)
    return lat


def library_edit(model, prompts, x_start, maps, first=0, ctrl=None, **kw):
    return ptp_utils.text2image_ldm_stable(model, prompts, ctrl or null_text.EmptyControl(), num_inference_steps=STEPS,
                                           guidance_scale=GUIDANCE, latent=x_start, latent_noise=maps,
                                           first_step=first, **kw)[0]


# ------------------------------------------------------------------ 4. the property
@pytest.mark.parametrize("skip", [0, 3])
def test_source_row_returns_to_the_image_latent(skip):
    """float64, T = 10, g = 7.5: with the extracted maps the source row of a two-prompt edit ends
    within 1e-9 max|z0| of z0 (an identity in exact arithmetic: each step undoes one division and one
    subtraction); with fresh N(0, I) maps, and with zero maps, the same loop misses by more than
    1e-2; the edited row leaves the source row.  With skip = 3 the loop starts from x_start =
    level[3] at first_step = 3."""
    model = stub_model()
    z0 = z_start(shape=(1, 4, 64, 64)).double()
    inv = DDPMInversion(model, STEPS, GUIDANCE, skip=skip)
    (image_gt, image_rec), x_start, maps = inv.invert(z0, SOURCE, generator=torch.Generator().manual_seed(21))
    assert image_gt is z0 and image_rec is None
    assert x_start.shape == (1, 4, 64, 64) and maps.shape == (STEPS, 1, 4, 64, 64) and torch.isfinite(maps).all()
    levels, want = restated_inversion(model, z0, SOURCE, 21)
    assert torch.equal(x_start, levels[skip])
    assert torch.equal(maps[skip:], want[skip:]) and (maps[:skip] == 0).all() and (maps[-1] == 0).all()
    assert maps[skip:-1].abs().max().item() > 0.1            # (maps of a guided step: not rounding dust)
    bar = 1e-9 * z0.abs().max().item()
    prompts = [SOURCE, EDIT]
    g = torch.Generator().manual_seed(22)
    errs = {}
    for name, m in (("maps", maps), ("fresh", torch.randn(maps.shape, generator=g, dtype=maps.dtype)),
                    ("zero", torch.zeros_like(maps))):
        final = library_edit(model, prompts, x_start, m, skip)
        assert final.dtype == torch.float64 and final.shape == (2, 4, 64, 64)
        errs[name] = (final[:1] - z0).abs().max().item()
        if name == "maps":
            assert torch.equal(final, restated_ddpm_edit(model, prompts, x_start, maps, skip))
            assert (final[1] - final[0]).abs().max().item() > 1e-2
    print(f"skip {skip}: bar {bar:.3e}  with the maps {errs['maps']:.3e}  fresh noise {errs['fresh']:.3e}  "
          f"zero maps {errs['zero']:.3e}")
    assert errs["maps"] <= bar
    assert errs["fresh"] > 1e-2 and errs["zero"] > 1e-2


# ------------------------------------------------------------------ 5. chunking
@pytest.mark.parametrize("steps_per_call", [1, 3, 4, 50])
def test_chunks_give_the_same_maps(steps_per_call):
    """10 steps in calls of 1, 3 (tail of 1), 4 (tail of 2) and 50 (one short call): every row carries
    its own timestep and coefficients, so the maps are the restatement's bit for bit."""
    model = stub_model()
    z0 = z_start(1)
    inv = DDPMInversion(model, STEPS, GUIDANCE, steps_per_call=steps_per_call)
    _, x_start, maps = inv.invert(z0, SOURCE, generator=torch.Generator().manual_seed(31))
    levels, want = restated_inversion(model, z0, SOURCE, 31)
    assert maps.dtype == torch.float32 and torch.equal(x_start, levels[0])
    assert torch.equal(maps, want), (maps - want).abs().max().item()
    rows = [x.shape[0] for x, t in model.unet.calls]
    full, tail = divmod(STEPS, steps_per_call)
    assert rows == [2 * steps_per_call] * full + ([2 * tail] if tail else [])
    ts = torch.cat([t.reshape(-1)[:t.numel() // 2] for x, t in model.unet.calls])
    assert ts.tolist() == model.scheduler.timesteps.tolist()
    # a skip leaves the earlier steps out of the U-Net calls, and the later maps as they are
    model = stub_model()
    _, x3, maps3 = DDPMInversion(model, STEPS, GUIDANCE, skip=3, steps_per_call=steps_per_call).invert(
        z0, SOURCE, generator=torch.Generator().manual_seed(31))
    assert torch.equal(x3, levels[3]) and torch.equal(maps3[3:], want[3:]) and (maps3[:3] == 0).all()
    assert sum(x.shape[0] for x, t in model.unet.calls) == 2 * (STEPS - 3)


def test_invert_batch_is_three_inverts():
    """One draw of [T, B, 4, h, w] serves the batch (another stream than three draws of [T, 1, ...]), so
    image b of the batch is compared with the single-image pass on ITS levels: the same maps bit for
    bit.  With one image the batch is ``invert``."""
    prompts = [SOURCE, EDIT, "a photo of a cat riding a bike"]
    model = stub_model()
    zs = [z_start(10 + b) for b in range(3)]
    inv = DDPMInversion(model, STEPS, GUIDANCE, steps_per_call=3)
    batch = inv.invert_batch(torch.cat(zs), prompts, generator=torch.Generator().manual_seed(41))
    listed = inv.invert_batch(zs, prompts, generator=torch.Generator().manual_seed(41))
    noise = torch.randn((STEPS, 3, 4, 8, 8), generator=torch.Generator().manual_seed(41))
    levels = restated_levels(model.scheduler, torch.cat(zs), noise)
    assert len(batch) == 3
    for b in range(3):
        inv.init_prompt(prompts[b])
        maps = inv.noise_maps([lv[b:b + 1] for lv in levels])
        for got in (batch[b], listed[b]):
            assert got[1].shape == (1, 4, 8, 8) and torch.equal(got[1], levels[0][b:b + 1])
            assert got[2].shape == (STEPS, 1, 4, 8, 8) and torch.equal(got[2], maps)
            assert torch.equal(got[0][0], zs[b]) and got[0][1] is None
    assert not torch.equal(batch[0][2], batch[1][2])
    one = inv.invert(zs[0], SOURCE, generator=torch.Generator().manual_seed(42))
    same = inv.invert_batch([zs[0]], [SOURCE], generator=torch.Generator().manual_seed(42))[0]
    assert torch.equal(one[1], same[1]) and torch.equal(one[2], same[2])
    with pytest.raises(ValueError, match="prompts"):
        inv.invert_batch(zs, prompts[:2])
    with pytest.raises(ValueError, match="one size"):
        inv.invert_batch([zs[0], torch.zeros(1, 4, 16, 16)], prompts[:2])


# ------------------------------------------------------------------ 6. order
@pytest.mark.parametrize("low_resource", [False, True])
def test_noise_is_added_before_the_blend(low_resource):
    """A mask-blending controller on 64 x 64 latents: what step_callback is given is ddpm_step's
    output, noise included, and the loop equals step_callback(ddpm_step(...)) -- not the blend followed
    by the noise, which is p2p_direct_step's order.  The tensor form and the per-step list agree."""
    steps, prompts = 4, [SOURCE, EDIT, "a painting of a squirrel eating a lasagna"]
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(1, 4, 64, 64, generator=g)
    maps = torch.randn(steps, 1, 4, 64, 64, generator=g)
    mask = (torch.rand(3, 1, 64, 64, generator=g) > 0.5).float()

    def blend(x):
        return x[:1] + mask * (x - x[:1])

    model = stub_model()
    ctrl = MaskBlend(mask)
    final, _ = ptp_utils.text2image_ldm_stable(model, prompts, ctrl, num_inference_steps=steps, latent=x_T,
                                               low_resource=low_resource, latent_noise=maps)
    assert len(ctrl.seen) == steps
    rows = 3 if low_resource else 6
    starts = [x[:3] for x, t in model.unet.calls if x.shape[0] == rows][::2 if low_resource else 1]
    sched = model.scheduler
    for i, ((given, blended), start) in enumerate(zip(ctrl.seen, starts)):
        t = int(sched.timesteps[i])
        ctx = torch.cat([encode(model, [""] * 3), encode(model, prompts)])
        eps_u, eps_c = StubUNet()(torch.cat([start] * 2), t, ctx)["sample"].chunk(2)
        stepped = sched.ddpm_step(eps_u + GUIDANCE * (eps_c - eps_u), t, start, maps[i].expand(3, -1, -1, -1))
        assert torch.equal(given, stepped), i                   # the callback sees the noised step
        assert torch.equal(blended, blend(given))
    want = restated_ddpm_edit(model, prompts, x_T, maps, callback=blend, steps=steps)
    assert torch.equal(final, want)
    as_list, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps,
                                                 latent=x_T, low_resource=low_resource, latent_noise=list(maps))
    assert torch.equal(as_list, final)
    # The other order, blend then noise (p2p_direct_step's place for its operand).  A group shares its
    # noise, so in exact arithmetic the two orders are one value: x0 + s z + m ((x + s z) - (x0 + s z)) =
    # x0 + m (x - x0) + s z.  They part in rounding wherever x - x0 is inexact, which rows of one x_T, kept
    # close by the stub, seldom are; one step from three independent rows shows it.
    lat = torch.randn(3, 4, 64, 64, generator=g)
    ctx = [encode(model, [""] * 3), encode(model, prompts)]
    ctx = ctx if low_resource else torch.cat(ctx)
    got = ptp_utils.diffusion_step(model, MaskBlend(mask), lat, ctx, 500, GUIDANCE, low_resource,
                                   latent_noise=maps[0])
    eps_u, eps_c = StubUNet()(torch.cat([lat] * 2), 500, torch.cat([encode(model, [""] * 3), encode(model, prompts)])
                              )["sample"].chunk(2)
    e = eps_u + GUIDANCE * (eps_c - eps_u)
    sz = torch.tensor(sched.ddpm_coeffs(500)[4]) * maps[0]
    assert torch.equal(got, blend(sched.ddpm_mean(e, 500, lat) + sz))
    after = blend(sched.ddpm_mean(e, 500, lat)) + sz
    assert not torch.equal(got, after) and torch.equal(got[:1], after[:1])         # (row 0 is never blended)
    assert (got - after).abs().max().item() < 1e-4                                 # ... by rounding alone


def test_noise_rows_go_to_their_groups():
    """[G, 4, h, w] with G = 2 groups of two prompts: every row of group g receives map g."""
    model = stub_model()
    model.scheduler.set_timesteps(4)
    g = torch.Generator().manual_seed(6)
    lat, z = torch.randn(4, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
    ctx = torch.cat([encode(model, [""] * 4), encode(model, [SOURCE, EDIT] * 2)])
    got = ptp_utils.diffusion_step(model, null_text.EmptyControl(), lat, ctx, 500, GUIDANCE, latent_noise=z)
    zero = ptp_utils.diffusion_step(model, null_text.EmptyControl(), lat, ctx, 500, GUIDANCE,
                                    latent_noise=torch.zeros_like(z))
    sigma = torch.tensor(model.scheduler.ddpm_coeffs(500)[4])
    assert torch.equal(got, zero + sigma * z[[0, 0, 1, 1]])
    half = ptp_utils.diffusion_step(model, null_text.EmptyControl(), lat, ctx, 500, GUIDANCE, latent_noise=z, eta=0.5)
    assert not torch.equal(half, got)


# ------------------------------------------------------------------ 7. defaults and refusals
def test_defaults_are_todays_loop():
    steps, prompts = 4, [SOURCE, EDIT]
    g = torch.Generator().manual_seed(4)
    x_T = torch.randn(1, 4, 64, 64, generator=g)
    mask = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float()
    model = stub_model()
    want = restated_edit(model, prompts, x_T, None, callback=lambda x: x[:1] + mask * (x - x[:1]), steps=steps)[-1]
    plain, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps, latent=x_T)
    named, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps, latent=x_T,
                                               latent_noise=None, eta=1.0, first_step=0)
    assert torch.equal(plain, want) and torch.equal(named, want)


@pytest.mark.parametrize("k", [0, 1, 3])
def test_first_step_runs_the_tail(k):
    steps, prompts = 4, [SOURCE, EDIT]
    x = z_start(5, (1, 4, 64, 64))
    model = stub_model()
    ptp_utils.text2image_ldm_stable(model, prompts, null_text.EmptyControl(), num_inference_steps=steps, latent=x,
                                    first_step=k)
    assert len(model.unet.calls) == steps - k
    assert [int(t.reshape(-1)[0]) for _, t in model.unet.calls] == model.scheduler.timesteps.tolist()[k:]
    # latent_noise stays indexed by the absolute step
    maps = torch.randn(steps, 1, 4, 64, 64, generator=torch.Generator().manual_seed(9))
    got, _ = ptp_utils.text2image_ldm_stable(model, prompts, null_text.EmptyControl(), num_inference_steps=steps,
                                             latent=x, latent_noise=maps, first_step=k)
    assert torch.equal(got, restated_ddpm_edit(model, prompts, x, maps, first=k, steps=steps))


def test_refusals():
    model = stub_model()
    model.scheduler.set_timesteps(4)
    lat = torch.zeros(3, 4, 8, 8)
    ctx = torch.cat([encode(model, [""] * 3), encode(model, [SOURCE] * 3)])
    ctrl = null_text.EmptyControl()
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(1, 4, 8, 4), torch.zeros(4, 8, 8)):
        with pytest.raises(ValueError, match="latent_noise"):
            ptp_utils.diffusion_step(model, ctrl, lat, ctx, 750, GUIDANCE, latent_noise=bad)
    ok = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match="latent_offset"):
        ptp_utils.diffusion_step(model, ctrl, lat, ctx, 750, GUIDANCE, latent_noise=ok, latent_offset=ok)
    for eta in (0.0, -1.0):
        with pytest.raises(ValueError, match="eta"):
            ptp_utils.diffusion_step(model, ctrl, lat, ctx, 750, GUIDANCE, latent_noise=ok, eta=eta)
        with pytest.raises(ValueError, match="eta"):
            DDPMInversion(stub_model(), STEPS, GUIDANCE, eta=eta)
    x = z_start(5, (1, 4, 64, 64))
    with pytest.raises(ValueError, match="latent_offsets"):
        ptp_utils.text2image_ldm_stable(model, [SOURCE, EDIT], ctrl, num_inference_steps=4, latent=x,
                                        latent_noise=torch.zeros(4, 1, 4, 64, 64),
                                        latent_offsets=torch.zeros(4, 1, 4, 64, 64))
    for first in (-1, 4):
        with pytest.raises(ValueError, match="first_step"):
            ptp_utils.text2image_ldm_stable(model, [SOURCE, EDIT], ctrl, num_inference_steps=4, latent=x, first_step=first)
    for skip in (-1, STEPS):
        with pytest.raises(ValueError, match="skip"):
            DDPMInversion(stub_model(), STEPS, GUIDANCE, skip=skip)
    with pytest.raises(ValueError, match="steps_per_call"):
        DDPMInversion(stub_model(), STEPS, GUIDANCE, steps_per_call=0)
    assert DDPMInversion(stub_model(), 4, skip=3).scheduler.num_inference_steps == 4


@pytest.mark.parametrize("scheduler", ["dpm", "pndm"])
def test_needs_a_ddim_scheduler(scheduler):
    """Refused as Direct Inversion refuses them (tests/test_direct.py test_needs_a_ddim_scheduler)."""
    with pytest.raises(TypeError, match="prev_step"):
        DDPMInversion(stub_model(scheduler))
    model = stub_model(scheduler)
    model.scheduler.set_timesteps(4)
    lat = torch.zeros(2, 4, 8, 8)
    ctx = torch.cat([encode(model, [""] * 2), encode(model, [SOURCE] * 2)])
    with pytest.raises(TypeError, match="prev_step"):
        ptp_utils.diffusion_step(model, null_text.EmptyControl(), lat, ctx, int(model.scheduler.timesteps[0]), GUIDANCE,
                                 latent_noise=torch.zeros(1, 4, 8, 8))
    assert model.unet.calls == []                                # refused before the U-Net runs
