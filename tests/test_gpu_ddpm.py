"""The edit-friendly DDPM inversion on the GPU: p2p_ddpm_noise and p2p_ddpm_step bit for bit against
the eager lines, the fused edit loop against scheduler.ddpm_step + step_callback, the fp16 workflow,
the reconstruction property on a real U-Net, and the graphed pass against the eager one.

The reference of every test is the eager restatement, the five factors of DDIMScheduler.ddpm_coeffs as
0-dim f32 tensors (the rounding model of eager_move in tests/test_gpu_direct.py):

    mu    = c2 * ((x - c0 * e) / c1) + c3' * e           e = eps_u + g * (eps_c - eps_u)
    noise = (target - mu) / c4                           (zeros where c4 == 0)
    out   = mu + sigma * noise[group], then the blend x0 + m * (x - x0) towards the group's first row
"""
import pytest
import torch

from test_gpu_blend_geometry import one_launch_inputs
from test_gpu_direct import DTYPE_IDS, DTYPES, GROUPINGS, SMALL_UNET, SOURCE, STEPS, EagerReplace, Kinds, eager_move, \
    make_ctrl, scheduler

from p2p_amd import _hip, config, null_text, ptp_utils
from p2p_amd import pipeline as pl
from p2p_amd.ddpm_inversion import DDPMInversion

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5


# ------------------------------------------------------------------ 1. p2p_ddpm_noise
@pytest.mark.parametrize("g", [1.0, 7.5])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("chw", [(4, 8, 8), (4, 6, 10), (4, 64, 64)], ids=["4x8x8", "4x6x10", "4x64x64"])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_ddpm_noise_bit_exact(cuda, R, chw, dtype, g):
    """Rows at timesteps 980 / 500 / 0 of the 50-step grid in one launch, each with its own five
    factors; t = 0 is the sigma = 0 row, which must come out all zeros (noise pre-filled with NaN).
    Where sigma > 0, mu is also p2p_ddpm_step's without a mask on that row at sigma = 0."""
    s = scheduler()
    gen = torch.Generator().manual_seed(R * 1000 + chw[1] * 10 + int(g))
    eps = torch.randn(2 * R, *chw, generator=gen).to(dtype).to(cuda)
    x = torch.randn(R, *chw, generator=gen).to(cuda)
    target = torch.randn(R, *chw, generator=gen).to(cuda)
    ts = [(500, 0, 980)[r % 3] for r in range(R)]
    coefs = [s.ddpm_coeffs(t) for t in ts]
    assert [c[4] == 0 for c in coefs] == [t == 0 for t in ts]
    coef = torch.tensor(coefs, dtype=torch.float32, device=cuda)
    before = [t.clone() for t in (eps, x, target, coef)]
    got = _hip.ddpm_noise(eps, x, target, coef, g, torch.full_like(x, float("nan")))
    assert torch.isfinite(got).all()
    for r in range(R):
        pair = torch.cat([eps[r:r + 1], eps[R + r:R + r + 1]]).contiguous()
        mu = eager_move(pair, x[r:r + 1], coefs[r][:4], g)
        if coefs[r][4] == 0:
            assert (got[r] == 0).all()
            continue
        want = (target[r:r + 1] - mu) / torch.tensor(coefs[r][4], dtype=torch.float32, device=cuda)
        assert torch.equal(got[r:r + 1], want), (r, (got[r:r + 1] - want).abs().max().item())
        z = torch.randn(1, *chw, generator=gen).to(cuda)
        step0 = _hip.ddpm_step(pair, x[r:r + 1].contiguous(), torch.empty(1, *chw, device=cuda), coefs[r][:4] + (0.0,), z, g)
        assert torch.equal(step0, mu)
    for t, b in zip((eps, x, target, coef), before):
        assert torch.equal(t, b)
    if R > 2:       # the rows' coefficients matter: row 2 (t = 980) with row 0's is another result
        wrong = _hip.ddpm_noise(eps, x, target, coef[:1].expand(R, 5).contiguous(), g, torch.empty_like(x))
        assert not torch.equal(wrong[2], got[2])


def test_ddpm_noise_wrapper_refuses_shapes(cuda):
    x = torch.zeros(2, 4, 8, 8, device=cuda)
    eps = torch.zeros(4, 4, 8, 8, device=cuda)
    coef = torch.ones(2, 5, device=cuda)
    for bad in (dict(eps=eps[:3]), dict(coef=coef[:1]), dict(coef=coef[:, :4].contiguous()), dict(coef=coef.cpu())):
        kw = dict(dict(eps=eps, coef=coef), **bad)
        with pytest.raises(_hip.HipError):
            _hip.ddpm_noise(kw["eps"], x, x.clone(), kw["coef"], 7.5, torch.empty_like(x))


# ------------------------------------------------------------------ 2. p2p_ddpm_step
def step_case(cuda, grouping, dtype, geometry, seed):
    kw = dict(GROUPINGS[grouping])
    explicit = kw.pop("explicit", False)
    eps, x, blend, mask, group_size, gb = one_launch_inputs(cuda, dict(kw, dtype=dtype, **geometry), seed)
    if explicit:
        group_size = kw["gs"]           # one group named by its size instead of 0
    n_groups = len(kw["groups"])
    noise = torch.randn(n_groups, *x.shape[1:], generator=torch.Generator().manual_seed(seed + 1)).to(cuda)
    return eps, x, blend, mask, group_size, gb, noise, kw["gs"], kw["groups"]


def eager_step(eps, x, coeffs, noise, gs, mask=None, groups=None):
    """scheduler.ddpm_step's lines on the whole batch (group g's noise row to its gs prompts), then
    LocalBlend's blend line per blending group."""
    sigma = torch.tensor(coeffs[4], dtype=torch.float32, device=x.device)
    out = eager_move(eps, x, coeffs[:4], GUIDANCE) + sigma * noise.repeat_interleave(gs, 0)
    if mask is not None:
        for gi, on in enumerate(groups):
            if on:
                rows = slice(gi * gs, (gi + 1) * gs)
                out[rows] = out[rows][:1] + mask[rows][:, None].float() * (out[rows] - out[rows][:1])
    return out


def check_ddpm_step(cuda, eps, x, blend, mask, group_size, gb, noise, gs, groups, form):
    coeffs = scheduler().ddpm_coeffs(500)
    assert coeffs[4] > 0.1
    args = {"nomask": (None, group_size, None, None), "mask": (mask, group_size, gb, None),
            "blend": (None, group_size, None, blend)}[form]
    want = eager_step(eps, x, coeffs, noise, gs, None if form == "nomask" else mask, groups)
    x_before = x.clone()
    got = _hip.ddpm_step(eps, x, torch.full_like(x, float("nan")), coeffs, noise, GUIDANCE, *args)
    assert torch.isfinite(got).all() and torch.equal(x, x_before)
    assert torch.equal(got, want), (form, (got - want).abs().max().item())
    # a group's rows all receive that group's noise row: against the noiseless step the unblended form
    # moves every row by (about) sigma * its group's row, and another group's row is another result
    if form == "nomask":
        still = _hip.ddpm_step(eps, x, torch.empty_like(x), coeffs, torch.zeros_like(noise), GUIDANCE, *args)
        moved = got - still
        bound = 4 * torch.finfo(torch.float32).eps * max(got.abs().max().item(), still.abs().max().item())
        assert (moved - coeffs[4] * noise.repeat_interleave(gs, 0)).abs().max().item() <= bound
        if len(groups) > 1:
            assert not torch.equal(got, _hip.ddpm_step(eps, x, torch.empty_like(x), coeffs, noise.flip(0).contiguous(),
                                                       GUIDANCE, *args))
    else:
        assert not torch.equal(got, eager_step(eps, x, coeffs, noise, gs))           # the blend changed something
    # sigma = 0 (the last step of the grid): p2p_latent_step with the same four factors, whatever the noise
    plain = _hip.latent_step(eps, x, torch.empty_like(x), coeffs[:4], GUIDANCE, *args)
    zero = _hip.ddpm_step(eps, x, torch.full_like(x, float("nan")), coeffs[:4] + (0.0,), noise, GUIDANCE, *args)
    assert torch.equal(zero, plain)
    if form != "blend":                                 # out aliasing x, where p2p_latent_step allows it
        buf = x.clone()
        assert _hip.ddpm_step(eps, buf, buf, coeffs, noise, GUIDANCE, *args) is buf
        assert torch.equal(buf, want)
    else:
        with pytest.raises(_hip.HipError):
            _hip.ddpm_step(eps, x, x, coeffs, noise, GUIDANCE, *args)


@pytest.mark.parametrize("form", ["nomask", "mask", "blend"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("grouping", list(GROUPINGS))
def test_ddpm_step_bit_exact(cuda, grouping, dtype, form):
    """4 x 16 x 16 latents with 8 x 8 maps: the eager step, sigma * noise, then the blend."""
    case = step_case(cuda, grouping, dtype, dict(R=8, lat=(16, 16)), 800 + list(GROUPINGS).index(grouping))
    check_ddpm_step(cuda, *case, form)


@pytest.mark.parametrize("form", ["nomask", "mask", "blend"])
def test_ddpm_step_bit_exact_product_geometry(cuda, form):
    """4 x 64 x 64 latents with 16 x 16 maps, three groups of four, bf16."""
    check_ddpm_step(cuda, *step_case(cuda, "12_4", torch.bfloat16, dict(R=16, lat=(64, 64)), 850), form)


def test_ddpm_step_wrapper_refuses_noise_shapes(cuda):
    eps, x, blend, mask, group_size, gb, noise, gs, groups = step_case(cuda, "6_2", torch.float32,
                                                                       dict(R=8, lat=(16, 16)), 860)
    coeffs = scheduler().ddpm_coeffs(500)
    for bad in (noise[:2].contiguous(), noise.double(), noise[:, :, :8], noise.cpu()):
        out = torch.full_like(x, 7.0)
        with pytest.raises(_hip.HipError):
            _hip.ddpm_step(eps, x, out, coeffs, bad, GUIDANCE, mask, group_size, gb)
        assert (out == 7.0).all()
    for sigma in (-1.0, float("nan"), float("inf")):       # the library's own refusal, before any launch
        out = torch.full_like(x, 7.0)
        with pytest.raises(_hip.HipError):
            _hip.ddpm_step(eps, x, out, coeffs[:4] + (sigma,), noise, GUIDANCE, mask, group_size, gb)
        torch.cuda.synchronize()
        assert (out == 7.0).all()


# ------------------------------------------------------------------ 3. the edit loop, fused against eager
def edit(model, cls, x_start, maps, cuda, fold=False, first=0):
    prompts = pl.north_star_prompts()
    ctrl = make_ctrl(cls, prompts, cuda, fold)
    obs, prev = Kinds(), _hip.LAUNCH_OBSERVER
    _hip.LAUNCH_OBSERVER = obs
    try:
        with config.compute_mode("bf16"):
            lat, _ = ptp_utils.text2image_ldm_stable(model, prompts, ctrl, num_inference_steps=STEPS, latent=x_start,
                                                     latent_noise=maps, first_step=first)
    finally:
        _hip.LAUNCH_OBSERVER = prev
    assert ctrl.cur_step == STEPS - first and ctrl.local_blend.counter == STEPS - first
    return lat, [k for k in obs.kinds if k.startswith(("ddpm", "direct", "latent"))]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_edit_loop_fused_equals_eager(cuda, dtype):
    """AttentionReplace + LocalBlend, 10 steps, a tiny U-Net: one p2p_ddpm_step per step against
    scheduler.ddpm_step (host factors, as the kernel's) and step_callback -- the same final latents.
    (fold_local_blend off, as in the other fused-against-eager loops.)  With the fold on, the loop runs
    the one-launch form, whose source row -- which no mask touches -- is the same bits again."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=dtype, unet_config=SMALL_UNET)
    x_T = pl.seed_latent(5)
    maps = torch.randn(STEPS, 1, 4, 64, 64, generator=torch.Generator().manual_seed(6)).to(cuda)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        edit(model, null_text.AttentionReplace, x_T, maps, cuda)          # warm-up: library kernel selection
        fused, kinds_f = edit(model, null_text.AttentionReplace, x_T, maps, cuda)
        eager, kinds_e = edit(model, EagerReplace, x_T, maps, cuda)
        folded, kinds_o = edit(model, null_text.AttentionReplace, x_T, maps, cuda, fold=True)
        still, kinds_z = edit(model, null_text.AttentionReplace, x_T, torch.zeros_like(maps), cuda)
    finally:
        torch.backends.cudnn.enabled = det
    assert kinds_f == ["ddpm_step"] * STEPS and kinds_e == [] and kinds_z == ["ddpm_step"] * STEPS
    assert kinds_o == ["ddpm_step"] * 2 + ["ddpm_blend"] * (STEPS - 2)
    assert torch.isfinite(fused).all() and (fused[1:] != fused[:1]).any()
    assert torch.equal(fused, eager), (fused - eager).abs().max().item()
    assert torch.equal(folded[:1], fused[:1])
    assert (fused[:1] - still[:1]).abs().max().item() > 1e-2               # the maps moved the source row


# ------------------------------------------------------------------ 4. fp16
def test_fp16_inverts_and_edits(cuda):
    """Invert with a float16 U-Net (no backward pass anywhere), then edit with the maps, from skip = 0
    and from skip = 3."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.float16, unet_config=SMALL_UNET)
    z0 = pl.seed_latent(11).to(cuda)
    for skip in (0, 3):
        obs, prev = Kinds(), _hip.LAUNCH_OBSERVER
        _hip.LAUNCH_OBSERVER = obs
        try:
            with config.compute_mode("bf16"):
                inv = DDPMInversion(model, num_ddim_steps=STEPS, skip=skip)
                (gt, rec), x_start, maps = inv.invert(z0, SOURCE, generator=torch.Generator().manual_seed(1))
        finally:
            _hip.LAUNCH_OBSERVER = prev
        assert gt is z0 and rec is None
        assert "ddpm_noise" in obs.kinds
        assert x_start.shape == (1, 4, 64, 64) and x_start.dtype == torch.float32 and torch.isfinite(x_start).all()
        assert maps.shape == (STEPS, 1, 4, 64, 64) and maps.dtype == torch.float32 and maps.is_cuda
        assert torch.isfinite(maps).all() and maps[skip:-1].abs().max().item() > 0
        assert (maps[:skip] == 0).all() and (maps[-1] == 0).all()
        lat, kinds = edit(model, null_text.AttentionReplace, x_start, maps, cuda, first=skip)
        assert kinds == ["ddpm_step"] * (STEPS - skip)
        assert lat.shape == (4, 4, 64, 64) and torch.isfinite(lat).all()


# ------------------------------------------------------------------ 5. the property on a real U-Net
@pytest.mark.parametrize("skip", [0, 3])
def test_source_row_returns_to_the_image_latent(cuda, skip):
    """f32 tiny SD-topology U-Net, 10 steps, g = 7.5: with the extracted maps the source row ends
    nearer to z0 than the same loop with fresh N(0, I) maps and than with zero maps.  No ratio is fixed
    (the GPU U-Net is not batch-invariant bit for bit: the inversion's 8-row calls and the edit's 4-row
    calls round differently); all three errors are printed."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.float32, unet_config=SMALL_UNET)
    z0 = pl.seed_latent(12).to(cuda)
    prompts = [SOURCE, "a painting of a lion eating a burger"]
    with config.compute_mode("bf16"):
        inv = DDPMInversion(model, num_ddim_steps=STEPS, guidance_scale=GUIDANCE, skip=skip)
        _, x_start, maps = inv.invert(z0, SOURCE, generator=torch.Generator().manual_seed(2))
        fresh = torch.randn(maps.shape, generator=torch.Generator().manual_seed(3)).to(cuda)
        runs = {}
        for name, m in (("maps", maps), ("fresh", fresh), ("zero", torch.zeros_like(maps))):
            lat, _ = ptp_utils.text2image_ldm_stable(model, prompts, null_text.EmptyControl(), num_inference_steps=STEPS,
                                                     guidance_scale=GUIDANCE, latent=x_start, latent_noise=m,
                                                     first_step=skip)
            runs[name] = (lat[:1] - z0).abs().max().item()
            if name == "maps":
                assert (lat[1:] - lat[:1]).abs().max().item() > 0
    print(f"skip {skip}: source row, max |final - z0| (max |z0| = {z0.abs().max().item():.3f}): with the maps "
          f"{runs['maps']:.3e}, fresh noise {runs['fresh']:.3e}, zero maps {runs['zero']:.3e}")
    assert runs["maps"] < runs["fresh"] and runs["maps"] < runs["zero"]


# ------------------------------------------------------------------ 6. graphs
def test_graphed_pass_equals_eager(cuda):
    """SD shape, bf16, 4 steps in calls of 3 (a full call and the short tail, two graphs): the graphed
    pass against use_graphs=False, on the same draw."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16)
    z0 = pl.seed_latent(14).to(cuda)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"):
            out = {}
            for graphs in (False, True):
                inv = DDPMInversion(model, num_ddim_steps=4, steps_per_call=3, use_graphs=graphs)
                if not graphs:
                    inv.invert(z0, SOURCE, generator=torch.Generator().manual_seed(4))    # warm-up: kernel selection
                out[graphs] = inv.invert(z0, SOURCE, generator=torch.Generator().manual_seed(4))
    finally:
        torch.backends.cudnn.enabled = det
    (_, x_e, z_e), (_, x_g, z_g) = out[False], out[True]
    assert z_g.shape == (4, 1, 4, 64, 64) and torch.isfinite(z_g).all() and z_g[:3].abs().max().item() > 0
    assert torch.equal(x_g, x_e), (x_g - x_e).abs().max().item()
    assert torch.equal(z_g, z_e), (z_g - z_e).abs().max().item()
