"""LocalBlend and the one-launch latent step away from the product geometry (16x16 maps, 5 x 8 maps
per prompt, 77 words, a 4 x 64 x 64 latent) -- GPU.

The mask builder (build_blend_mask: fast and generic path, buffer-load batches of 48 maps, scalar
loads when R*R % 4 != 0), the word-sum kernel, p2p_localblend's x_t blend and the one-launch form of
p2p_latent_step / p2p_plms_step, each at the map resolutions, map counts, latent sizes, channel
counts and group sizes at which its code takes another branch, against tests/blend_ref.py's float64
restatement of null_text.py:41-70 (checked on the CPU in tests/test_blend_ref.py) or, where two
kernel paths must agree, bit for bit against the path the reference has validated.
"""
from types import SimpleNamespace

import pytest
import torch

import blend_ref as br
from p2p_amd import _hip
from p2p_amd.ddim import DDIMScheduler

pytestmark = pytest.mark.gpu

POISON = 0xAB


def mask_only(sums, R, th_pool, th_sub, lat, sub, dev):
    """p2p_localblend with word_sums_ready = 1 and mask_out only, on sums [B, 2, LH, R*R] (host or
    device).  mask_out sits in front of a poisoned tail: every byte of the mask must be written
    with 0 or 1, none of the tail.  Returns the mask as a bool tensor on the host."""
    B, _, LH, R2 = sums.shape
    assert R2 == R * R
    n = B * lat[0] * lat[1]
    buf = torch.full((n + 256,), POISON, dtype=torch.uint8, device=dev)
    mask = buf[:n].view(B, *lat)
    maps = [torch.empty(1, R2, 1, device=dev)]          # not read (word sums ready): the shape alone counts
    alpha = torch.ones(B, 1, device=dev)
    _hip.localblend(maps, LH, alpha, alpha if sub else None, th_pool, th_sub, None, sums.to(dev).contiguous(),
                    mask_out=mask, word_sums_ready=True)
    out = buf.cpu()
    assert bool((out[n:] == POISON).all()), "p2p_localblend wrote behind mask_out"
    assert bool((out[:n] <= 1).all()), "a mask byte is neither 0 nor 1"
    return out[:n].view(B, *lat).bool()


def outside_near(got, want, dist):
    """The pixels where the kernel's mask differs from a reference's and the reference's deciding
    value is not within NEAR of a threshold."""
    return (got != want) & ~(dist < br.NEAR)


# ------------------------------------------------------------------ a. the mask builder against the reference
@pytest.mark.parametrize("R", br.RES)
def test_mask_builder_matches_reference(cuda, R):
    """Every (LH, latent, B, substruct, thresholds) of the grid at one map resolution: each pixel
    where the kernel's mask differs from the float64 reference's lies in the reference's near set
    (a deciding value within 1e-5 of its threshold), with no allowance beyond that."""
    n, paths, largest_near, differing = 0, {False: 0, True: 0}, 0, 0
    for key, sums, lat, (tp, ts) in br.mask_cases(R):
        _, LH, B, sub = key
        got = mask_only(sums, R, tp, ts, lat, sub, cuda)
        want, dist = br.blend_mask_ref(sums, R, tp, ts, lat, sub)
        bad = outside_near(got, want, dist)
        assert not bool(bad.any()), (key, lat, (tp, ts), int(bad.sum()), int((got != want).sum()))
        n += 1
        paths[br.fast_path(R, lat)] += 1
        largest_near = max(largest_near, int((dist < br.NEAR).sum()))
        differing += int((got != want).sum())
    assert paths[True] > 0 and paths[False] > 0, paths          # both paths of build_blend_mask ran
    assert n == 420
    print(f"mask builder R = {R}: {n} (LH, latent, B, sub, th) cases, fast path {paths[True]}, generic path "
          f"{paths[False]}; largest near set {largest_near} pixels; {differing} pixels differ, all inside it")


# ------------------------------------------------------------------ b. degenerate planes
@pytest.mark.parametrize("R", sorted(br.DEGENERATE_LATENTS))
def test_degenerate_planes(cuda, R):
    """An all-zero plane normalises to 0/0 = NaN in torch, which is not > th: an edit prompt whose
    alpha plane is zero takes the source's mask, a zero source plane masks nothing by itself, a
    zero substruct plane gates nothing.  A constant plane masks everything."""
    for name, sums, sub in br.degenerate_cases(R):
        for lat in br.DEGENERATE_LATENTS[R]:
            for tp, ts in br.THRESHOLDS:
                got = mask_only(sums, R, tp, ts, lat, sub, cuda)
                want, dist = br.blend_mask_ref(sums, R, tp, ts, lat, sub)
                bad = outside_near(got, want, dist)
                assert not bool(bad.any()), (name, lat, (tp, ts), int(bad.sum()))
                if name == "edit_alpha_zero":
                    assert torch.equal(got[1], got[0]), (name, lat)
                elif name == "edit_constant":
                    assert bool(got[1].all()), (name, lat)
                elif name == "source_constant":
                    assert bool(got.all()), (name, lat)


# ------------------------------------------------------------------ c. negative controls
@pytest.mark.parametrize("R,lat", br.NEGATIVE_CONTROLS, ids=["R16_64x64", "R10_8x20"])
def test_comparison_rejects_wrong_references(cuda, R, lat):
    """The comparison of (a) can fail: against a reference without the 3x3 max-pool, and one without
    mask[:1] | mask, the kernel's mask leaves the (wrong) reference's near set.  With >= for >, on
    constant planes and the threshold at 1.0, every normalised value is exactly 1.0 at either
    precision -- the decision is an exact comparison, no pixel may differ from the right reference,
    and every pixel differs from the wrong one."""
    sums = br.case_sums((R, 40, 2, False))
    got = mask_only(sums, R, 0.5, 0.45, lat, False, cuda)
    want, dist = br.blend_mask_ref(sums, R, 0.5, 0.45, lat, False)
    assert not bool(outside_near(got, want, dist).any())
    for kw in (dict(pool=False), dict(source_or=False)):
        wrong, wdist = br.blend_mask_ref(sums, R, 0.5, 0.45, lat, False, **kw)
        assert bool(outside_near(got, wrong, wdist).any()), kw
    const = torch.full((2, 2, 40, R * R), 0.7)
    got = mask_only(const, R, 1.0, 1.0, lat, False, cuda)
    right, _ = br.blend_mask_ref(const, R, 1.0, 1.0, lat, False)
    wrong, _ = br.blend_mask_ref(const, R, 1.0, 1.0, lat, False, strict=False)
    assert torch.equal(got, right) and not bool(got.any())
    assert bool((got != wrong).all())


# ------------------------------------------------------------------ d. the word sums
@pytest.mark.parametrize("W", [1, 76, 77, 128])
def test_word_sums_match_float64_einsum(cuda, W):
    """blend_wordsum_kernel (word_sums_ready = 0) against the float64 einsum of the maps with alpha
    and with the substruct weights.  R = 16, 10, 5: four pixel chunks, 64 + 36, one partial chunk;
    W = 76 keeps every map row 16-byte aligned, 77 does not.  Bound: one product rounding and W
    sequential f32 adds per sum, |got - ref| <= 2^-23 * W * sum_w |v_w a_w|."""
    worst, n = 0.0, 0
    for R in (16, 10, 5):
        for heads in (1, 8):
            for n_maps in (1, 5, 8):
                for B in (1, 4):
                    for sub in (False, True):
                        seed = (((W * 17 + R) * 9 + heads) * 9 + n_maps) * 5 + B
                        maps, alpha, subw = br.word_inputs(B, heads, n_maps, R, W, sub, seed)
                        ref, mag = br.word_sums_ref(maps, heads, alpha, subw)
                        numel = ref.numel()
                        buf = torch.full((numel + 64,), float("nan"), device=cuda)
                        ws = buf[:numel]
                        mask = torch.empty(B, 16, 16, dtype=torch.uint8, device=cuda)
                        dmaps = [m.to(cuda) for m in maps]
                        da, ds = alpha.to(cuda), subw.to(cuda) if sub else None
                        _hip.localblend(dmaps, heads, da, ds, 0.3, 0.3, None, ws, mask_out=mask)
                        first = buf.clone()
                        _hip.localblend(dmaps, heads, da, ds, 0.3, 0.3, None, ws, mask_out=mask)
                        assert torch.equal(first[:numel], buf[:numel]), "two launches differ"
                        assert bool(torch.isnan(buf[numel:]).all()), "wrote behind the workspace"
                        got = first[:numel].cpu().double().reshape(ref.shape)
                        assert bool(torch.isfinite(got).all())
                        err, bound = (got - ref).abs(), 2.0 ** -23 * W * mag
                        assert bool((err <= bound).all()), (R, heads, n_maps, B, sub, (err - bound).max().item())
                        if not sub:
                            assert bool((got[:, 1] == 0).all())
                        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
                        n += 1
    print(f"word sums W = {W}: {n} cases, worst |got - ref| / bound = {worst:.4f}")


# ------------------------------------------------------------------ e. p2p_localblend's x_t blend
@pytest.mark.parametrize("channels", [1, 4, 5])
@pytest.mark.parametrize("lat", [(64, 64), (24, 40), (12, 12)], ids=["64x64", "24x40", "12x12"])
def test_localblend_x_t_blend_bit_exact(cuda, channels, lat):
    """x_out is torch's f32 x[:1] + m * (x - x[:1]) bit for bit, with m the same call's mask_out
    (validated against the reference in (a)); x_t[0] keeps its bits; and mask_out is the
    mask-only call's."""
    R, LH, B, sub = key = (16, 40, 16, True)
    sums = br.case_sums(key).to(cuda)
    g = torch.Generator().manual_seed(channels * 100 + lat[0])
    x = torch.randn(B, channels, *lat, generator=g).to(cuda)
    maps = [torch.empty(1, R * R, 1, device=cuda)]
    alpha = torch.ones(B, 1, device=cuda)
    got = x.clone()
    mask = torch.full((B, *lat), POISON, dtype=torch.uint8, device=cuda)
    _hip.localblend(maps, LH, alpha, alpha, 0.5, 0.45, got, sums, mask_out=mask, word_sums_ready=True)
    m = mask[:, None].to(torch.float32)
    want = x[:1] + m * (x - x[:1])
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert torch.equal(got[0].view(torch.int32), x[0].view(torch.int32))
    assert torch.equal(mask.cpu().bool(), mask_only(sums, R, 0.5, 0.45, lat, sub, cuda))
    assert bool((mask <= 1).all()) and 0.02 < mask.float().mean().item() < 0.98


# ------------------------------------------------------------------ f. the one-launch form
def ddim_coeffs():
    s = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                      set_alpha_to_one=False)
    s.set_timesteps(50)
    return s.prev_coeffs(500)


def plms_plan(n_hist):
    """A PLMS plan with n_hist history terms (the scheduler's own plans stop at 3; the entry point
    serves 4): Adams-Bashforth-like weights and the transfer's three scalars."""
    weights = {0: (1.0,), 4: (1901 / 720, -2774 / 720, 2616 / 720, -1274 / 720, 251 / 720)}[n_hist]
    return SimpleNamespace(weights=weights, n_hist=n_hist, sample_coeff=1.0117, eps_num=-0.0213, eps_den=0.8731)


ONE_LAUNCH_BASE = dict(R=16, lat=(64, 64), C=4, LH=40, gs=4, groups=(True,), dtype=torch.float32)
ONE_LAUNCH_CASES = (
    [dict()] +
    [dict(R=15, lat=(15, 16)), dict(R=10, lat=(10, 10)), dict(R=8, lat=(8, 8))] +
    [dict(lat=(16, 16)), dict(lat=(24, 40)), dict(lat=(96, 32))] +         # H*W = 256, 960 (a partial workgroup), 3072
    [dict(C=c) for c in (1, 3, 5, 8)] +
    [dict(LH=lh) for lh in (1, 48, 49)] +
    [dict(gs=gs, groups=groups) for gs in (2, 16) for groups in ((True,), (True, False, True))] +
    [dict(dtype=torch.bfloat16), dict(dtype=torch.float16)]
)


def _case_id(kw):
    return "-".join(f"{k}{str(v).replace('torch.', '').replace(' ', '')}" for k, v in kw.items()) or "base"


def one_launch_inputs(cuda, kw, seed):
    """A case's eps, x, the per-group blend entries of the one-launch form and the (mask, group_size,
    group_blend) of the two-launch path: each blending group's mask from p2p_localblend
    (word_sums_ready) on the same sums."""
    c = dict(ONE_LAUNCH_BASE, **kw)
    R, lat, C, LH, gs, groups = c["R"], c["lat"], c["C"], c["LH"], c["gs"], c["groups"]
    G = len(groups)
    B = G * gs
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(2 * B, C, *lat, generator=g).to(c["dtype"]).to(cuda)
    x = torch.randn(B, C, *lat, generator=g).to(cuda)
    blend, masks = [], []
    for gi, on in enumerate(groups):
        sums = br.smooth_sums(gs, LH, R, True, seed * 10 + gi).to(cuda)
        if on:
            blend.append((sums, 0.5, 0.45, True))
            masks.append(mask_only(sums, R, 0.5, 0.45, lat, True, cuda).to(torch.uint8).to(cuda))
        else:
            blend.append(None)
            masks.append(torch.zeros(gs, *lat, dtype=torch.uint8, device=cuda))
    mask = torch.cat(masks)
    on_frac = torch.cat([m for m, on in zip(masks, groups) if on]).float().mean().item()
    assert 0.02 < on_frac < 0.98, on_frac
    group_size = gs if G > 1 else 0
    gb = torch.tensor([int(on) for on in groups], dtype=torch.uint8, device=cuda) if G > 1 else None
    return eps, x, blend, mask, group_size, gb


@pytest.mark.parametrize("kw", ONE_LAUNCH_CASES, ids=_case_id)
def test_one_launch_latent_step_matches_two_launch(cuda, kw):
    """p2p_latent_step with blend sums, one axis at a time away from the product geometry, bit for
    bit against the mask-reading step on p2p_localblend's mask (whose mask (a) has validated)."""
    eps, x, blend, mask, group_size, gb = one_launch_inputs(cuda, kw, 300 + ONE_LAUNCH_CASES.index(kw))
    coeffs = ddim_coeffs()
    got = _hip.latent_step(eps, x, torch.full_like(x, float("nan")), coeffs, 7.5, None, group_size, None, blend)
    want = _hip.latent_step(eps, x, torch.empty_like(x), coeffs, 7.5, mask, group_size, gb)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want), (got - want).abs().max().item()
    plain = _hip.latent_step(eps, x, torch.empty_like(x), coeffs, 7.5, None)
    assert not torch.equal(got, plain)                    # the blend changed something


@pytest.mark.parametrize("n_hist", [0, 4])
@pytest.mark.parametrize("kw", [dict(), dict(R=10, lat=(10, 10)), dict(lat=(24, 40)), dict(C=5), dict(LH=49),
                                dict(gs=2, groups=(True, False, True)), dict(dtype=torch.bfloat16)], ids=_case_id)
def test_one_launch_plms_step_matches_two_launch(cuda, kw, n_hist):
    """The same for p2p_plms_step with no and with four history terms: out and hist_out bit for bit."""
    eps, x, blend, mask, group_size, gb = one_launch_inputs(cuda, kw, 500 + n_hist)
    g = torch.Generator().manual_seed(n_hist)
    hist = [torch.randn(*x.shape, generator=g).to(cuda) for _ in range(n_hist)]
    plan = plms_plan(n_hist)
    h_got, h_want = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    got = _hip.plms_step(eps, x, torch.full_like(x, float("nan")), plan, 7.5, None, group_size, None, blend,
                         hist=hist, hist_out=h_got)
    want = _hip.plms_step(eps, x, torch.empty_like(x), plan, 7.5, mask, group_size, gb, hist=hist, hist_out=h_want)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(h_got).all())
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert torch.equal(h_got, h_want)


def _misaligned(t):
    """A contiguous copy of t that starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    off = 4 // t.element_size()
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("step", ["ddim", "plms"])
def test_one_launch_form_rejects_before_any_launch(cuda, step):
    """What the one-launch form does not serve raises HipError and leaves ``out`` untouched."""
    def call(eps, x, out, mask, blend):
        if step == "ddim":
            return _hip.latent_step(eps, x, out, ddim_coeffs(), 7.5, mask, 0, None, blend)
        return _hip.plms_step(eps, x, out, plms_plan(0), 7.5, mask, 0, None, blend, hist=(), hist_out=None)

    def tensors(lat):
        g = torch.Generator().manual_seed(9)
        return torch.randn(8, 4, *lat, generator=g).to(cuda), torch.randn(4, 4, *lat, generator=g).to(cuda)

    def entry(R):
        return (br.smooth_sums(4, 40, R, True, 77).to(cuda), 0.5, 0.45, True)

    rejects = []
    for lat in ((12, 64), (64, 12)):                      # res > H, res > W
        rejects.append((f"latent {lat} below the maps", *tensors(lat), None, entry(16), None))
    rejects.append(("H*W % 4 != 0", *tensors((17, 17)), None, entry(16), None))
    rejects.append(("res*res > 256", *tensors((64, 64)), None, entry(17), None))
    eps, x = tensors((64, 64))
    rejects.append(("x misaligned", eps, _misaligned(x), None, entry(16), None))
    rejects.append(("eps misaligned", _misaligned(eps), x, None, entry(16), None))
    rejects.append(("out misaligned", eps, x, None, entry(16), "misaligned"))
    rejects.append(("mask with blend sums", eps, x, torch.ones(4, 64, 64, dtype=torch.uint8, device=cuda), entry(16), None))
    for what, eps, x, mask, blend, out_kind in rejects:
        out = torch.full_like(x, 7.0)
        if out_kind:
            out = _misaligned(out)
        with pytest.raises(_hip.HipError):
            call(eps, x, out, mask, [blend])
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), what
    # and the same operands, aligned and in range, are served
    eps, x = tensors((64, 64))
    out = call(eps, x, torch.full_like(x, 7.0), None, [entry(16)])
    assert not bool((out == 7.0).any())
