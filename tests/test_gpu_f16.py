"""float16 inputs (a Stable Diffusion model loaded with torch_dtype=torch.float16) through every
forward kernel and the latent step (GPU).

fp16 q/k/v run on the 16-bit MFMA pipe with f16 operands: Q K^T products of two 11-bit values are
exact in the f32 accumulator, P is packed to f16 for the PV product, O is rounded to f16 once.
Bars: the project's 16-bit-pipe bar for O (2^-7 max|V|, test_gpu_kernels.o_tol) plus one f16
output ulp; 2e-3 for probabilities; bit-exactness where it can be derived (one-hot rows, the
latent step against torch's eager fp16 arithmetic).
"""
import pytest
import torch

from oracle import control as oc
from oracle_runs import oracle_controller
from p2p_amd import _hip, attention, config, controllers
from p2p_amd import null_text as pn
from p2p_amd import pipeline as pl

from test_gpu_controllers import EDIT_LAYERS, PROMPTS, SD_LAYERS, _edit_pair, run_pair
from test_gpu_kernels import make_qkv, o_tol, ref_out, ref_probs
from test_gpu_latent import eager, sched

pytestmark = pytest.mark.gpu

F16 = torch.float16


def o_bar(v, want):
    """The 16-bit pipe's O bar plus one rounding of the stored fp16 output."""
    return o_tol(v, "bf16") + 2.0 ** -10 * want.abs().max().item()


# ------------------------------------------------------------------ 1. selection, bit-exact
def _selection_inputs(N, P, K, H, d, j, seed):
    """q = 8 everywhere, key j = 8 everywhere, every other key and all of V random fp16: the f32
    softmax is exactly one-hot at key j (its logit leads by hundreds of log2 units), every product is
    exact, so O must be V[:, j] bit for bit -- and most fp16 V values are not bf16 values, so a path
    that detours through bf16 cannot pass."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    C = H * d
    q = torch.full((N, P, C), 8.0, device="cuda", dtype=F16)
    k = torch.randn(N, K, C, device="cuda", generator=g).half()
    v = torch.randn(N, K, C, device="cuda", generator=g).half()
    k[:, j, :] = 8.0
    return q, k, v


def _assert_one_hot(q, k, H, d, j):
    p = ref_probs(q, k, H, d ** -0.5)
    assert torch.equal(p[..., j], torch.ones_like(p[..., j]))
    assert p.sum(-1).eq(1).all()


# (N, P, K, H, d, j); the d = 40 / 80 shapes of the tuned kernels: test_gpu_f16_tuned.py
SELECT_SELF = [(2, 256, 256, 2, 160, 250), (2, 64, 64, 2, 160, 60), (2, 100, 130, 2, 64, 120), (3, 33, 96, 2, 8, 90)]


def check_selection_self(geom):
    N, P, K, H, d, j = geom
    q, k, v = _selection_inputs(N, P, K, H, d, j, seed=d + j)
    _assert_one_hot(q, k, H, d, j)
    assert (v != v.bfloat16().half()).float().mean().item() > 0.8
    o = torch.empty_like(q)
    _hip.self_attn(q, k, v, o, H, d ** -0.5)
    assert o.dtype == F16
    assert torch.equal(o, v[:, j:j + 1].expand_as(o))


@pytest.mark.parametrize("geom", SELECT_SELF, ids=lambda g: "x".join(map(str, g)))
def test_selection_self_bit_exact(cuda, geom):
    check_selection_self(geom)


@pytest.mark.parametrize("geom", [(4, 4096, 77, 2, 40, 70), (4, 1024, 77, 2, 80, 70)],
                         ids=lambda g: "x".join(map(str, g)))
def test_selection_cross_bit_exact(cuda, geom):
    N, P, K, H, d, j = geom
    q, k, v = _selection_inputs(N, P, K, H, d, j, seed=d + j)
    _assert_one_hot(q, k, H, d, j)
    o = torch.empty_like(q)
    _hip.cross_attn(q, k, v, o, H, d ** -0.5, [(n, 1, None, None) for n in range(N)])
    assert torch.equal(o, v[:, j:j + 1].expand_as(o))


def test_selection_pv_bit_exact(cuda):
    N, P, K, H, d, j = 2, 40, 1100, 2, 64, 1090
    _, _, v = _selection_inputs(N, P, K, H, d, j, seed=3)
    probs = torch.zeros(N * H, P, K, device=cuda)
    probs[..., j] = 1.0
    o = torch.empty(N, P, H * d, device=cuda, dtype=F16)
    _hip.attn_pv(probs, v, o, H)
    assert torch.equal(o, v[:, j:j + 1].expand_as(o))


# ------------------------------------------------------------------ 3. stored probabilities
@pytest.mark.parametrize("geom,qscale", [((2, 1024, 1024, 2, 80), 16.0), ((2, 256, 256, 4, 160), 8.0)],
                         ids=["1024x80", "256x160"])
def test_self_attention_store_probs_f16_inputs(cuda, geom, qscale):
    N, P, K, H, d = geom
    q, k, v = make_qkv(N, P, K, H, d, F16, qscale=qscale, seed=3)
    o = torch.empty_like(q)
    scale = d ** -0.5
    store = torch.full((N * H, P, K), 7.0, device=cuda)
    slots = [n * H for n in range(N)]
    _hip.self_attn(q, k, v, o, H, scale, store=store, store_slot=slots, accumulate=False)
    p = ref_probs(q, k, H, scale)
    assert (store - p.reshape(N * H, P, K)).abs().max().item() < 2e-3
    _hip.self_attn(q, k, v, o, H, scale, store=store, store_slot=slots, accumulate=True)
    assert (store - 2 * p.reshape(N * H, P, K)).abs().max().item() < 4e-3
    want = ref_out(p, v, H)
    assert (o.float() - want).abs().max().item() < o_bar(v, want)


# ------------------------------------------------------------------ 4. materialise
@pytest.mark.parametrize("geom", [(4, 256, 77, 8, 160), (2, 33, 130, 2, 8)], ids=lambda g: "x".join(map(str, g)))
def test_probs_and_pv_materialise_f16_inputs(cuda, geom):
    N, P, K, H, d = geom
    q, k, v = make_qkv(N, P, K, H, d, F16, qscale=4.0, seed=11)
    probs = torch.empty(N * H, P, K, device=cuda)
    _hip.attn_probs(q, k, H, d ** -0.5, probs)
    p = ref_probs(q, k, H, d ** -0.5).reshape(N * H, P, K)
    assert (probs - p).abs().max().item() < 2e-3
    o = torch.empty_like(q)
    _hip.attn_pv(probs, v, o, H)
    assert o.dtype == F16
    want = ref_out(probs.reshape(N, H, P, K), v, H)
    assert (o.float() - want).abs().max().item() < o_bar(v, want)


# ------------------------------------------------------------------ 5. edits at SD geometry
@pytest.mark.parametrize("edit", ["refine", "reweight", "reweight_refine", "reweight_replace"])
def test_edits_f16_inputs_sd_geometry(cuda, tok, edit):
    steps = 2
    with config.compute_mode("bf16"):
        prompts, prod, orc = _edit_pair(edit, tok, cuda, 10)
        assert prod.fused_supported()
        assert prod._edit_program().dense_f16() is not None
        run_pair(prod, orc, EDIT_LAYERS, steps, 4e-2, 2e-3 * steps, qscale=16.0, prompts=prompts,
                 io_dtype=F16, seed=16)


def test_replace_with_localblend_f16_inputs_sd_geometry(cuda, tok):
    words = (("squirrel", "burger"), ("lion",), ("cat",), ("lasagna",))
    steps = 2
    with config.compute_mode("bf16"):
        lb = pn.LocalBlend(PROMPTS, words, start_blend=0.0, tokenizer=tok, device=cuda)
        prod = pn.AttentionReplace(PROMPTS, 50, {"default_": .8, "lasagna": .3}, .4, local_blend=lb,
                                   tokenizer=tok, device=cuda)
        olb = oc.OracleLocalBlend("null", PROMPTS, words, tok, start_blend=0.0)
        orc = oc.OracleController("null", "replace", PROMPTS, 50, {"default_": .8, "lasagna": .3}, .4, tok,
                                  local_blend=olb)
        orc.mapper = orc.mapper.to(cuda)
        orc.alpha = orc.alpha.to(cuda)
        olb.alpha = olb.alpha.to(cuda)
        x_t = torch.randn(4, 4, 64, 64, device=cuda)
        run_pair(prod, orc, SD_LAYERS, steps, 4e-2, 2e-3 * steps, x_t=x_t, io_dtype=F16)


# ------------------------------------------------------------------ 6. latent step
@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("t", [980, 0])
def test_fused_prev_step_bit_exact_f16_eps(cuda, B, with_mask, t):
    g = torch.Generator(device=cuda).manual_seed(B * 1000 + t)
    eps = torch.randn(2 * B, 4, 64, 64, device=cuda, generator=g).half()
    x = torch.randn(B, 4, 64, 64, device=cuda, generator=g)
    mask = (torch.rand(B, 64, 64, device=cuda, generator=g) > 0.5).to(torch.uint8) if with_mask else None
    coeffs = sched().prev_coeffs(t)
    got = _hip.latent_step(eps, x, torch.empty_like(x), coeffs, 7.5, mask)
    want = eager(eps, x, coeffs, 7.5, mask)
    assert want.dtype == torch.float32
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("sub,groups", [(False, (True,)), (True, (True, False, True))],
                         ids=["one_group_nosub", "three_groups_substruct"])
def test_latent_step_builds_folded_blend_mask_f16_eps(cuda, sub, groups):
    """test_latent_step_builds_folded_blend_mask with fp16 eps: the one-launch LocalBlend + latent
    step equals the mask-reading latent step bit for bit."""
    gs, H, L = 4, 8, 5
    G = len(groups)
    B = G * gs
    g = torch.Generator(device=cuda).manual_seed(17 + G + 2 * sub)
    eps = torch.randn(2 * B, 4, 64, 64, device=cuda, generator=g).half()
    x = torch.randn(B, 4, 64, 64, device=cuda, generator=g)
    coeffs = sched().prev_coeffs(500)
    maps = [torch.zeros(gs * H, 256, 77, device=cuda) for _ in range(L)]
    alpha = torch.ones(gs, 77, device=cuda)
    subt = torch.ones(gs, 77, device=cuda) if sub else None
    blend, masks = [], []
    for on in groups:
        base = torch.rand(gs * 2, 1, 4, 4, device=cuda, generator=g) ** 3
        field = torch.nn.functional.interpolate(base, size=(16, 16), mode="bilinear", align_corners=False)
        sums = field.reshape(gs, 2, 1, 256) * (0.8 + 0.4 * torch.rand(gs, 2, L * H, 256, device=cuda, generator=g))
        sums = sums.contiguous()
        if not sub:
            sums[:, 1] = 0
        fm = controllers.FoldedBlendMask(maps, H, alpha, subt, 0.5, 0.45, (64, 64), sums)
        blend.append(fm.latent_entry() if on else None)
        masks.append(fm.materialize() if on else torch.zeros(gs, 64, 64, dtype=torch.uint8, device=cuda))
    got = _hip.latent_step(eps, x, torch.empty_like(x), coeffs, 7.5, None, gs if G > 1 else 0, None, blend)
    gb = torch.tensor([1 if on else 0 for on in groups], dtype=torch.uint8, device=cuda)
    want = _hip.latent_step(eps, x, torch.empty_like(x), coeffs, 7.5, torch.cat(masks), gs if G > 1 else 0,
                            gb if G > 1 else None)
    frac = torch.cat(masks).float().mean().item()
    assert 0.05 < frac < 0.95, frac
    assert torch.equal(got, want), (got - want).abs().max().item()


# ------------------------------------------------------------------ 7. end to end, teacher-forced
def test_f16_unet_teacher_forced_every_call(cuda, tok):
    """test_bench_config_teacher_forced_every_call's construction with an fp16 U-Net, 5 DDIM steps
    (0-1 inside the self-injection window, 0-3 inside the cross window, 4 outside both): every
    attention call's fp16 q / k / v also go through the oracle's fp32 softmax + reference
    controller; the product's O must match within 2^-7 max|V|, the stored cross maps within 2e-3
    per accumulated step."""
    steps = 5
    prompts = pl.north_star_prompts()
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=F16)
    ctrl = pl.make_replace_controller(prompts, steps, device=cuda)
    octrl = oracle_controller("replace", prompts, tok, steps, cuda)
    orig = ctrl.attention
    worst = {"self": 0.0, "cross": 0.0}
    calls = {"self": 0, "cross": 0}

    def split(t, heads):
        t = t.float()
        return t.reshape(t.shape[0], t.shape[1], heads, -1).permute(0, 2, 1, 3)

    def attn_hook(q, k, v, heads, scale, is_cross, place_in_unet, mask=None):
        assert q.dtype == k.dtype == v.dtype == F16
        out = orig(q, k, v, heads, scale, is_cross, place_in_unet, mask)
        octrl.num_att_layers = ctrl.num_att_layers
        N = q.shape[0]
        attn = (torch.einsum("nhid,nhjd->nhij", split(q, heads), split(k, heads)) * scale).softmax(-1)
        attn = octrl(attn.reshape(N * heads, q.shape[1], k.shape[1]), is_cross, place_in_unet)
        ref = torch.einsum("nhij,nhjd->nhid", attn.reshape(N, heads, q.shape[1], k.shape[1]), split(v, heads))
        ref = ref.permute(0, 2, 1, 3).reshape(q.shape)
        kind = "cross" if is_cross else "self"
        err = (out.float() - ref).abs().max().item() / v.float().abs().max().item()
        worst[kind] = max(worst[kind], err)
        calls[kind] += 1
        return out

    ctrl.attention = attn_hook
    with config.compute_mode("bf16"):
        latents = pl.run_edit_group(model, prompts, ctrl, pl.seed_latent(0), num_steps=steps)
    torch.cuda.synchronize()
    lat = latents[0] if isinstance(latents, (tuple, list)) else latents
    assert torch.isfinite(lat.float()).all()
    print(f"fp16 U-Net, teacher-forced at every call: {calls}, worst |O - O_oracle| / max|V| "
          f"self {worst['self']:.2e}, cross {worst['cross']:.2e} (bar {2.0 ** -7:.2e})")
    assert calls == {"self": 16 * steps, "cross": 16 * steps}, calls
    assert worst["self"] < 2.0 ** -7 and worst["cross"] < 2.0 ** -7, worst
    assert ctrl.cur_step == octrl.cur_step == steps
    worst_map = 0.0
    for key in ("down_cross", "mid_cross", "up_cross"):
        ours, ref = ctrl.attention_store[key], octrl.attention_store[key]
        assert len(ours) == len(ref) > 0, key
        for x, y in zip(ours, ref):
            worst_map = max(worst_map, (x - y).abs().max().item())
    print(f"  stored cross maps: worst |diff| {worst_map:.3e} = {worst_map / steps:.2e} per accumulated step")
    assert worst_map < 2e-3 * steps


# ------------------------------------------------------------------ 8. refusals
def test_f16_backward_is_refused_before_any_launch(cuda):
    q, k, v = make_qkv(1, 64, 64, 2, 40, F16)
    q.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        attention.plain_attention(q, k, v, 2, 40 ** -0.5)


def test_f16_in_f32_check_mode_is_refused(cuda):
    q, k, v = make_qkv(1, 64, 64, 2, 40, F16)
    with config.compute_mode("f32"):
        with pytest.raises(_hip.HipError):
            attention.plain_attention(q, k, v, 2, 40 ** -0.5)
