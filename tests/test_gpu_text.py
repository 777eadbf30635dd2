"""The text encoder on the GPU: the causal attention kernel, LayerNorm with its adds and bias +
quick-GELU (csrc/p2p_text.hip) against the same formulas evaluated by torch in f32 from the same
16-bit inputs, the module's fused path against its own torch lines, and the pipeline handing the
encoder's causally mixed context to the U-Net."""
import copy

import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, null_text, ptp_utils, unet
from p2p_amd import pipeline as pl
from p2p_amd import text_encoder as te
from test_gpu_kernels import o_tol, ref_out, ref_probs
from test_gpu_unet_glue import check, rand

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
D = 64
SCALE = D ** -0.5
# (N, T, heads): the SD length, a length inside the second block, one full block, the largest
# length, one token, two full blocks
CASES = [(2, 77, 2), (2, 33, 2), (1, 32, 1), (2, 96, 2), (1, 1, 1), (3, 64, 3)]
SMALL = dict(vocab_size=49408, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2)
SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128), cross_attention_dim=128)   # test_gpu_pndm.py's, 128-d context
PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger"]

_cache = {}


def causal_ref(q, k, v, H):
    """f32 torch on the same 16-bit inputs, the future masked with triu(1)."""
    N, T, C = q.shape
    qh = q.float().reshape(N, T, H, D).permute(0, 2, 1, 3)
    kh = k.float().reshape(N, T, H, D).permute(0, 2, 1, 3)
    s = torch.einsum("nhid,nhjd->nhij", qh, kh) * SCALE
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return ref_out(s.softmax(-1), v, H)


def causal_case(N, T, H, dtype, dev):
    """One geometry's strided q / k / v (views of one [N, T, 3C] tensor) and its references,
    computed once and shared (never modified)."""
    key = (N, T, H, dtype)
    if key not in _cache:
        g = torch.Generator(device=dev).manual_seed(100 * T + 10 * N + H)
        C = H * D
        qkv = torch.randn(N, T, 3 * C, device=dev, generator=g).to(dtype)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        _cache[key] = (q, k, v, causal_ref(q, k, v, H), ref_out(ref_probs(q, k, H, SCALE), v, H))
    return _cache[key]


def bound(v, want):
    # tests/test_gpu_vae.py's bar for a 16-bit output
    return o_tol(v, "bf16") + 2.0 ** -8 * want.abs().max().item()


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------ 1. the causal kernel
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_causal_kernel_output(cuda, case, dtype):
    N, T, H = case
    q, k, v, want, unmasked = causal_case(N, T, H, dtype, cuda)
    assert q.stride(1) == k.stride(1) == v.stride(1) == 3 * H * D      # views of one QKV tensor
    o = _hip.causal_attn(q, k, v, H, SCALE)
    assert o is not None and o.shape == (N, T, H * D) and o.dtype == dtype and o.is_contiguous()
    assert torch.isfinite(o.float()).all()
    err, bar = (o.float() - want).abs().max().item(), bound(v, want)
    print(f"causal {case} {dtype}: max |O - ref| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    # dense operands: the same bits as the strided views
    o_dense = _hip.causal_attn(q.contiguous(), k.contiguous(), v.contiguous(), H, SCALE)
    assert torch.equal(bits(o_dense), bits(o))
    assert torch.equal(bits(_hip.causal_attn(q, k, v, H, SCALE)), bits(o)), "two launches on one input differ"
    if T >= 2:      # the negative control: the comparison sees the mask
        wrong = (o.float() - unmasked).abs().max().item()
        print(f"  against the unmasked reference: {wrong:.3e}, bar {bound(v, unmasked):.3e}")
        assert wrong > bound(v, unmasked)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("j", [0, 31, 32, 63])
def test_causal_kernel_rows_do_not_see_the_future(cuda, j, dtype):
    N, T, H = 2, 77, 2
    q, k, v, _, _ = causal_case(N, T, H, dtype, cuda)
    base = _hip.causal_attn(q, k, v, H, SCALE)
    g = torch.Generator(device=cuda).manual_seed(j + 1)
    q2, k2, v2 = (t.clone() for t in (q, k, v))
    for t in (q2, k2, v2):
        t[:, j + 1:] = (3.0 * torch.randn(N, T - j - 1, H * D, device=cuda, generator=g)).to(dtype)
    out = _hip.causal_attn(q2, k2, v2, H, SCALE)
    assert torch.equal(bits(out[:, :j + 1]), bits(base[:, :j + 1]))
    assert not torch.equal(bits(out[:, j + 1:]), bits(base[:, j + 1:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("T", [77, 33, 64])
def test_causal_kernel_reads_nothing_past_T(cuda, T, dtype):
    """q / k / v are the first T rows of a 96-row buffer whose other rows hold 6e4: finite, so a read
    past T would show as a wrong value, not as a fault."""
    N, H = 2, 2
    C = H * D
    q, k, v, want, _ = causal_case(N, T, H, dtype, cuda)
    buf = torch.full((N, 96, 3 * C), 6e4, dtype=dtype, device=cuda)
    buf[:, :T, :C], buf[:, :T, C:2 * C], buf[:, :T, 2 * C:] = q, k, v
    o = _hip.causal_attn(buf[:, :T, :C], buf[:, :T, C:2 * C], buf[:, :T, 2 * C:], H, SCALE)
    err, bar = (o.float() - want).abs().max().item(), bound(v, want)
    print(f"poisoned tail T={T} {dtype}: max |O - ref| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    assert torch.equal(bits(o), bits(_hip.causal_attn(q, k, v, H, SCALE)))


# ------------------------------------------------------------------ 2. LayerNorm
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["plain", "add", "add+bias+sum", "alias"])
@pytest.mark.parametrize("rows,C", [(77, 768), (154, 128), (1, 8), (231, 1280)])
def test_layer_norm(cuda, rows, C, mode, dtype, eps=1e-5):
    x = rand((rows, C), dtype, cuda, 1, 2.0, 0.5)
    gamma, beta = rand((C,), dtype, cuda, 2, 0.5, 1.0), rand((C,), dtype, cuda, 3)
    add = rand((rows, C), dtype, cuda, 4) if mode != "plain" else None
    bias = rand((C,), dtype, cuda, 5) if mode in ("add+bias+sum", "alias") else None
    x_in = x.clone()
    sum_out = {"plain": None, "add": None, "add+bias+sum": torch.empty_like(x), "alias": x_in}[mode]
    s = x.float()
    if add is not None:
        s = s + add.float()
    if bias is not None:
        s = s + bias.float()
    s = s.to(dtype)                                   # the rounded sum: what LayerNorm normalises
    ref = F.layer_norm(s.float(), (C,), gamma.float(), beta.float(), eps)
    chain = F.layer_norm(s, (C,), gamma, beta, eps)

    def run():
        return _hip.layer_norm(x_in, gamma, beta, eps, add=add, add_bias=bias, sum_out=sum_out)

    y = run()
    assert y is not None and y.shape == x.shape and y.dtype == dtype
    check(y, ref, dtype, f"layer_norm {rows}x{C} {mode} {dtype}", chain)
    if sum_out is not None:
        assert torch.equal(bits(sum_out), bits(s))
    if mode != "alias":                               # (in place, a second launch adds again)
        assert torch.equal(bits(x_in), bits(x))
        assert torch.equal(bits(run()), bits(y)), "two launches on the same input differ"
    else:
        x_in.copy_(x)
        assert torch.equal(bits(run()), bits(y)) and torch.equal(bits(x_in), bits(s))


# ------------------------------------------------------------------ 3. bias + quick-GELU
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("d", [3072, 512])
def test_bias_quick_gelu(cuda, d, inplace, dtype, rows=154):
    x = rand((2, rows // 2, d), dtype, cuda, 7, 2.0)
    bias = rand((d,), dtype, cuda, 8)
    h = x.float() + bias.float()
    ref = h * torch.sigmoid(1.702 * h)
    hc = x + bias
    chain = hc * torch.sigmoid(1.702 * hc)
    x_in = x.clone()
    y = _hip.bias_quick_gelu(x_in, bias, out=x_in if inplace else None)
    assert y is not None and y.shape == x.shape and y.dtype == dtype
    assert (y is x_in) == inplace
    check(y, ref, dtype, f"bias_quick_gelu {rows}x{d} inplace={inplace} {dtype}", chain)
    if not inplace:
        assert torch.equal(bits(x_in), bits(x))
        assert torch.equal(bits(_hip.bias_quick_gelu(x_in, bias)), bits(y))
        # a row-strided view of a wider buffer
        wide = rand((rows, d + 64), dtype, cuda, 9)
        wide[:, :d] = x.reshape(rows, d)
        assert torch.equal(bits(_hip.bias_quick_gelu(wide[:, :d], bias)), bits(y.reshape(rows, d)))


def test_unsupported_falls_back(cuda):
    # f32 and a channel count off the 16-byte vectors are "unsupported", not errors: None
    x, w = torch.randn(4, 128, device=cuda), torch.ones(128, device=cuda)
    assert _hip.layer_norm(x, w, w, 1e-5) is None
    assert _hip.bias_quick_gelu(x, w) is None
    xb, wb = torch.randn(4, 100, device=cuda).bfloat16(), torch.ones(100, device=cuda).bfloat16()
    assert _hip.layer_norm(xb, wb, wb, 1e-5) is None
    assert _hip.bias_quick_gelu(xb, wb) is None
    q = torch.randn(1, 8, 64, device=cuda)
    assert _hip.causal_attn(q, q, q, 1, SCALE) is None
    q40 = torch.randn(1, 8, 80, device=cuda).bfloat16()
    assert _hip.causal_attn(q40, q40, q40, 2, 40 ** -0.5) is None          # head dim 40
    q97 = torch.randn(1, 97, 64, device=cuda).bfloat16()
    assert _hip.causal_attn(q97, q97, q97, 1, SCALE) is None               # 97 tokens


# ------------------------------------------------------------------ 4. the module
def module_errors(cuda, m32, ids, dtype, monkeypatch):
    """tests/test_gpu_unet_glue.py's _module_errors rule on the encoder: the fused 16-bit module may be
    no further from the f32 module than the unfused 16-bit module plus one bf16 ulp of max |ref|."""
    m16 = copy.deepcopy(m32).to(dtype)
    layers = m16.text_model.encoder.layers
    launches = []
    real = _hip.causal_attn

    def spy(*a, **kw):
        out = real(*a, **kw)
        launches.append(out is not None)
        return out

    monkeypatch.setattr(_hip, "causal_attn", spy)
    with torch.no_grad():
        ref = m32(ids)
        fused = m16(ids)
        assert [l.fused_calls for l in layers] == [1] * len(layers), "the fused path was not taken"
        assert launches == [True] * len(layers), "the causal kernel was not launched"
        monkeypatch.setattr(te, "FUSED_ATTENTION", False)
        glue_only = m16(ids)
        assert [l.fused_calls for l in layers] == [2] * len(layers) and len(launches) == len(layers)
        monkeypatch.setattr(te, "FUSED_ATTENTION", True)
        monkeypatch.setattr(unet, "FUSE_UNET", False)
        plain = m16(ids)
        assert [l.fused_calls for l in layers] == [2] * len(layers)
    for name, i in (("last_hidden_state", 0), ("pooler_output", 1)):
        top = ref[i].abs().max().item()
        e_f, e_g, e_p = ((o[i].float() - ref[i]).abs().max().item() for o in (fused, glue_only, plain))
        print(f"{name} {dtype}: fused err {e_f:.4e}, fused glue + torch attention {e_g:.4e}, unfused {e_p:.4e}, "
              f"max|ref| {top:.3f}")
        assert fused[i].dtype == dtype and torch.isfinite(fused[i].float()).all()
        assert e_f <= e_p + 2.0 ** -8 * top
        assert e_g <= e_p + 2.0 ** -8 * top


def tokenizer_ids(cuda, prompts):
    from p2p_amd.tokenizer import StandInTokenizer
    return StandInTokenizer()(prompts, padding="max_length", max_length=77).input_ids.to(cuda)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_module_small(cuda, monkeypatch, dtype):
    m32 = te.CLIPTextModel(**SMALL, generator=torch.Generator().manual_seed(1)).to(cuda).eval()
    module_errors(cuda, m32, tokenizer_ids(cuda, PROMPTS + [""]), dtype, monkeypatch)


def test_module_sd_shape(cuda, monkeypatch):
    """768-wide rows and 12 heads meet only here."""
    m32 = te.CLIPTextModel(generator=torch.Generator().manual_seed(2)).to(cuda).eval()
    module_errors(cuda, m32, tokenizer_ids(cuda, PROMPTS), torch.bfloat16, monkeypatch)


# ------------------------------------------------------------------ 5. end to end
def test_text2image_with_the_clip_encoder(cuda):
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=SMALL_UNET,
                                        text_encoder_config=SMALL)
    assert isinstance(model.text_encoder, te.CLIPTextModel) and model.text_encoder.dtype == torch.bfloat16
    steps = 3
    lb = null_text.LocalBlend(PROMPTS, (("squirrel",), ("lion",)), th=(.3, .3), device=cuda)
    lb.start_blend = 1
    ctrl = null_text.AttentionReplace(PROMPTS, steps, cross_replace_steps=.8, self_replace_steps=.4, local_blend=lb,
                                      device=cuda)
    seen = []
    hook = model.unet.register_forward_pre_hook(lambda mod, args, kw: seen.append(kw["encoder_hidden_states"]),
                                                with_kwargs=True)
    try:
        latents, _ = ptp_utils.text2image_ldm_stable(model, PROMPTS, ctrl, num_inference_steps=steps,
                                                     latent=pl.seed_latent(4))
    finally:
        hook.remove()
    assert latents.shape == (2, 4, 64, 64) and torch.isfinite(latents.float()).all()
    layers = model.text_encoder.text_model.encoder.layers
    assert all(l.fused_calls == 2 for l in layers)          # the prompts and the uncond "" rows
    assert len(seen) == steps and all(c is seen[0] for c in seen)
    ctx = seen[0]
    with torch.no_grad():
        want = torch.cat([model.text_encoder(tokenizer_ids(cuda, [""] * 2))[0],
                          model.text_encoder(tokenizer_ids(cuda, PROMPTS))[0]])
    assert ctx.shape == (4, 77, 128) and torch.equal(ctx, want)
    # a one-word swap: the rows before the swapped word are the source's bit for bit, the swapped
    # word's row and every later one differ -- CLIP's causal mixing, which the stand-in never had
    tok = model.tokenizer
    swap = tok.encode(PROMPTS[0]).index(tok.encode("squirrel")[1])
    src, edit = ctx[2], ctx[3]
    assert torch.equal(src[:swap], edit[:swap])
    assert all(not torch.equal(src[t], edit[t]) for t in range(swap, 77))
