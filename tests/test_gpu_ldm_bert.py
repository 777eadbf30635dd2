"""LDMBert on the GPU: the bidirectional attention kernel with its key counts and bias + erf-GELU
(csrc/p2p_text.hip) against the same formulas evaluated by torch in f32 from the same 16-bit inputs,
the module's fused path against its own torch lines, and the LDM-256 pipeline handing the encoder's
fully mixed context to the U-Net and uint8 images back."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, controllers, ptp_utils, unet
from p2p_amd import ldm_bert as lb
from p2p_amd import pipeline as pl
from test_gpu_kernels import ref_out
from test_gpu_text import D, DTYPES, SCALE, SMALL_UNET, bits, bound, causal_case, tokenizer_ids
from test_gpu_unet_glue import check, rand

pytestmark = pytest.mark.gpu

# test_gpu_text.py's geometries and LDMBert's own eight heads
CASES = [(2, 77, 2), (2, 33, 2), (1, 32, 1), (2, 96, 2), (1, 1, 1), (3, 64, 3), (1, 77, 8)]
SMALL = dict(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=512)   # on the pipeline's vocabulary
# four levels, as the f8 autoencoder has (32 x 32 latents -> 256 x 256 images), at a fraction of its widths
SMALL_VQVAE = dict(block_out_channels=(32, 32, 64, 64), layers_per_block=1, norm_num_groups=8)
TRUE_WIDTHS = dict(vocab_size=49408, encoder_layers=2)      # 1280 / 8 x 64 / 5120, two of the 32 layers


def counted_ref(q, k, v, H, counts):
    """f32 torch on the same 16-bit inputs, entry n restricted to its first counts[n] keys."""
    N, T, C = q.shape
    qh = q.float().reshape(N, T, H, D).permute(0, 2, 1, 3)
    kh = k.float().reshape(N, T, H, D).permute(0, 2, 1, 3)
    s = torch.einsum("nhid,nhjd->nhij", qh, kh) * SCALE
    hidden = torch.arange(T, device=q.device)[None, :] >= torch.as_tensor(counts, device=q.device)[:, None]
    s = s.masked_fill(hidden[:, None, None, :], float("-inf"))
    return ref_out(s.softmax(-1), v, H)


# ------------------------------------------------------------------ 1. the bidirectional kernel
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_text_attn_output(cuda, case, dtype):
    N, T, H = case
    q, k, v, causal, want = causal_case(N, T, H, dtype, cuda)      # want: the unmasked f32 reference
    assert q.stride(1) == k.stride(1) == v.stride(1) == 3 * H * D      # views of one QKV tensor
    o = _hip.text_attn(q, k, v, H, SCALE)
    assert o is not None and o.shape == (N, T, H * D) and o.dtype == dtype and o.is_contiguous()
    assert torch.isfinite(o.float()).all()
    err, bar = (o.float() - want).abs().max().item(), bound(v, want)
    print(f"text_attn {case} {dtype}: max |O - ref| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    # dense operands: the same bits as the strided views
    o_dense = _hip.text_attn(q.contiguous(), k.contiguous(), v.contiguous(), H, SCALE)
    assert torch.equal(bits(o_dense), bits(o))
    assert torch.equal(bits(_hip.text_attn(q, k, v, H, SCALE)), bits(o)), "two launches on one input differ"
    if T >= 2:      # the negative control: the comparison tells the two kernels apart
        wrong = (o.float() - causal).abs().max().item()
        print(f"  against the causal reference: {wrong:.3e}, bar {bound(v, causal):.3e}")
        assert wrong > bound(v, causal)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("T", [77, 33, 64])
def test_text_attn_tail(cuda, T, dtype):
    """q / k / v are the first T rows of a 96-row buffer whose other rows hold 6e4: finite, so a read
    past T would show as a wrong value, not as a fault -- and so would keys T .. 95 left unmasked
    (zero rows of the tile score 0, not -inf), the case the causal kernel never needed."""
    N, H = 2, 2
    C = H * D
    q, k, v, _, want = causal_case(N, T, H, dtype, cuda)
    buf = torch.full((N, 96, 3 * C), 6e4, dtype=dtype, device=cuda)
    buf[:, :T, :C], buf[:, :T, C:2 * C], buf[:, :T, 2 * C:] = q, k, v
    o = _hip.text_attn(buf[:, :T, :C], buf[:, :T, C:2 * C], buf[:, :T, 2 * C:], H, SCALE)
    err, bar = (o.float() - want).abs().max().item(), bound(v, want)
    print(f"poisoned tail T={T} {dtype}: max |O - ref| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    assert torch.equal(bits(o), bits(_hip.text_attn(q, k, v, H, SCALE)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_text_attn_key_counts(cuda, dtype):
    N, T, H = 6, 77, 2
    counts = [1, 31, 32, 33, 64, T]
    q, k, v, _, _ = causal_case(N, T, H, dtype, cuda)
    kc = torch.tensor(counts, dtype=torch.int32, device=cuda)
    want = counted_ref(q, k, v, H, counts)
    o = _hip.text_attn(q, k, v, H, SCALE, key_counts=kc)
    assert o is not None and o.shape == (N, T, H * D) and torch.isfinite(o.float()).all()
    for n, c in enumerate(counts):      # every entry, all T rows of it
        err, bar = (o[n].float() - want[n]).abs().max().item(), bound(v[n], want[n])
        print(f"key_counts {dtype} count {c}: max |O - ref| = {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (c, err, bar)
    # the negative control: the unmasked kernel misses the bar of the entries that lose more than
    # half their keys (13 keys of 77 hidden need not move a row past it)
    full = _hip.text_attn(q, k, v, H, SCALE)
    for n, c in enumerate(counts[:-2]):
        assert (full[n].float() - want[n]).abs().max().item() > bound(v[n], want[n]), c
    assert torch.equal(bits(full[-1]), bits(o[-1]))
    # what stands at or behind the count is never seen
    g = torch.Generator(device=cuda).manual_seed(11)
    k2, v2 = k.clone(), v.clone()
    for n, c in enumerate(counts):
        for t in (k2, v2):
            t[n, c:] = (3.0 * torch.randn(T - c, H * D, device=cuda, generator=g)).to(dtype)
    assert torch.equal(bits(_hip.text_attn(q, k2, v2, H, SCALE, key_counts=kc)), bits(o))
    # counts of T: the bits of the call without counts
    all_T = torch.full((N,), T, dtype=torch.int32, device=cuda)
    assert torch.equal(bits(_hip.text_attn(q, k, v, H, SCALE, key_counts=all_T)), bits(full))


# ------------------------------------------------------------------ 2. bias + erf-GELU
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("d", [5120, 512])
def test_bias_gelu(cuda, d, inplace, dtype, rows=154):
    x = rand((2, rows // 2, d), dtype, cuda, 7, 2.0)
    bias = rand((d,), dtype, cuda, 8)
    ref = F.gelu(x.float() + bias.float())
    chain = F.gelu(x + bias)
    x_in = x.clone()
    y = _hip.bias_gelu(x_in, bias, out=x_in if inplace else None)
    assert y is not None and y.shape == x.shape and y.dtype == dtype
    assert (y is x_in) == inplace
    check(y, ref, dtype, f"bias_gelu {rows}x{d} inplace={inplace} {dtype}", chain)
    if not inplace:
        assert torch.equal(bits(x_in), bits(x))
        assert torch.equal(bits(_hip.bias_gelu(x_in, bias)), bits(y))
        # a row-strided view of a wider buffer
        wide = rand((rows, d + 64), dtype, cuda, 9)
        wide[:, :d] = x.reshape(rows, d)
        assert torch.equal(bits(_hip.bias_gelu(wide[:, :d], bias)), bits(y.reshape(rows, d)))
        # the negative control: the comparison tells the two activations apart
        with pytest.raises(AssertionError):
            check(_hip.bias_quick_gelu(x_in, bias), ref, dtype, "quick-GELU against the erf reference")


def test_unsupported_falls_back(cuda):
    x, w = torch.randn(4, 128, device=cuda), torch.ones(128, device=cuda)
    assert _hip.bias_gelu(x, w) is None                                    # f32
    xb, wb = torch.randn(4, 100, device=cuda).bfloat16(), torch.ones(100, device=cuda).bfloat16()
    assert _hip.bias_gelu(xb, wb) is None                                  # off the 16-byte vectors
    q = torch.randn(1, 8, 64, device=cuda)
    assert _hip.text_attn(q, q, q, 1, SCALE) is None
    q40 = torch.randn(1, 8, 80, device=cuda).bfloat16()
    assert _hip.text_attn(q40, q40, q40, 2, 40 ** -0.5) is None            # head dim 40
    q97 = torch.randn(1, 97, 64, device=cuda).bfloat16()
    assert _hip.text_attn(q97, q97, q97, 1, SCALE) is None                 # 97 tokens
    qu = torch.randn(1, 8, 72, device=cuda).bfloat16()[..., 4:68]
    assert _hip.text_attn(qu, qu, qu, 1, SCALE) is None                    # operands off 16 bytes
    q8 = torch.randn(2, 8, 64, device=cuda).bfloat16()
    with pytest.raises(_hip.HipError):
        _hip.text_attn(q8, q8, q8, 1, SCALE, key_counts=torch.ones(2, dtype=torch.int64, device=cuda))


# ------------------------------------------------------------------ 3. the module
def module_errors(cuda, m32, ids, dtype, monkeypatch, mask=None, counts=None):
    """test_gpu_text.py's module_errors rule on this encoder: the fused 16-bit module may be no
    further from the f32 module than the unfused 16-bit module plus one bf16 ulp of max |ref|.
    ``counts``: what the kernel must be handed for ``mask`` (None: no counts)."""
    m16 = copy.deepcopy(m32).to(dtype)
    layers = m16.model.layers
    launches = []
    real = _hip.text_attn

    def spy(q, k, v, heads, scale, key_counts=None):
        out = real(q, k, v, heads, scale, key_counts)
        launches.append((out is not None, None if key_counts is None else key_counts.tolist()))
        return out

    monkeypatch.setattr(_hip, "text_attn", spy)
    with torch.no_grad():
        ref = m32(ids, mask)[0]
        fused = m16(ids, mask)[0]
        assert [l.fused_calls for l in layers] == [1] * len(layers), "the fused path was not taken"
        assert launches == [(True, counts)] * len(layers), "the kernel was not launched, or not with these counts"
        monkeypatch.setattr(lb, "FUSED_ATTENTION", False)
        glue_only = m16(ids, mask)[0]
        assert [l.fused_calls for l in layers] == [2] * len(layers) and len(launches) == len(layers)
        monkeypatch.setattr(lb, "FUSED_ATTENTION", True)
        monkeypatch.setattr(unet, "FUSE_UNET", False)
        plain = m16(ids, mask)[0]
        assert [l.fused_calls for l in layers] == [2] * len(layers) and len(launches) == len(layers)
    top = ref.abs().max().item()
    e_f, e_g, e_p = ((o.float() - ref).abs().max().item() for o in (fused, glue_only, plain))
    print(f"hidden states {dtype}: fused err {e_f:.4e}, fused glue + torch attention {e_g:.4e}, unfused {e_p:.4e}, "
          f"max|ref| {top:.3f}")
    assert fused.dtype == dtype and fused.shape == ref.shape and torch.isfinite(fused.float()).all()
    assert e_f <= e_p + 2.0 ** -8 * top
    assert e_g <= e_p + 2.0 ** -8 * top
    return m16, ref, plain


def small_model(cuda, seed=1):
    return lb.LDMBertModel(vocab_size=49408, **SMALL, generator=torch.Generator().manual_seed(seed)).to(cuda).eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_module_small(cuda, monkeypatch, dtype):
    module_errors(cuda, small_model(cuda), tokenizer_ids(cuda, pl.LDM_PROMPTS + [""]), dtype, monkeypatch)


def test_module_true_widths(cuda, monkeypatch):
    """1280-wide rows, a 512-wide attention of eight heads and the 5120 MLP meet only here."""
    m32 = lb.LDMBertModel(**TRUE_WIDTHS, generator=torch.Generator().manual_seed(2)).to(cuda).eval()
    module_errors(cuda, m32, tokenizer_ids(cuda, pl.LDM_PROMPTS), torch.bfloat16, monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_module_masks(cuda, monkeypatch, dtype):
    m32 = small_model(cuda, seed=3)
    ids = tokenizer_ids(cuda, pl.LDM_PROMPTS + [""])
    lengths = [11, 77, 2]
    mask = (torch.arange(77, device=cuda)[None, :] < torch.tensor(lengths, device=cuda)[:, None]).long()
    # a prefix mask reaches the kernel as counts
    module_errors(cuda, m32, ids, dtype, monkeypatch, mask=mask, counts=lengths)
    monkeypatch.undo()
    # a mask with a hole is no prefix: the torch lines, and still the module's answer
    holes = mask.clone()
    holes[:, 1] = 0
    holes[2, 0] = 1
    m16 = copy.deepcopy(m32).to(dtype)
    called = []
    monkeypatch.setattr(_hip, "text_attn", lambda *a, **kw: called.append(1))
    with torch.no_grad():
        ref, got = m32(ids, holes)[0], m16(ids, holes)[0]
        assert not called and [l.fused_calls for l in m16.model.layers] == [0, 0]
        monkeypatch.setattr(unet, "FUSE_UNET", False)
        plain = m16(ids, holes)[0]
    err, top = (got.float() - ref).abs().max().item(), ref.abs().max().item()
    print(f"non-prefix mask {dtype}: max |16-bit - f32 module| = {err:.4e}, max|ref| {top:.3f}")
    # the same torch lines, whatever the switch says: the unfused 16-bit module's bits
    assert torch.isfinite(got.float()).all() and torch.equal(got, plain)


# ------------------------------------------------------------------ 4. end to end
def test_text2image_ldm_with_ldmbert_and_vqvae(cuda):
    model = pl.SyntheticLatentDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=SMALL_UNET, bert_config=SMALL,
                                        vqvae_config=SMALL_VQVAE)
    assert isinstance(model.bert, lb.LDMBertModel) and model.bert.dtype == torch.bfloat16
    assert model.bert.model.embed_tokens.num_embeddings == 49408
    steps = 3
    ctrl = controllers.AttentionReplace(pl.LDM_PROMPTS, steps, cross_replace_steps=0.8, self_replace_steps=0.4,
                                        device=cuda)
    seen, decoded = [], []
    hook = model.unet.register_forward_pre_hook(lambda mod, args, kw: seen.append(kw["encoder_hidden_states"]),
                                                with_kwargs=True)
    decode = model.vqvae.decode

    def spy(z):
        decoded.append(z)
        return decode(z)

    model.vqvae.decode = spy
    try:
        image, x_T = ptp_utils.text2image_ldm(model, pl.LDM_PROMPTS, ctrl, num_inference_steps=steps,
                                              latent=pl.ldm_seed_latent(4))
    finally:
        hook.remove()
        del model.vqvae.decode
    # (the reference's latent2image hands back a numpy array)
    assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (2, 256, 256, 3)
    assert len(decoded) == 1 and decoded[0].shape == (2, 4, 32, 32) and torch.isfinite(decoded[0].float()).all()
    assert all(l.fused_calls == 2 for l in model.bert.model.layers)          # the prompts and the uncond "" rows
    assert len(seen) == steps and all(c is seen[0] for c in seen)
    ctx = seen[0]
    ids = tokenizer_ids(cuda, pl.LDM_PROMPTS)
    with torch.no_grad():
        want = torch.cat([model.bert(tokenizer_ids(cuda, [""] * 2))[0], model.bert(ids)[0]])
    assert ctx.shape == (4, 77, 128) and torch.equal(ctx, want)
    # a one-word swap moves all 77 rows; the embedding-table stand-in moves the swapped word's alone
    src, edit = ctx[2], ctx[3]
    assert all(not torch.equal(src[t], edit[t]) for t in range(77))
    swapped = (ids[0] != ids[1]).tolist()
    assert 1 <= sum(swapped) < 77
    table = pl.SyntheticTextEncoder(dim=1280, seed=2).to(cuda)(ids)[0]
    assert [not torch.equal(table[0, t], table[1, t]) for t in range(77)] == swapped
