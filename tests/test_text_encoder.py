"""The CLIP text encoder (p2p_amd/text_encoder.py) as far as a CPU can check: parity of its torch
lines with the installed transformers model on the same weights (which also pins the parameter
names), causality, the SD-v1.4 shapes, the pipeline switch, and the argument checks of the three
new entry points (no launch)."""
import ctypes

import pytest
import torch

from p2p_amd import _hip, ptp_utils
from p2p_amd import pipeline as pl
from p2p_amd import text_encoder as te

from test_capi import _tensors

SMALL = dict(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
             eos_token_id=999)
BOS = 998
# the pipeline's tokenizer hands out ids up to 49407: the small shape with the full vocabulary
SMALL_FULL_VOCAB = dict(SMALL, vocab_size=49408, eos_token_id=49407)
NARROW_UNET = dict(block_out_channels=(32, 64, 64, 64), cross_attention_dim=128)   # tests/test_vae.py's, 128-d context


def make_ids(N, T, vocab, bos, eos, seed=0):
    """Rows that begin with BOS and are EOS from a different position on in each row."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, bos, (N, T), generator=g)      # below BOS and EOS: no EOS by chance
    ids[:, 0] = bos
    for n in range(N):
        ids[n, min(T - 1, 3 + 7 * n):] = eos
    assert ids.max() < vocab
    return ids


def load_theirs(ours, theirs):
    """transformers names its parameters as the SD checkpoint does, without the text_model. prefix
    (5.x); strict loading pins every name and shape."""
    sd = {k if k.startswith("text_model.") else "text_model." + k: v for k, v in theirs.state_dict().items()}
    ours.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("shape,N,T", [(SMALL, 3, 77), (SMALL, 3, 33), (None, 2, 77)],
                         ids=["small-77", "small-33", "sd-77"])
def test_parity_with_transformers(shape, N, T):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    if shape is None:      # the SD-v1.4 shape, the library's own defaults but the activation
        cfg = transformers.CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072,
                                          num_hidden_layers=12, num_attention_heads=12, max_position_embeddings=77,
                                          hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407,
                                          bos_token_id=49406, pad_token_id=49407)
        ours = te.CLIPTextModel().eval()
        vocab, bos, eos = 49408, 49406, 49407
    else:
        cfg = transformers.CLIPTextConfig(vocab_size=shape["vocab_size"], hidden_size=shape["hidden_size"],
                                          intermediate_size=shape["intermediate_size"],
                                          num_hidden_layers=shape["num_hidden_layers"],
                                          num_attention_heads=shape["num_attention_heads"], max_position_embeddings=77,
                                          hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                          eos_token_id=shape["eos_token_id"], bos_token_id=BOS,
                                          pad_token_id=shape["eos_token_id"])
        ours = te.CLIPTextModel(**shape).eval()
        vocab, bos, eos = shape["vocab_size"], BOS, shape["eos_token_id"]
    theirs = transformers.CLIPTextModel(cfg).eval()
    load_theirs(ours, theirs)
    ids = make_ids(N, T, vocab, bos, eos)
    with torch.no_grad():
        want = theirs(input_ids=ids)
        got = ours(ids)
    assert got[0] is got.last_hidden_state and got[0].shape == (N, T, cfg.hidden_size)
    for name, a, b in (("last_hidden_state", got[0], want.last_hidden_state),
                       ("pooler_output", got.pooler_output, want.pooler_output)):
        err, ref = (a - b).abs().max().item(), b.abs().max().item()
        print(f"{name}: max |ours - theirs| = {err:.3e}, max |theirs| = {ref:.3f}")
        assert a.shape == b.shape and err <= 1e-5 * ref, (name, err, ref)
    # the pooled row is the first EOS's
    first_eos = (ids == eos).int().argmax(-1)
    assert torch.equal(got.pooler_output, got[0][torch.arange(N), first_eos])


def test_causality():
    m = te.CLIPTextModel(**SMALL, generator=torch.Generator().manual_seed(3)).eval()
    ids = make_ids(2, 40, 1000, BOS, 999, seed=1)
    with torch.no_grad():
        base = m(ids)[0]
        for j in (0, 5, 38):
            other = ids.clone()
            other[:, j + 1:] = (other[:, j + 1:] + 17) % 900
            out = m(other)[0]
            assert torch.equal(out[:, :j + 1], base[:, :j + 1]), j
            assert not torch.equal(out[:, j + 1], base[:, j + 1]), j      # the negative control: the mask is not a wall


def expected_keys(layers):
    keys = ["text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight"]
    for i in range(layers):
        p = f"text_model.encoder.layers.{i}."
        for mod in ("self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj", "layer_norm1",
                    "mlp.fc1", "mlp.fc2", "layer_norm2"):
            keys += [p + mod + ".weight", p + mod + ".bias"]
    return keys + ["text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias"]


def test_default_names_and_shapes():
    """On the meta device: nothing is allocated."""
    with torch.device("meta"):
        m = te.CLIPTextModel()
    sd = m.state_dict()
    assert list(sd) == expected_keys(12)
    assert sd["text_model.embeddings.token_embedding.weight"].shape == (49408, 768)
    assert sd["text_model.embeddings.position_embedding.weight"].shape == (77, 768)
    assert sd["text_model.encoder.layers.3.self_attn.q_proj.bias"].shape == (768,)
    assert sd["text_model.encoder.layers.11.self_attn.out_proj.weight"].shape == (768, 768)
    assert sd["text_model.encoder.layers.0.mlp.fc1.weight"].shape == (3072, 768)
    assert sd["text_model.encoder.layers.0.mlp.fc2.weight"].shape == (768, 3072)
    assert sd["text_model.final_layer_norm.weight"].shape == (768,)
    att = m.text_model.encoder.layers[0].self_attn
    assert att.num_heads == 12 and att.head_dim == 64 and att.scale == 64 ** -0.5
    assert m.text_model.eos_token_id == 49407 and m.text_model.final_layer_norm.eps == 1e-5
    assert sum(p.numel() for p in m.parameters()) == 123_060_480     # the SD-v1.4 text encoder's parameter count


def test_generator_init_is_seeded_and_leaves_the_global_generator():
    torch.manual_seed(5)
    before = torch.get_rng_state()
    a = te.CLIPTextModel(**SMALL, generator=torch.Generator().manual_seed(7))
    assert torch.equal(torch.get_rng_state(), before)
    b = te.CLIPTextModel(**SMALL, generator=torch.Generator().manual_seed(7))
    c = te.CLIPTextModel(**SMALL, generator=torch.Generator().manual_seed(8))
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not torch.equal(sa["text_model.encoder.layers.0.mlp.fc1.bias"], sc["text_model.encoder.layers.0.mlp.fc1.bias"])


# ------------------------------------------------------------------ the pipeline
def test_pipeline_default_keeps_the_stub_and_the_seeded_weights_stay():
    from test_vae import NARROW_VAE
    narrow = dict(block_out_channels=(32, 64, 64, 64))
    plain = pl.SyntheticStableDiffusion(device="cpu", unet_config=narrow, vae_config=NARROW_VAE)
    assert type(plain.text_encoder) is pl.SyntheticTextEncoder
    clip = pl.SyntheticStableDiffusion(device="cpu", unet_config=narrow, vae_config=NARROW_VAE,
                                       text_encoder_config=SMALL_FULL_VOCAB)
    assert isinstance(clip.text_encoder, te.CLIPTextModel) and not clip.text_encoder.training
    assert not any(p.requires_grad for p in clip.text_encoder.parameters())
    for a, b in ((plain.unet.state_dict(), clip.unet.state_dict()), (plain.vae.state_dict(), clip.vae.state_dict())):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    again = pl.SyntheticStableDiffusion(device="cpu", unet_config=narrow, text_encoder_config=SMALL_FULL_VOCAB)
    a, b = clip.text_encoder.state_dict(), again.text_encoder.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)      # its own seeded generator: with or without the VAE


def test_pipeline_encoder_follows_the_unet_dtype():
    m = pl.SyntheticStableDiffusion(device="cpu", dtype=torch.bfloat16, unet_config=NARROW_UNET,
                                    text_encoder_config=SMALL_FULL_VOCAB)
    assert m.text_encoder.dtype == torch.bfloat16 and m.unet.dtype == torch.bfloat16


def test_pipeline_context_on_cpu():
    """The sampling loop needs the GPU kernels (there is no CPU path in the product: every attention
    of the U-Net is a HIP launch), so text2image_ldm_stable itself runs in tests/test_gpu_text.py;
    what it does with the encoder -- ptp_utils._encode and unet_context -- is checked here."""
    m = pl.SyntheticStableDiffusion(device="cpu", unet_config=NARROW_UNET, text_encoder_config=SMALL_FULL_VOCAB)
    prompts = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger"]
    with torch.no_grad():
        text = ptp_utils._encode(m, prompts, m.text_encoder)
        uncond = ptp_utils._encode(m, [""] * 2, m.text_encoder)
        ctx = ptp_utils.unet_context(m, torch.cat([uncond, text]))
    assert ctx.shape == (4, 77, 128) and ctx.dtype == m.unet.dtype and torch.isfinite(ctx).all()
    assert torch.allclose(ctx[0], ctx[1], rtol=0, atol=1e-5)          # equal prompts, equal rows
    swap = m.tokenizer.encode(prompts[0]).index(m.tokenizer.encode("squirrel")[1])
    assert torch.allclose(text[0, :swap], text[1, :swap], rtol=0, atol=1e-5)
    assert all((text[0, t] - text[1, t]).abs().max() > 1e-3 for t in range(swap, 77))
    # bit for bit, one prompt per call (the CPU GEMMs round rows of different batch entries
    # differently; the GPU test compares the rows of one batch)
    with torch.no_grad():
        a, b = (ptp_utils._encode(m, [p], m.text_encoder)[0] for p in prompts)
    assert torch.equal(a[:swap], b[:swap])                   # rows before the swapped word
    assert all(not torch.equal(a[t], b[t]) for t in range(swap, 77))


# ------------------------------------------------------------------ C ABI, no GPU
def _causal(**kw):
    base = dict(io_dtype=1, n_batch=2, n_query=77, n_key=77, n_heads=12, head_dim=64, scale=0.125,
                q_row_stride=2304, k_row_stride=2304, v_row_stride=2304, o_row_stride=768,
                q_batch_stride=2304 * 77, k_batch_stride=2304 * 77, v_batch_stride=2304 * 77, o_batch_stride=768 * 77)
    base.update(kw)
    return _tensors(**base)


@pytest.mark.parametrize("kw,code", [
    (dict(io_dtype=0), -3),                      # f32 inputs
    (dict(compute=1), -3),                       # the exact-f32 check mode
    (dict(n_query=97, n_key=97), -4),            # more tokens than P2P_MAX_KEYS_CROSS
    (dict(n_query=64), -1),                      # n_query != n_key
    (dict(head_dim=40), -2),
    (dict(q_row_stride=324), -6),                # 648 bytes: off 16
    (dict(v=24), -6),
    (dict(o=None), -1),
])
def test_causal_attn_rejects(kw, code):
    t = _causal(**kw)
    assert _hip.lib().p2p_causal_attn_fwd(ctypes.byref(t), None) == code


def _ln(**kw):
    a = _hip.LayerNormArgs()
    a.x, a.gamma, a.beta, a.y = 64, 128, 256, 512
    a.rows, a.channels, a.eps, a.dtype = 77, 768, 1e-5, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _act(**kw):
    a = _hip.BiasActArgs()
    a.inp, a.bias, a.out = 64, 128, 64
    a.in_row_stride = a.out_row_stride = 3072
    a.rows, a.d, a.dtype = 154, 3072, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(dtype=0), -3), (dict(channels=100), -6), (dict(x=None), -1), (dict(y=None), -1), (dict(gamma=None), -1),
    (dict(add=8), -6), (dict(channels=2056), -1), (dict(rows=0), -1),
])
def test_layer_norm_rejects(kw, code):
    L = _hip.lib()
    assert L.p2p_layer_norm(ctypes.byref(_ln(**kw)), None) == code
    assert L.p2p_layer_norm(None, None) == -1


@pytest.mark.parametrize("kw,code", [
    (dict(dtype=0), -3), (dict(d=100, in_row_stride=104, out_row_stride=104), -6), (dict(inp=None), -1),
    (dict(bias=None), -1), (dict(out=None), -1), (dict(in_row_stride=3076), -6), (dict(in_row_stride=1024), -1),
])
def test_bias_quick_gelu_rejects(kw, code):
    L = _hip.lib()
    assert L.p2p_bias_quick_gelu(ctypes.byref(_act(**kw)), None) == code
    assert L.p2p_bias_quick_gelu(None, None) == -1


def test_abi_is_still_16():
    assert _hip.lib().p2p_abi_version() == 16 == _hip.ABI_VERSION
    for fn in ("p2p_causal_attn_fwd", "p2p_layer_norm", "p2p_bias_quick_gelu"):
        assert fn in _hip.EXPORTED_SYMBOLS


def test_bindings_return_none_off_the_gpu():
    x = torch.randn(4, 128).bfloat16()
    w = torch.ones(128).bfloat16()
    assert _hip.layer_norm(x, w, w, 1e-5) is None
    assert _hip.bias_quick_gelu(x, w) is None
    q = torch.randn(1, 8, 64).bfloat16()
    assert _hip.causal_attn(q, q, q, 1, 0.125) is None
