"""The LDMBert text encoder (p2p_amd/ldm_bert.py) as far as a CPU can check: its parameter names and
shapes, bidirectional mixing, the padding mask, the pipeline switches, and the argument checks of
the two new entry points (no launch)."""
import ctypes

import pytest
import torch

from p2p_amd import _hip
from p2p_amd import ldm_bert as lb
from p2p_amd import pipeline as pl

from test_capi import HEADER, _tensors, declared_functions
from test_vae import NARROW_VAE

SMALL = dict(vocab_size=1000, d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=512)
# the pipeline's tokenizer hands out ids up to 49407: the small shape on the pipeline's own vocabulary
SMALL_PIPE = {k: v for k, v in SMALL.items() if k != "vocab_size"}
NARROW_UNET = dict(block_out_channels=(32, 64, 64, 64), cross_attention_dim=128)   # tests/test_vae.py's, 128-d context


def make_ids(N, T, seed=0):
    return torch.randint(0, 900, (N, T), generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ shape and names
def expected_keys(layers):
    keys = ["model.embed_tokens.weight", "model.embed_positions.weight"]
    for i in range(layers):
        p = f"model.layers.{i}."
        keys += [p + f"self_attn.{m}_proj.weight" for m in ("k", "v", "q")]
        for mod in ("self_attn.out_proj", "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"):
            keys += [p + mod + ".weight", p + mod + ".bias"]
    return keys + ["model.layer_norm.weight", "model.layer_norm.bias", "to_logits.weight", "to_logits.bias"]


def test_default_names_and_shapes():
    """On the meta device: nothing is allocated."""
    with torch.device("meta"):
        m = lb.LDMBertModel()
    sd = m.state_dict()
    assert sorted(sd) == sorted(expected_keys(32))
    assert sd["model.embed_tokens.weight"].shape == (30522, 1280)
    assert sd["model.embed_positions.weight"].shape == (77, 1280)
    assert sd["model.layers.3.self_attn.q_proj.weight"].shape == (512, 1280)
    assert "model.layers.3.self_attn.q_proj.bias" not in sd
    assert sd["model.layers.31.self_attn.out_proj.weight"].shape == (1280, 512)
    assert sd["model.layers.31.self_attn.out_proj.bias"].shape == (1280,)
    assert sd["model.layers.0.fc1.weight"].shape == (5120, 1280)
    assert sd["model.layers.0.fc2.weight"].shape == (1280, 5120)
    assert sd["to_logits.weight"].shape == (30522, 1280)
    att = m.model.layers[0].self_attn
    assert att.num_heads == 8 and att.head_dim == 64 and att.scale == 64 ** -0.5
    assert m.model.layer_norm.eps == 1e-5 and m.model.layers[0].final_layer_norm.eps == 1e-5
    V, C, A, Fd, T, Ly = 30522, 1280, 8 * 64, 5120, 77, 32
    layer = 3 * A * C + (A * C + C) + 2 * 2 * C + (C * Fd + Fd) + (Fd * C + C)
    count = V * C + T * C + Ly * layer + 2 * C + (C * V + V)
    assert sum(p.numel() for p in m.parameters()) == count


def test_generator_init_is_seeded_and_leaves_the_global_generator():
    torch.manual_seed(5)
    before = torch.get_rng_state()
    a = lb.LDMBertModel(**SMALL, generator=torch.Generator().manual_seed(7))
    assert torch.equal(torch.get_rng_state(), before)
    b = lb.LDMBertModel(**SMALL, generator=torch.Generator().manual_seed(7))
    c = lb.LDMBertModel(**SMALL, generator=torch.Generator().manual_seed(8))
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not torch.equal(sa["model.layers.0.fc1.bias"], sc["model.layers.0.fc1.bias"])


# ------------------------------------------------------------------ mixing and padding
def test_every_row_sees_every_token():
    """The opposite of test_text_encoder.py's causal check: a changed token at position j changes
    every row, the ones before j included."""
    m = lb.LDMBertModel(**SMALL, generator=torch.Generator().manual_seed(3)).eval()
    ids = make_ids(2, 40, seed=1)
    with torch.no_grad():
        out = m(ids)
        assert isinstance(out, tuple) and out[0].shape == (2, 40, 128)
        base = out[0]
        for j in (0, 5, 39):
            other = ids.clone()
            other[:, j] = (other[:, j] + 17) % 900
            got = m(other)[0]
            assert all(not torch.equal(got[:, t], base[:, t]) for t in range(40)), j


def test_padding_mask():
    m = lb.LDMBertModel(**SMALL, generator=torch.Generator().manual_seed(4)).eval()
    N, T = 3, 33
    ids = make_ids(N, T, seed=2)
    lengths = [5, 33, 17]
    mask = torch.zeros(N, T, dtype=torch.int64)
    other = ids.clone()
    for n, L in enumerate(lengths):
        mask[n, :L] = 1
        other[n, L:] = (other[n, L:] + 17) % 900
    with torch.no_grad():
        a, b = m(ids, attention_mask=mask)[0], m(other, attention_mask=mask)[0]
        unmasked = m(other)[0]
        plain = m(ids)[0]
        for n, L in enumerate(lengths):
            # the rows of the kept tokens do not see what stands behind them
            err = (a[n, :L] - b[n, :L]).abs().max().item()
            assert err <= 1e-5, (n, L, err)
            if L < T:      # the negative controls: without the mask they do, and the mask is not a no-op
                assert (plain[n, :L] - unmasked[n, :L]).abs().max().item() > 1e-3
                assert (plain[n, :L] - a[n, :L]).abs().max().item() > 1e-3
        assert torch.equal(m(ids, attention_mask=torch.ones(N, T, dtype=torch.int64))[0], plain)
        # a mask with holes is a mask too (torch lines): the hidden key's token does not matter
        holes = torch.ones(N, T, dtype=torch.int64)
        holes[:, 7] = 0
        swapped = ids.clone()
        swapped[:, 7] = (swapped[:, 7] + 17) % 900
        c, d = m(ids, attention_mask=holes)[0], m(swapped, attention_mask=holes)[0]
        keep = [t for t in range(T) if t != 7]
        assert (c[:, keep] - d[:, keep]).abs().max().item() <= 1e-5
    with pytest.raises(ValueError):
        m(ids, attention_mask=torch.zeros(N, T, dtype=torch.int64))


def test_prefix_masks_become_counts():
    keys = lb.LDMBertEncoder._keys
    ids = make_ids(2, 6)
    assert keys(None, ids) == (None, None)
    km, counts = keys(torch.tensor([[1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1]]), ids)
    assert km.dtype == torch.bool and counts.dtype == torch.int32 and counts.tolist() == [3, 6]
    km, counts = keys(torch.tensor([[1, 0, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1]]), ids)
    assert km.tolist()[0] == [True, False, True, False, False, False] and counts is None


# ------------------------------------------------------------------ the pipeline
def test_pipeline_defaults_stay_and_the_new_parts_move_no_unet_weight():
    narrow = dict(block_out_channels=(32, 64, 64, 64), cross_attention_dim=128)
    plain = pl.SyntheticLatentDiffusion(device="cpu", unet_config=narrow)
    assert type(plain.bert) is pl.SyntheticTextEncoder and plain.vqvae is None
    full = pl.SyntheticLatentDiffusion(device="cpu", unet_config=narrow, bert_config=SMALL_PIPE, vqvae_config=NARROW_VAE)
    assert isinstance(full.bert, lb.LDMBertModel) and not full.bert.training
    assert full.bert.model.embed_tokens.num_embeddings == 49408      # the stand-in tokenizer's ids
    assert not any(p.requires_grad for p in full.bert.parameters())
    from p2p_amd import vae
    assert isinstance(full.vqvae, vae.AutoencoderKL) and not full.vqvae.training
    a, b = plain.unet.state_dict(), full.unet.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(plain.bert.token, pl.SyntheticLatentDiffusion(device="cpu", unet_config=narrow,
                                                                     vqvae_config=NARROW_VAE).bert.token)
    # each from a generator of its own: the encoder with or without the VQ-VAE, and the other way round
    bert_only = pl.SyntheticLatentDiffusion(device="cpu", unet_config=narrow, bert_config=SMALL_PIPE)
    vq_only = pl.SyntheticLatentDiffusion(device="cpu", unet_config=narrow, vqvae_config=NARROW_VAE)
    for x, y in ((full.bert, bert_only.bert), (full.vqvae, vq_only.vqvae)):
        a, b = x.state_dict(), y.state_dict()
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_pipeline_default_unet_keeps_its_bits():
    """The LDM-256 U-Net itself (0.87 G parameters, some ten seconds a build): the same weights, bit
    for bit, with the defaults and beside a small encoder and VQ-VAE."""
    plain = pl.SyntheticLatentDiffusion(device="cpu")
    assert type(plain.bert) is pl.SyntheticTextEncoder and plain.bert.token.shape == (49408, 1280)
    assert plain.vqvae is None
    a = plain.unet.state_dict()
    b = pl.SyntheticLatentDiffusion(device="cpu", bert_config=dict(SMALL_PIPE, d_model=1280, encoder_layers=1),
                                    vqvae_config=NARROW_VAE).unet.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_pipeline_bert_true_and_dtype():
    m = pl.SyntheticLatentDiffusion(device="cpu", dtype=torch.bfloat16, unet_config=NARROW_UNET,
                                    bert_config=dict(SMALL_PIPE, encoder_layers=1), bert=True)
    assert isinstance(m.bert, lb.LDMBertModel) and m.bert.dtype == torch.bfloat16 == m.unet.dtype
    with torch.no_grad():
        from p2p_amd import ptp_utils
        ctx = ptp_utils._encode(m, pl.LDM_PROMPTS, m.bert)
    assert ctx.shape == (2, 77, 128) and torch.isfinite(ctx.float()).all()
    assert all(not torch.equal(ctx[0, t], ctx[1, t]) for t in range(77))     # a one-word edit moves every row


def test_pipeline_vqvae_decodes_latents_to_images():
    """What text2image_ldm does behind its sampling loop (which needs the GPU kernels): 32 x 32 latents
    through an f8 autoencoder are 256 x 256 uint8 images."""
    import numpy as np
    from p2p_amd import ptp_utils
    f8 = dict(block_out_channels=(32, 32, 64, 64), layers_per_block=1, norm_num_groups=8)
    m = pl.SyntheticLatentDiffusion(device="cpu", unet_config=NARROW_UNET, vqvae_config=f8)
    with torch.no_grad():
        image = ptp_utils.latent2image(m.vqvae, pl.ldm_seed_latent(0).expand(2, 4, 32, 32))
    assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (2, 256, 256, 3)


# ------------------------------------------------------------------ C ABI, no GPU
def test_new_symbols_are_declared_and_exported():
    L = _hip.lib()
    assert L.p2p_abi_version() == 16 == _hip.ABI_VERSION
    declared = declared_functions()
    for fn in ("p2p_text_attn_fwd", "p2p_bias_gelu"):
        assert fn in declared and fn in _hip.EXPORTED_SYMBOLS and hasattr(L, fn)
    text = open(HEADER).read()
    assert "clamps" in text[text.index("Bidirectional self-attention"):text.index("int p2p_text_attn_fwd")]


def _text(**kw):
    base = dict(io_dtype=1, n_batch=2, n_query=77, n_key=77, n_heads=8, head_dim=64, scale=0.125,
                q_row_stride=1536, k_row_stride=1536, v_row_stride=1536, o_row_stride=512,
                q_batch_stride=1536 * 77, k_batch_stride=1536 * 77, v_batch_stride=1536 * 77, o_batch_stride=512 * 77)
    base.update(kw)
    return _tensors(**base)


@pytest.mark.parametrize("counts", [None, 64], ids=["no-counts", "counts"])
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
def test_text_attn_rejects(kw, code, counts):
    t = _text(**kw)
    assert _hip.lib().p2p_text_attn_fwd(ctypes.byref(t), counts, None) == code


def test_text_attn_rejects_misaligned_counts():
    assert _hip.lib().p2p_text_attn_fwd(ctypes.byref(_text()), 66, None) == -6
    assert _hip.lib().p2p_text_attn_fwd(None, None, None) == -1


def _act(**kw):
    a = _hip.BiasActArgs()
    a.inp, a.bias, a.out = 64, 128, 64
    a.in_row_stride = a.out_row_stride = 5120
    a.rows, a.d, a.dtype = 154, 5120, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(dtype=0), -3), (dict(d=100, in_row_stride=104, out_row_stride=104), -6), (dict(inp=None), -1),
    (dict(bias=None), -1), (dict(out=None), -1), (dict(in_row_stride=5124), -6), (dict(in_row_stride=1024), -1),
])
def test_bias_gelu_rejects(kw, code):
    L = _hip.lib()
    assert L.p2p_bias_gelu(ctypes.byref(_act(**kw)), None) == code
    assert L.p2p_bias_gelu(None, None) == -1


def test_bindings_return_none_off_the_gpu():
    x = torch.randn(4, 128).bfloat16()
    w = torch.ones(128).bfloat16()
    assert _hip.bias_gelu(x, w) is None
    q = torch.randn(1, 8, 64).bfloat16()
    assert _hip.text_attn(q, q, q, 1, 0.125) is None
