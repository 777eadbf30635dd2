"""The SD-shaped VAE (p2p_amd/vae.py) and what it brings with it, as far as a CPU can check: module
shapes, the ResnetBlock2D form without a time embedding (and that the default form did not move),
the pipeline's default, the image ends' torch lines, the selection of the d = 512 kernel through the
query entry points (no launch), and the new entry points' argument checks."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from p2p_amd import _hip, null_text, ptp_utils, unet, vae
from p2p_amd import pipeline as pl

NARROW_VAE = dict(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8)
NARROW_UNET = dict(block_out_channels=(32, 64, 64, 64))
WIDE = "self_wide_kernel<512,…>"


# ------------------------------------------------------------------ shapes
def test_narrow_vae_shapes():
    torch.manual_seed(0)
    m = vae.AutoencoderKL(**NARROW_VAE).eval()
    with torch.no_grad():
        dist = m.encode(torch.randn(1, 3, 32, 32))["latent_dist"]
        assert dist.mean.shape == (1, 4, 16, 16)
        assert dist.mode() is dist.mean
        g = torch.Generator().manual_seed(1)
        s = dist.sample(g)
        assert s.shape == dist.mean.shape and not torch.equal(s, dist.mean)
        assert dist.logvar.min() >= -30 and dist.logvar.max() <= 20
        img = m.decode(dist.mean)["sample"]
    assert img.shape == (1, 3, 32, 32)


def test_logvar_is_clamped():
    moments = torch.cat([torch.zeros(1, 4, 2, 2), torch.tensor([-100.0, 100.0, 0.0, 1.0]).reshape(1, 4, 1, 1).expand(1, 4, 2, 2)], 1)
    d = vae.DiagonalGaussianDistribution(moments)
    assert d.logvar.min().item() == -30.0 and d.logvar.max().item() == 20.0


def test_default_vae_is_sd_shaped():
    """On the meta device: nothing is allocated, shapes still propagate."""
    with torch.device("meta"):
        m = vae.AutoencoderKL()
        x = torch.empty(1, 3, 512, 512)
    m.eval()
    with torch.no_grad():
        h = m.encoder.conv_in(x)            # the encoder trunk in front of the mid block (shapes only)
        for blk in m.encoder.down_blocks:
            h = blk(h)
    assert h.shape == (1, 512, 64, 64)                     # the latent of a 512^2 image is 64^2
    assert m.encoder.conv_out.out_channels == 8 and m.quant_conv.out_channels == 8
    assert m.post_quant_conv.in_channels == 4 and m.decoder.conv_in.in_channels == 4
    for mid in (m.encoder.mid_block, m.decoder.mid_block):
        att = mid.attentions[0]
        assert att.channels == 512 and att.query.in_features == 512 and att.query.bias is not None
        assert type(att).__name__ != "CrossAttention"
    assert [len(b.resnets) for b in m.encoder.down_blocks] == [2, 2, 2, 2]
    assert [len(b.resnets) for b in m.decoder.up_blocks] == [3, 3, 3, 3]
    assert [b.resnets[0].conv1.out_channels for b in m.decoder.up_blocks] == [512, 512, 256, 128]
    assert [b.downsamplers is not None for b in m.encoder.down_blocks] == [True, True, True, False]
    assert [b.upsamplers is not None for b in m.decoder.up_blocks] == [True, True, True, False]
    assert sum(p.numel() for p in m.parameters()) == 83_653_863   # the SD-v1.4 VAE's parameter count
    keys = set(m.state_dict())
    for k in ("encoder.down_blocks.0.resnets.0.conv1.weight", "encoder.down_blocks.1.resnets.0.conv_shortcut.bias",
              "encoder.down_blocks.0.downsamplers.0.conv.weight", "encoder.mid_block.attentions.0.group_norm.weight",
              "decoder.mid_block.attentions.0.proj_attn.bias", "decoder.up_blocks.0.upsamplers.0.conv.weight",
              "decoder.conv_norm_out.bias", "quant_conv.weight", "post_quant_conv.bias"):
        assert k in keys, k
    assert not any("time_emb_proj" in k for k in keys)


def test_vae_downsample_pads_bottom_right():
    d = vae.Downsample2D(4)
    x = torch.randn(1, 4, 8, 8)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), d.conv.weight, d.conv.bias, stride=2)
    assert d.conv.padding == (0, 0) and torch.equal(d(x), want) and want.shape == (1, 4, 4, 4)


# ------------------------------------------------------------------ ResnetBlock2D
def test_resnet_default_form_did_not_move():
    """The seeded construction of today's block, written out from plain layers in today's order."""
    torch.manual_seed(11)
    blk = unet.ResnetBlock2D(64, 128, temb_ch=64)
    torch.manual_seed(11)
    want = nn.ModuleDict()
    want["norm1"] = nn.GroupNorm(32, 64, eps=1e-5)
    want["conv1"] = nn.Conv2d(64, 128, 3, padding=1)
    want["time_emb_proj"] = nn.Linear(64, 128)
    want["norm2"] = nn.GroupNorm(32, 128, eps=1e-5)
    want["conv2"] = nn.Conv2d(128, 128, 3, padding=1)
    want["conv_shortcut"] = nn.Conv2d(64, 128, 1)
    got, ref = blk.state_dict(), want.state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), k
    # and the default argument is still the U-Net's 1280
    assert unet.ResnetBlock2D(32, 32).time_emb_proj.in_features == 1280
    x, temb = torch.randn(2, 64, 8, 8), torch.randn(2, 64)
    with torch.no_grad():
        h = want["conv1"](F.silu(want["norm1"](x))) + want["time_emb_proj"](F.silu(temb))[:, :, None, None]
        h = want["conv2"](F.silu(want["norm2"](h)))
        assert torch.equal(blk(x, temb), want["conv_shortcut"](x) + h)


def test_resnet_without_time_embedding():
    torch.manual_seed(12)
    blk = unet.ResnetBlock2D(64, 128, temb_ch=None, groups=8, eps=1e-6)
    assert not hasattr(blk, "time_emb_proj") and not any("time_emb" in k for k in blk.state_dict())
    assert blk.norm1.eps == 1e-6 and blk.norm2.num_groups == 8
    x = torch.randn(2, 64, 8, 8)
    with torch.no_grad():
        h = blk.conv1(F.silu(blk.norm1(x)))
        h = blk.conv2(F.silu(blk.norm2(h)))
        assert torch.equal(blk(x), blk.conv_shortcut(x) + h)
    same = unet.ResnetBlock2D(64, 64, temb_ch=None)
    with torch.no_grad():
        h = same.conv2(F.silu(same.norm2(same.conv1(F.silu(same.norm1(x))))))
        assert same.conv_shortcut is None and torch.equal(same(x), x + h)


def test_attention_block_torch_lines():
    """softmax(q k^T C^-1/2) v with biased projections, one head, residual -- written out."""
    torch.manual_seed(13)
    att = vae.AttentionBlock(64, groups=8).eval()
    x = torch.randn(2, 64, 4, 4)
    with torch.no_grad():
        t = att.group_norm(x).reshape(2, 64, 16).transpose(1, 2)
        q, k, v = att.query(t), att.key(t), att.value(t)
        # diffusers' form: q and k scaled by C^-1/4 each
        p = ((q * 64 ** -0.25) @ (k * 64 ** -0.25).transpose(1, 2)).softmax(-1)
        want = att.proj_attn(p @ v).transpose(1, 2).reshape(2, 64, 4, 4) + x
        got = att(x)
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()


# ------------------------------------------------------------------ the pipeline
def test_pipeline_default_has_no_vae_and_the_seeded_weights_stay():
    """(The sampling loop needs the GPU kernels -- there is no CPU path in the product -- so the
    image end of text2image_ldm_stable is checked here through latent2image on CPU tensors; the loop
    itself is in tests/test_gpu_vae.py.)"""
    plain = pl.SyntheticStableDiffusion(device="cpu", unet_config=NARROW_UNET)
    assert plain.vae is None
    with_vae = pl.SyntheticStableDiffusion(device="cpu", unet_config=NARROW_UNET, vae_config=NARROW_VAE)
    assert isinstance(with_vae.vae, vae.AutoencoderKL) and not with_vae.vae.training
    assert not any(p.requires_grad for p in with_vae.vae.parameters())
    a, b = plain.unet.state_dict(), with_vae.unet.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(plain.text_encoder.token, with_vae.text_encoder.token)
    lat = torch.randn(2, 4, 8, 8)
    img = ptp_utils.latent2image(with_vae.vae, lat)
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (2, 16, 16, 3)
    # a model without a VAE: the caller's guard keeps returning the latents
    assert getattr(plain, "vae", None) is None


def test_pipeline_vae_follows_the_unet_dtype():
    m = pl.SyntheticStableDiffusion(device="cpu", dtype=torch.bfloat16, unet_config=NARROW_UNET, vae_config=NARROW_VAE)
    assert m.vae.dtype == torch.bfloat16 and m.unet.dtype == torch.bfloat16


# ------------------------------------------------------------------ the image ends, torch lines
def test_latent2image_torch_lines_take_bf16():
    torch.manual_seed(3)
    m = vae.AutoencoderKL(**NARROW_VAE).to(torch.bfloat16).eval()
    lat = torch.randn(1, 4, 8, 8)
    with torch.no_grad():
        img = ptp_utils.latent2image(m, lat)
        dec = m.decode(1 / 0.18215 * lat)["sample"]
    assert dec.dtype == torch.bfloat16
    want = (((dec.float() / 2 + 0.5).clamp(0, 1)) * 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert img.dtype == np.uint8 and img.shape == (1, 16, 16, 3) and np.array_equal(img, want)


def test_image_to_model_torch_lines():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(6, 10, 3), dtype=np.uint8)
    img[0, 0] = (0, 255, 128)
    x = ptp_utils.image_to_model(img, "cpu", torch.float32)
    want = torch.from_numpy(img).float() / 127.5 - 1
    assert x.shape == (1, 3, 6, 10) and torch.equal(x[0], want.permute(2, 0, 1))
    assert x.min().item() == -1.0 and x.max().item() == 1.0
    xb = ptp_utils.image_to_model(img[None], "cpu", torch.bfloat16)
    assert xb.dtype == torch.bfloat16 and torch.equal(xb, x.to(torch.bfloat16))


def test_null_inversion_image2latent_on_cpu():
    model = pl.SyntheticStableDiffusion(device="cpu", unet_config=NARROW_UNET, vae_config=NARROW_VAE)
    inv = null_text.NullInversion(model, num_ddim_steps=3)
    img = np.random.default_rng(1).integers(0, 256, size=(16, 16, 3), dtype=np.uint8)
    lat = inv.image2latent(img)
    x = (torch.from_numpy(img).float() / 127.5 - 1).permute(2, 0, 1)[None].contiguous()
    with torch.no_grad():
        want = model.vae.encode(x)["latent_dist"].mean * 0.18215
    assert lat.shape == (1, 4, 8, 8) and torch.equal(lat, want)
    back = inv.latent2image(lat)
    assert back.dtype == np.uint8 and back.shape == (16, 16, 3)
    # the latent form still passes through, and a model without a VAE still says so
    assert inv.image2latent(lat) is not None
    with pytest.raises(ValueError):
        null_text.NullInversion(pl.SyntheticStableDiffusion(device="cpu", unet_config=NARROW_UNET), 3).image2latent(img)


# ------------------------------------------------------------------ selection (queries only)
def _tensors(dtype, compute=0, P=4096, K=None, d=512, heads=1, N=1):
    K = P if K is None else K
    t = _hip.AttnTensors()
    t.q = t.k = t.v = t.o = 16
    C = heads * d
    t.q_row_stride = t.k_row_stride = t.v_row_stride = t.o_row_stride = C
    t.q_batch_stride = t.o_batch_stride = C * P
    t.k_batch_stride = t.v_batch_stride = C * K
    t.n_batch, t.n_query, t.n_key, t.n_heads, t.head_dim = N, P, K, heads, d
    t.io_dtype, t.compute, t.scale = dtype, compute, d ** -0.5
    return t


@pytest.mark.parametrize("dtype", [_hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("P", [4096, 20])
def test_wide_kernel_is_selected_at_d512(dtype, P):
    t = _tensors(dtype, P=P)
    assert _hip.self_attn_kernel(t) == WIDE
    assert _hip.self_attn_kernel(_tensors(dtype, P=P, heads=2, N=2)) == WIDE
    assert _hip.self_attn_kernel(t, keeps_maps=True) is None
    assert _hip.self_attn_kernel(t, wants_lse=True) is None


def test_wide_kernel_is_the_only_d512_kernel():
    assert _hip.self_attn_kernel(_tensors(_hip.P2P_DTYPE_F32)) is None                 # f32 inputs, bf16 pipe
    assert _hip.self_attn_kernel(_tensors(_hip.P2P_DTYPE_F32, compute=1)) is None      # exact-f32 check mode
    assert _hip.self_attn_kernel(_tensors(_hip.P2P_DTYPE_BF16, d=256)) is None
    assert _hip.self_attn_kernel(_tensors(_hip.P2P_DTYPE_BF16, d=48)) is None
    assert _hip.self_attn_kernel(_tensors(_hip.P2P_DTYPE_BF16, d=44)) is None
    # a strided launch (q / k / v views of one [N, P, 3 * 512] tensor) selects the same kernel
    t = _tensors(_hip.P2P_DTYPE_BF16, P=200)
    t.q_row_stride = t.k_row_stride = t.v_row_stride = 1536
    t.q_batch_stride = t.k_batch_stride = t.v_batch_stride = 1536 * 200
    assert _hip.self_attn_kernel(t) == WIDE
    # cross at d = 512
    tc = _tensors(_hip.P2P_DTYPE_BF16, P=64, K=77)
    G = (_hip.Group * 1)()
    G[0].first, G[0].count = 0, 1
    assert _hip.cross_attn_kernel(tc, G) is None


def test_c_abi_refuses_everything_else_at_d512():
    L = _hip.lib()
    E_HEAD_DIM = -2
    for dtype in (_hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F32):
        t = _tensors(dtype, P=64)
        assert L.p2p_attn_fwd_lse(ctypes.byref(t), 16, None) == E_HEAD_DIM
        assert L.p2p_attn_bwd_workspace(ctypes.byref(t)) == E_HEAD_DIM
        assert L.p2p_attn_pv(ctypes.byref(t), 16, None) == E_HEAD_DIM
        assert L.p2p_attn_probs(ctypes.byref(t), None, 16, None) == E_HEAD_DIM
    G = (_hip.Group * 1)()
    G[0].first, G[0].count = 0, 1
    tc = _tensors(_hip.P2P_DTYPE_BF16, P=64, K=77)
    assert L.p2p_cross_attn_fwd(ctypes.byref(tc), G, 1, None, None, 0, None) == E_HEAD_DIM
    # f32 inputs through the forward entry point itself, and the check mode
    assert L.p2p_self_attn_fwd(ctypes.byref(_tensors(_hip.P2P_DTYPE_F32, P=64)), None, None, None, 0, None, None) == E_HEAD_DIM
    assert L.p2p_self_attn_fwd(ctypes.byref(_tensors(_hip.P2P_DTYPE_F32, compute=1, P=64)), None, None, None, 0, None,
                               None) == E_HEAD_DIM


# ------------------------------------------------------------------ the new entry points' checks
def _img_args(cls, **kw):
    a = cls()
    if cls is _hip.ImageU8Args:
        a.x, a.out = 16, 16
    else:
        a.img, a.out = 16, 16
    a.n, a.height, a.width, a.dtype = 1, 8, 8, _hip.P2P_DTYPE_BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("fn,cls,src", [("p2p_image_u8", _hip.ImageU8Args, "x"),
                                        ("p2p_image_to_model", _hip.ImageToModelArgs, "img")])
def test_image_entry_points_reject_before_any_launch(fn, cls, src):
    f = getattr(_hip.lib(), fn)
    E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
    assert f(None, None) == E_ARG
    assert f(ctypes.byref(_img_args(cls, **{src: None})), None) == E_ARG
    assert f(ctypes.byref(_img_args(cls, out=None)), None) == E_ARG
    assert f(ctypes.byref(_img_args(cls, n=0)), None) == E_ARG
    assert f(ctypes.byref(_img_args(cls, height=0)), None) == E_ARG
    assert f(ctypes.byref(_img_args(cls, width=-1)), None) == E_ARG
    for bad in (-1, 3, 99):
        assert f(ctypes.byref(_img_args(cls, dtype=bad)), None) == E_DTYPE
    # height * width % 4 != 0: refused as the header says (the callers then run their torch lines)
    assert f(ctypes.byref(_img_args(cls, height=3, width=3)), None) == E_ALIGN
    assert f(ctypes.byref(_img_args(cls, height=5, width=2)), None) == E_ALIGN


def test_group_norm_workspace_grows_only_above_the_unet_slabs():
    f = _hip.lib().p2p_group_norm_stats_floats
    assert f(2, 320, 4096, 32) == 2 * 32 * 2                  # a U-Net slab: {mean, rstd} only
    assert f(1, 960, 4096, 32) == 64                          # 30 x 4096 = 122,880: the U-Net's largest
    assert f(1, 960, 4096 + 8, 32) == 64                      # above it, below the split threshold
    assert f(1, 128, 65536 - 8, 32) == 64                     # 262,112: the last one-workgroup slab
    assert f(1, 128, 65536, 32) == 64 + 32 * 8 * 3            # 262,144: 8 chunks of {count, mean, M2}
    assert f(1, 128, 512 * 512, 32) == 64 + 32 * 32 * 3       # 1,048,576: 32 chunks
    assert f(0, 128, 64, 32) == -1 and f(1, 100, 64, 32) == -1
