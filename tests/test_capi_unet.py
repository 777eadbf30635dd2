"""The U-Net glue entry points (p2p_group_norm, p2p_bias_residual, p2p_geglu) reject bad arguments
before launching anything, the fused-path predicate is off wherever today's torch lines must run,
and on the CPU in f32 the modules still compute today's formulas bit for bit."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

from p2p_amd import _hip, unet

E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32


def _gn(**kw):
    a = _hip.GroupNormArgs()
    a.x, a.gamma, a.beta, a.y, a.stats = 4096, 8192, 8208, 16384, 32768
    a.n, a.channels, a.hw, a.groups = 2, 64, 64, 32
    a.eps, a.act, a.y_layout, a.dtype = 1e-5, _hip.ACT_SILU, _hip.LAYOUT_NCHW, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), E_ARG), (dict(gamma=None), E_ARG), (dict(beta=None), E_ARG), (dict(y=None), E_ARG),
    (dict(stats=None), E_ARG),
    (dict(groups=24), E_ARG),                       # 64 % 24 != 0
    (dict(groups=0), E_ARG),
    (dict(chan_add=64, chan_add_stride=32), E_ARG),  # neither [C] (0) nor [N, C] (channels)
    (dict(act=2), E_ARG),
    (dict(y_layout=2), E_ARG),                      # unsupported layout
    (dict(dtype=F32), E_DTYPE), (dict(dtype=9), E_DTYPE),
    (dict(hw=60), E_ALIGN),                         # pixel vectors of 8
    (dict(channels=36, groups=4, y_layout=_hip.LAYOUT_TOKENS), E_ALIGN),   # channel vectors of 8
    (dict(x=4104), E_ALIGN), (dict(y=16392), E_ALIGN), (dict(stats=32770), E_ALIGN),
])
def test_group_norm_rejects(kw, code):
    assert _hip.lib().p2p_group_norm(ctypes.byref(_gn(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_group_norm(ctypes.byref(_gn(dtype=F16, **kw)), None) == code


def _br(**kw):
    a = _hip.BiasResidualArgs()
    a.a, a.b, a.out = 4096, 8192, 16384
    a.n, a.channels, a.hw, a.b_layout, a.dtype = 2, 64, 64, _hip.LAYOUT_NCHW, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(a=None), E_ARG), (dict(b=None), E_ARG), (dict(out=None), E_ARG), (dict(n=0), E_ARG),
    (dict(b_layout=5), E_ARG),
    (dict(dtype=F32), E_DTYPE),
    (dict(hw=12), E_ALIGN), (dict(channels=36, b_layout=_hip.LAYOUT_TOKENS), E_ALIGN),
    (dict(a=4100), E_ALIGN), (dict(b=8200), E_ALIGN), (dict(out=16386), E_ALIGN),
])
def test_bias_residual_rejects(kw, code):
    assert _hip.lib().p2p_bias_residual(ctypes.byref(_br(**kw)), None) == code


def _gg(**kw):
    a = _hip.GegluArgs()
    a.inp, a.out = 4096, 1 << 20
    a.in_row_stride, a.out_row_stride, a.rows, a.d, a.dtype = 2560, 1280, 64, 1280, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(inp=None), E_ARG), (dict(out=None), E_ARG), (dict(rows=0), E_ARG),
    (dict(in_row_stride=2552), E_ARG),              # rows overlap: stride below 2 d
    (dict(dtype=F32), E_DTYPE),
    (dict(d=1276, in_row_stride=2560), E_ALIGN), (dict(in_row_stride=2564), E_ALIGN),
    (dict(out_row_stride=1284), E_ALIGN), (dict(inp=4098), E_ALIGN), (dict(out=(1 << 20) + 8), E_ALIGN),
])
def test_geglu_rejects(kw, code):
    assert _hip.lib().p2p_geglu(ctypes.byref(_gg(**kw)), None) == code


def test_null_args_rejected():
    L = _hip.lib()
    assert L.p2p_group_norm(None, None) == E_ARG
    assert L.p2p_bias_residual(None, None) == E_ARG
    assert L.p2p_geglu(None, None) == E_ARG


class _FakeGpu:
    """What the predicate looks at, for a machine without a GPU."""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype


def test_predicate():
    bf, hf, f32 = _FakeGpu(torch.bfloat16), _FakeGpu(torch.float16), _FakeGpu(torch.float32)
    with torch.no_grad():
        assert unet.FUSE_UNET and unet.fused_glue(bf) and unet.fused_glue(hf, hf)
        assert not unet.fused_glue(torch.zeros(2, dtype=torch.bfloat16))      # a CPU tensor
        assert not unet.fused_glue(bf, torch.zeros(2, dtype=torch.bfloat16))
        assert not unet.fused_glue(f32) and not unet.fused_glue(bf, f32)
        with torch.enable_grad():
            assert not unet.fused_glue(bf)
    with torch.enable_grad():
        assert not unet.fused_glue(bf)


def test_switch_is_read_from_the_environment():
    code = ("import torch; from p2p_amd import unet\n"
            "class T: is_cuda = True; dtype = torch.bfloat16\n"
            "with torch.no_grad(): print(unet.FUSE_UNET, unet.fused_glue(T()))")
    env = dict(os.environ, P2P_FUSE_UNET="0", PYTHONPATH=PKG)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["False", "False"]


def test_modules_keep_todays_formulas_on_cpu():
    torch.manual_seed(0)
    with torch.no_grad():
        x, temb = torch.randn(2, 64, 8, 8), torch.randn(2, 64)
        for cout in (128, 64):
            m = unet.ResnetBlock2D(64, cout, temb_ch=64)
            h = m.conv1(F.silu(m.norm1(x)))
            h = h + m.time_emb_proj(F.silu(temb))[:, :, None, None]
            h = m.conv2(F.silu(m.norm2(h)))
            want = (m.conv_shortcut(x) if m.conv_shortcut is not None else x) + h
            assert torch.equal(m(x, temb), want)

        g = unet.GEGLU(64, 128)
        t = torch.randn(2, 16, 64)
        a, gate = g.proj(t).chunk(2, dim=-1)
        assert torch.equal(g(t), a * F.gelu(gate))

        tr = unet.Transformer2DModel(8, 8, 64, context_dim=32)
        ident = lambda y, context=None: y          # noqa: E731  (the unpatched attention is GPU-only)
        blk = tr.transformer_blocks[0]
        blk.attn1.forward = blk.attn2.forward = ident
        ctx = torch.randn(2, 5, 32)
        y = tr.proj_in(tr.norm(x)).permute(0, 2, 3, 1).reshape(2, 64, 64)
        y = blk.norm1(y) + y
        y = blk.norm2(y) + y
        y = blk.ff(blk.norm3(y)) + y
        want = tr.proj_out(y.reshape(2, 8, 8, 64).permute(0, 3, 1, 2)) + x
        assert torch.equal(tr(x, encoder_hidden_states=ctx), want)
