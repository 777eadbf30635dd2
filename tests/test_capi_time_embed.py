"""The time-path entry points (p2p_time_embed, p2p_time_proj) reject bad arguments before launching
anything, are declared and exported, and the U-Net's fused time path is off wherever today's torch
lines must run: on the CPU in f32 the model computes today's formulas bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, unet
from test_capi import declared_functions

E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32


def _te(**kw):
    a = _hip.TimeEmbedArgs()
    a.timesteps, a.timestep_stride = 4096, 1
    a.w1, a.b1, a.w2, a.b2, a.workspace, a.emb = 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21
    a.n, a.in_channels, a.d, a.dtype = 8, 320, 1280, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(timesteps=None), E_ARG), (dict(w1=None), E_ARG), (dict(b1=None), E_ARG), (dict(w2=None), E_ARG),
    (dict(b2=None), E_ARG), (dict(workspace=None), E_ARG), (dict(emb=None), E_ARG),
    (dict(n=0), E_ARG), (dict(n=65), E_ARG), (dict(d=0), E_ARG), (dict(d=2056), E_ARG), (dict(in_channels=0), E_ARG),
    (dict(timestep_stride=2), E_ARG),
    (dict(dtype=F32), E_DTYPE), (dict(dtype=9), E_DTYPE),
    (dict(d=1284), E_ALIGN), (dict(in_channels=324), E_ALIGN),
    (dict(w1=(1 << 16) + 8), E_ALIGN), (dict(w2=(1 << 18) + 2), E_ALIGN), (dict(workspace=(1 << 20) + 4), E_ALIGN),
    (dict(emb=(1 << 21) + 8), E_ALIGN), (dict(timesteps=4100), E_ALIGN), (dict(b1=(1 << 17) + 1), E_ALIGN),
])
def test_time_embed_rejects(kw, code):
    assert _hip.lib().p2p_time_embed(ctypes.byref(_te(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_time_embed(ctypes.byref(_te(dtype=F16, **kw)), None) == code


def _tp(**kw):
    a = _hip.TimeProjArgs()
    a.emb, a.table, a.out = 1 << 16, 1 << 17, 1 << 18
    a.n, a.d, a.segments, a.tiles, a.dtype = 8, 1280, 22, 1260, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(emb=None), E_ARG), (dict(table=None), E_ARG), (dict(out=None), E_ARG),
    (dict(n=0), E_ARG), (dict(n=65), E_ARG), (dict(d=0), E_ARG), (dict(d=2056), E_ARG),
    (dict(segments=0), E_ARG), (dict(tiles=0), E_ARG),
    (dict(dtype=F32), E_DTYPE),
    (dict(d=1284), E_ALIGN), (dict(emb=(1 << 16) + 8), E_ALIGN), (dict(table=(1 << 17) + 4), E_ALIGN),
    (dict(out=(1 << 18) + 1), E_ALIGN),
])
def test_time_proj_rejects(kw, code):
    assert _hip.lib().p2p_time_proj(ctypes.byref(_tp(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_time_proj(ctypes.byref(_tp(dtype=F16, **kw)), None) == code


def test_null_args_and_exports():
    L = _hip.lib()
    assert L.p2p_time_embed(None, None) == E_ARG
    assert L.p2p_time_proj(None, None) == E_ARG
    declared = declared_functions()
    for fn in ("p2p_time_embed", "p2p_time_proj"):
        assert fn in declared and fn in _hip.EXPORTED_SYMBOLS and hasattr(L, fn)
    assert _hip.ABI_VERSION == 16 == L.p2p_abi_version()


def test_binding_returns_none_for_the_cpu():
    t = torch.tensor([3], dtype=torch.int64)
    w = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)   # noqa: E731
    assert _hip.time_embed(t, w(128, 32), w(128), w(128, 128), w(128)) is None
    table = _hip.TimeProjTable([(w(64, 128), w(64))])
    assert not table.supported and table.table is None
    assert _hip.time_proj(w(1, 128), table) is None


def test_model_keeps_todays_formulas_on_cpu():
    """f32 on the CPU: the time path is the torch lines, and a resnet handed the plain emb computes
    its own projection."""
    torch.manual_seed(0)
    m = unet.UNet2DConditionModel(block_out_channels=(32, 64), layers_per_block=1, heads=2, cross_attention_dim=32)
    m.eval()
    seen = []
    for r in (mod for mod in m.modules() if isinstance(mod, unet.ResnetBlock2D)):
        r.register_forward_pre_hook(lambda mod, args: seen.append(args[1]))
    ident = lambda y, context=None: y          # noqa: E731  (the unpatched attention is GPU-only)
    for b in (mod for mod in m.modules() if isinstance(mod, unet.BasicTransformerBlock)):
        b.attn1.forward = b.attn2.forward = ident
    with torch.no_grad():
        t = torch.tensor([7, 431])
        m(torch.randn(2, 4, 8, 8), t, torch.randn(2, 5, 32))
        want = m.time_embedding(unet.timestep_embedding(t, 32))
    assert len(seen) == len(m._time_linears) > 0 and m._time_proj_table is None
    assert all(torch.is_tensor(e) and torch.equal(e, want) for e in seen)
    # a block handed a TimeProjections takes its own slice and the plain emb beside it
    r = unet.ResnetBlock2D(32, 64, temb_ch=16).eval()
    x, temb = torch.randn(2, 32, 8, 8), torch.randn(2, 16)
    with torch.no_grad():
        proj = r.time_emb_proj(F.silu(temb))
        assert torch.equal(r(x, unet.TimeProjections(temb, {r.time_emb_proj: proj})), r(x, temb))
