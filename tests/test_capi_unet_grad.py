"""The backward entry points of the U-Net glue (p2p_group_norm_bwd, p2p_geglu_bwd,
p2p_nchw_to_tokens) are exported and declared and reject bad arguments before launching anything;
the autograd predicate ``unet.fused_glue_grad`` is off wherever the torch lines must run, and
``unet.fused_glue`` stays off under grad."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT

from p2p_amd import _hip, unet

E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32
NEW = ("p2p_group_norm_bwd", "p2p_group_norm_bwd_workspace_floats", "p2p_geglu_bwd", "p2p_nchw_to_tokens")


def test_symbols_exported_and_declared():
    text = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(p2p_\w+)\s*\(", text, flags=re.M))
    L = _hip.lib()
    for fn in NEW:
        assert fn in declared and fn in _hip.EXPORTED_SYMBOLS and hasattr(L, fn)
    assert L.p2p_abi_version() == 16


def _gn(**kw):
    a = _hip.GroupNormBwdArgs()
    a.x, a.gamma, a.beta, a.dy, a.stats, a.dx, a.workspace = 4096, 8192, 8208, 16384, 32768, 65536, 131072
    a.n, a.channels, a.hw, a.groups = 2, 64, 64, 32
    a.act, a.dy_layout, a.dtype = _hip.ACT_SILU, _hip.LAYOUT_NCHW, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), E_ARG), (dict(gamma=None), E_ARG), (dict(beta=None), E_ARG), (dict(dy=None), E_ARG),
    (dict(stats=None), E_ARG), (dict(dx=None), E_ARG), (dict(workspace=None), E_ARG),
    (dict(groups=24), E_ARG), (dict(groups=0), E_ARG), (dict(n=0), E_ARG),
    (dict(chan_add=64, chan_add_stride=32), E_ARG),
    (dict(act=2), E_ARG), (dict(dy_layout=2), E_ARG),
    (dict(channels=32, groups=1, hw=8192), E_ARG),          # a slab of 262,144 elements: the split statistics'
    (dict(channels=64, groups=1, hw=8192), E_ARG),          # and above
    (dict(dtype=F32), E_DTYPE), (dict(dtype=9), E_DTYPE),
    (dict(hw=60), E_ALIGN),
    (dict(channels=36, groups=4, dy_layout=_hip.LAYOUT_TOKENS), E_ALIGN),
    (dict(x=4104), E_ALIGN), (dict(dy=16392), E_ALIGN), (dict(dx=65544), E_ALIGN),
    (dict(stats=32770), E_ALIGN), (dict(workspace=131074), E_ALIGN),
])
def test_group_norm_bwd_rejects(kw, code):
    assert _hip.lib().p2p_group_norm_bwd(ctypes.byref(_gn(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_group_norm_bwd(ctypes.byref(_gn(dtype=F16, **kw)), None) == code


def test_group_norm_bwd_slab_limit_is_the_split_threshold():
    # 262,136 elements would be served (the arguments are otherwise bad on purpose: f32 comes after the size check)
    L = _hip.lib()
    assert L.p2p_group_norm_bwd(ctypes.byref(_gn(channels=32, groups=1, hw=8192 - 8, dtype=F32)), None) == E_DTYPE
    assert L.p2p_group_norm_bwd(ctypes.byref(_gn(channels=32, groups=1, hw=8192, dtype=F32)), None) == E_ARG
    assert unet.GN_SLAB_LIMIT == 262144


def test_workspace_floats():
    f = _hip.lib().p2p_group_norm_bwd_workspace_floats
    assert f(1, 320, 4096, 32) > 0 and f(2, 64, 64, 32) > 0
    assert f(2, 64, 64, 32) == f(2, 64, 64, 32)
    # it covers, per sample, two sums per channel and 64-pixel tile and two means per group, for either layout
    for n, c, hw, g in ((1, 320, 4096, 32), (3, 72, 24, 9), (2, 64, 64, 32)):
        assert f(n, c, hw, g) == n * (2 * c * -(-hw // 64) + 2 * g)
        assert f(n, c, hw, g) == n * f(1, c, hw, g)
    assert f(0, 64, 64, 32) == E_ARG and f(1, 64, 64, 24) == E_ARG and f(1, 64, 0, 32) == E_ARG


def _gg(**kw):
    a = _hip.GegluBwdArgs()
    a.inp, a.dout, a.din = 4096, 1 << 20, 1 << 22
    a.in_row_stride, a.rows, a.d, a.dtype = 2560, 64, 1280, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(inp=None), E_ARG), (dict(dout=None), E_ARG), (dict(din=None), E_ARG), (dict(rows=0), E_ARG),
    (dict(in_row_stride=2552), E_ARG),
    (dict(dtype=F32), E_DTYPE),
    (dict(d=1276, in_row_stride=2560), E_ALIGN), (dict(in_row_stride=2564), E_ALIGN),
    (dict(inp=4098), E_ALIGN), (dict(dout=(1 << 20) + 8), E_ALIGN), (dict(din=(1 << 22) + 2), E_ALIGN),
])
def test_geglu_bwd_rejects(kw, code):
    assert _hip.lib().p2p_geglu_bwd(ctypes.byref(_gg(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_geglu_bwd(ctypes.byref(_gg(dtype=F16, **kw)), None) == code


def _tt(**kw):
    a = _hip.NchwToTokensArgs()
    a.src, a.dst = 4096, 1 << 20
    a.n, a.channels, a.hw, a.dtype = 2, 64, 64, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(src=None), E_ARG), (dict(dst=None), E_ARG), (dict(n=0), E_ARG), (dict(channels=0), E_ARG),
    (dict(dtype=F32), E_DTYPE),
    (dict(hw=60), E_ALIGN), (dict(channels=36), E_ALIGN), (dict(src=4100), E_ALIGN), (dict(dst=(1 << 20) + 8), E_ALIGN),
])
def test_nchw_to_tokens_rejects(kw, code):
    assert _hip.lib().p2p_nchw_to_tokens(ctypes.byref(_tt(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_nchw_to_tokens(ctypes.byref(_tt(dtype=F16, **kw)), None) == code


def test_null_args_rejected():
    L = _hip.lib()
    assert L.p2p_group_norm_bwd(None, None) == E_ARG
    assert L.p2p_geglu_bwd(None, None) == E_ARG
    assert L.p2p_nchw_to_tokens(None, None) == E_ARG


class _FakeGpu:
    """What the predicates look at, for a machine without a GPU."""
    is_cuda = True

    def __init__(self, dtype, shape=(2, 64, 8, 8), requires_grad=False):
        self.dtype, self.shape, self.requires_grad = dtype, shape, requires_grad

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self.shape[-1] if i == -2 else 1


def test_predicate():
    bf, hf, f32 = _FakeGpu(torch.bfloat16), _FakeGpu(torch.float16), _FakeGpu(torch.float32)
    w, w_grad = _FakeGpu(torch.bfloat16, (64,)), _FakeGpu(torch.bfloat16, (64,), requires_grad=True)
    gn = torch.nn.GroupNorm(32, 64)
    with torch.enable_grad():
        assert unet.FUSE_UNET and unet.FUSE_UNET_GRAD
        assert unet.fused_glue_grad(bf) and unet.fused_glue_grad(hf, params=(w, None), norms=(gn,))
        assert unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (2, 64, 2560)))          # GEGLU's input
        assert not unet.fused_glue_grad(torch.zeros(2, 64, 8, 8, dtype=torch.bfloat16))    # a CPU tensor
        assert not unet.fused_glue_grad(f32) and not unet.fused_glue_grad(bf, params=(f32,))
        assert not unet.fused_glue_grad(bf, params=(w, w_grad))                       # a parameter wants a gradient
        # sizes the backward does not serve
        assert not unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (2, 64, 3, 3)))
        assert not unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (2, 36, 8, 8)), tokens=True)
        assert unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (2, 36, 8, 8)))
        assert not unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (2, 64, 2552)))
        big = torch.nn.GroupNorm(1, 32)
        assert not unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (1, 32, 64, 128)), norms=(big,))
        assert unet.fused_glue_grad(_FakeGpu(torch.bfloat16, (1, 32, 64, 120)), norms=(big,))
        assert not unet.fused_glue(bf)                                                # as before
        with torch.no_grad():
            assert not unet.fused_glue_grad(bf) and unet.fused_glue(bf)
    with torch.no_grad():
        assert not unet.fused_glue_grad(bf)


@pytest.mark.parametrize("switch", ["P2P_FUSE_UNET", "P2P_FUSE_UNET_GRAD"])
def test_switches_are_read_from_the_environment(switch):
    code = ("import torch; from p2p_amd import unet\n"
            "class T:\n"
            "    is_cuda = True; dtype = torch.bfloat16; shape = (2, 64, 8, 8); requires_grad = False\n"
            "    def dim(self): return 4\n"
            "with torch.enable_grad(): print(unet.fused_glue_grad(T()))\n"
            "with torch.no_grad(): print(unet.fused_glue(T()))")
    env = dict(os.environ, PYTHONPATH=PKG)
    env[switch] = "0"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["False", str(switch == "P2P_FUSE_UNET_GRAD")]


def test_modules_decline_on_cpu_and_with_trainable_parameters():
    """f32 on the CPU under grad: today's formulas, and gradients for the parameters."""
    torch.manual_seed(0)
    m = unet.ResnetBlock2D(64, 128, temb_ch=64)
    x, temb = torch.randn(2, 64, 8, 8, requires_grad=True), torch.randn(2, 64)
    m(x, temb).sum().backward()
    assert x.grad is not None and m.norm1.weight.grad is not None and m.conv2.bias.grad is not None
