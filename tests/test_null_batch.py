"""Batched null-text inversion, the parts that need no GPU: the two new C entry points are
exported beside ABI 16, p2p_null_loss and p2p_null_adam reject every bad argument before launching
anything, and NullInversion.invert_batch refuses inconsistent arguments before any kernel runs."""
import ctypes

import pytest
import torch

from p2p_amd import _hip, _srchash, null_text
from p2p_amd import pipeline as pl

E_ARG, E_DTYPE, E_BATCH, E_ALIGN = -1, -3, -5, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32


def test_symbols_abi_and_sources():
    for name in ("p2p_null_loss", "p2p_null_adam"):
        assert name in _hip.EXPORTED_SYMBOLS
        assert hasattr(_hip.lib(), name)
    for name in ("NullLossArgs", "NullAdamArgs", "null_loss", "null_adam"):
        assert hasattr(_hip, name)
    assert _hip.lib().p2p_abi_version() == 16
    assert "p2p_null.hip" in _srchash.SOURCES


def _loss(**kw):
    a = _hip.NullLossArgs()
    a.eps_u, a.eps_c, a.x, a.target = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    a.coef, a.active, a.loss, a.grad_eps_u = 4096, 8192, 8448, 5 << 20
    a.eps_dtype, a.guidance, a.B, a.n = F32, 7.5, 3, 16384
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(eps_u=None), E_ARG), (dict(eps_c=None), E_ARG), (dict(x=None), E_ARG), (dict(target=None), E_ARG),
    (dict(coef=None), E_ARG), (dict(active=None), E_ARG), (dict(loss=None), E_ARG), (dict(grad_eps_u=None), E_ARG),
    (dict(B=0), E_ARG), (dict(B=-1), E_ARG), (dict(n=0), E_ARG), (dict(n=-4), E_ARG),
    (dict(eps_dtype=F16), E_DTYPE), (dict(eps_dtype=9), E_DTYPE),
    (dict(B=65536), E_BATCH),
    (dict(n=16382), E_ALIGN), (dict(n=16385), E_ALIGN),
    (dict(eps_u=(1 << 20) + 8), E_ALIGN), (dict(eps_c=(2 << 20) + 4), E_ALIGN), (dict(x=(3 << 20) + 8), E_ALIGN),
    (dict(target=(4 << 20) + 4), E_ALIGN), (dict(coef=4100), E_ALIGN), (dict(grad_eps_u=(5 << 20) + 8), E_ALIGN),
    (dict(loss=8450), E_ALIGN),
])
def test_null_loss_rejects(kw, code):
    assert _hip.lib().p2p_null_loss(ctypes.byref(_loss(**kw)), None) == code
    if "eps_dtype" not in kw:
        assert _hip.lib().p2p_null_loss(ctypes.byref(_loss(eps_dtype=BF16, **kw)), None) == code


def test_null_entry_points_reject_null_struct():
    assert _hip.lib().p2p_null_loss(None, None) == E_ARG
    assert _hip.lib().p2p_null_adam(None, None) == E_ARG


def _adam(**kw):
    a = _hip.NullAdamArgs()
    a.param, a.grad, a.exp_avg, a.exp_avg_sq = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    a.lr, a.step, a.active, a.loss, a.threshold, a.steps_run = 4096, 4352, 4609, 4864, 5120, 5376
    a.B, a.m, a.beta1, a.beta2, a.eps = 3, 77 * 768, 0.9, 0.999, 1e-8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(param=None), E_ARG), (dict(grad=None), E_ARG), (dict(exp_avg=None), E_ARG), (dict(exp_avg_sq=None), E_ARG),
    (dict(lr=None), E_ARG), (dict(step=None), E_ARG), (dict(active=None), E_ARG), (dict(loss=None), E_ARG),
    (dict(threshold=None), E_ARG), (dict(steps_run=None), E_ARG),
    (dict(B=0), E_ARG), (dict(m=0), E_ARG), (dict(m=-4), E_ARG),
    (dict(beta1=1.0), E_ARG), (dict(beta2=-0.1), E_ARG), (dict(eps=-1e-8), E_ARG), (dict(beta1=float("nan")), E_ARG),
    (dict(B=65536), E_BATCH),
    (dict(m=77 * 768 + 2), E_ALIGN),
    (dict(param=(1 << 20) + 4), E_ALIGN), (dict(grad=(2 << 20) + 8), E_ALIGN), (dict(exp_avg=(3 << 20) + 4), E_ALIGN),
    (dict(exp_avg_sq=(4 << 20) + 8), E_ALIGN),
    (dict(lr=4098), E_ALIGN), (dict(step=4354), E_ALIGN), (dict(loss=4866), E_ALIGN), (dict(threshold=5121), E_ALIGN),
    (dict(steps_run=5378), E_ALIGN),
])
def test_null_adam_rejects(kw, code):
    assert _hip.lib().p2p_null_adam(ctypes.byref(_adam(**kw)), None) == code


NARROW = dict(block_out_channels=(32, 32, 32, 32), heads=2, layers_per_block=1)


@pytest.fixture(scope="module")
def cpu_inversion():
    model = pl.SyntheticStableDiffusion(device="cpu", dtype=torch.float32, unet_config=NARROW)
    return null_text.NullInversion(model, num_ddim_steps=2)


def test_invert_batch_value_errors(cpu_inversion):
    """Every one raised from the arguments alone: a CPU model has no kernels to call."""
    inv = cpu_inversion
    x = [torch.zeros(1, 4, 8, 8) for _ in range(3)]
    with pytest.raises(ValueError, match="prompts"):
        inv.invert_batch(x, ["a", "b"])
    with pytest.raises(ValueError, match="prompts"):
        inv.invert_batch(torch.zeros(3, 4, 8, 8), ["a", "b", "c", "d"])
    with pytest.raises(ValueError, match="prompts"):
        inv.invert_batch([], [])
    with pytest.raises(ValueError, match="early_stop_epsilon"):
        inv.invert_batch(x, ["a", "b", "c"], early_stop_epsilon=(1e-5, 1e-5))
    with pytest.raises(ValueError, match="one size"):
        inv.invert_batch([x[0], torch.zeros(1, 4, 16, 16), x[2]], ["a", "b", "c"])
    with pytest.raises(ValueError, match="one size"):
        inv.invert_batch([x[0], torch.zeros(2, 4, 8, 8)], ["a", "b"])


def test_invert_batch_refuses_fp16(cpu_inversion):
    inv = null_text.NullInversion(cpu_inversion.model, num_ddim_steps=2)
    unet = inv.model.unet
    try:
        inv.model.unet = unet.half()
        with pytest.raises(NotImplementedError, match="not float16"):
            inv.invert_batch(torch.zeros(2, 4, 8, 8), ["a", "b"])
    finally:
        inv.model.unet = unet.float()
