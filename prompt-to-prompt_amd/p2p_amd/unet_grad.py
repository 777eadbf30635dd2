"""The U-Net glue under autograd: the forward kernels of csrc/p2p_unet.hip with their HIP backward
(p2p_group_norm_bwd, p2p_geglu_bwd, p2p_nchw_to_tokens), as ``torch.autograd.Function``s.

Gradients flow to the tensors only -- x of GroupNorm, the input of GEGLU, the two operands of the
residual add.  Parameters, biases and the per-channel adds get none: ``unet.fused_glue_grad`` declines
a call in which one of them requires grad, before the forward runs.  Nothing here synchronises with
the host or reads a value back, so a step that goes through these functions captures into one HIP
graph.  A call whose tensors do not require grad goes straight to the inference binding and costs
what it costs there (the layers ahead of the first cross-attention, in null-text inversion).

The wrappers return None where the forward binding reports the input unsupported, as the bindings
do; a backward binding that rejects what its forward served raises ``HipError``.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _hip


class _GroupNorm(torch.autograd.Function):
    """Saves x, the forward's {mean, rstd} and the per-channel operands; z and g are recomputed."""

    @staticmethod
    def forward(ctx, x, gamma, beta, chan_add, chan_bias, groups, eps, silu, tokens):
        out = _hip.group_norm(x, gamma, beta, groups, eps, silu=silu, tokens=tokens, chan_add=chan_add,
                              chan_bias=chan_bias, return_stats=True)
        if out is None:
            raise _hip.HipError(f"group_norm under autograd: {tuple(x.shape)} {x.dtype} is not served")
        y, stats = out
        ctx.save_for_backward(x, stats, gamma, beta, chan_add, chan_bias)
        ctx.glue = (groups, silu, tokens)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, stats, gamma, beta, chan_add, chan_bias = ctx.saved_tensors
        groups, silu, tokens = ctx.glue
        dx = _hip.group_norm_bwd(dy.contiguous(), x, stats, gamma, beta, groups, silu=silu, tokens=tokens,
                                 chan_add=chan_add, chan_bias=chan_bias)
        return dx, None, None, None, None, None, None, None, None


class _Geglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        out = _hip.geglu(x)
        if out is None:
            raise _hip.HipError(f"geglu under autograd: {tuple(x.shape)} {x.dtype} is not served")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, = ctx.saved_tensors
        return _hip.geglu_bwd(dout.contiguous(), x)


class _BiasResidual(torch.autograd.Function):
    """a + b + biases: both tensor gradients are dout; token-major b takes it transposed.  Saves
    nothing."""

    @staticmethod
    def forward(ctx, a, b, bias, bias2, tokens):
        out = _hip.bias_residual(a, b, bias, bias2, tokens=tokens)
        if out is None:
            raise _hip.HipError(f"bias_residual under autograd: {tuple(a.shape)} {a.dtype} is not served")
        ctx.tokens = tokens
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        da = dout if ctx.needs_input_grad[0] else None
        db = None
        if ctx.needs_input_grad[1]:
            db = _hip.nchw_to_tokens(dout.contiguous()) if ctx.tokens else dout
        return da, db, None, None, None


def _dense16(x: torch.Tensor) -> bool:
    return x.dim() == 4 and x.is_contiguous()


def group_norm(x, gamma, beta, groups: int, eps: float, silu: bool = False, tokens: bool = False,
               chan_add=None, chan_bias=None):
    """_hip.group_norm, differentiable with respect to x."""
    if not x.requires_grad:
        return _hip.group_norm(x, gamma, beta, groups, eps, silu=silu, tokens=tokens, chan_add=chan_add,
                               chan_bias=chan_bias)
    if not _dense16(x):
        return None
    return _GroupNorm.apply(x, gamma, beta, chan_add, chan_bias, int(groups), float(eps), bool(silu), bool(tokens))


def geglu(x):
    """_hip.geglu, differentiable with respect to x."""
    if not x.requires_grad:
        return _hip.geglu(x)
    x2 = x.reshape(-1, x.shape[-1])
    if x.shape[-1] % 2 or x2.stride(-1) != 1 or x2.data_ptr() != x.data_ptr():
        return None
    return _Geglu.apply(x)


def bias_residual(a_nchw, b, bias=None, bias2=None, tokens: bool = False):
    """_hip.bias_residual, differentiable with respect to a_nchw and b."""
    if not (a_nchw.requires_grad or b.requires_grad):
        return _hip.bias_residual(a_nchw, b, bias, bias2, tokens=tokens)
    if not _dense16(a_nchw) or not b.is_contiguous() or b.dtype != a_nchw.dtype:
        return None
    return _BiasResidual.apply(a_nchw, b, bias, bias2, bool(tokens))
