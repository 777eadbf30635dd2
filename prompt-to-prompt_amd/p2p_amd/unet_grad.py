"""The U-Net glue under autograd: the forward kernels of csrc/p2p_unet.hip with their HIP backward
(p2p_group_norm_bwd, p2p_geglu_bwd, p2p_nchw_to_tokens), as ``torch.autograd.Function``s.

Gradients flow to the tensors only -- x of GroupNorm, the input of GEGLU, the two operands of the
residual add.  Parameters, biases and the per-channel adds get none: ``unet.fused_glue_grad`` declines
a call in which one of them requires grad, before the forward runs.  Nothing here synchronises with
the host or reads a value back, so a step that goes through these functions captures into one HIP
graph.  A call whose tensors do not require grad goes straight to the inference binding and costs
what it costs there (the layers ahead of the first cross-attention, in null-text inversion).

LayerNorm (the transformer blocks') has no HIP backward: ``_LayerNorm`` runs the p2p_layer_norm
forward, so that the autograd and no-grad forwards share their bits, and takes torch's gradient of
F.layer_norm at the saved sum.

The 3x3 convolution (csrc/p2p_conv.hip) has no HIP backward either: ``_GroupNormConv3x3`` runs the
token-major p2p_group_norm and p2p_conv3x3 forward -- the bits of the no-grad forward again -- and
takes torch's own input gradient of the convolution from the weight and dy into p2p_group_norm_bwd;
the convolution's input is not saved.  ``_ResampleConv3x3`` does the same for Upsample2D's and
Downsample2D's convolutions (the kernel's Up2 / Down2 forms on a token-major copy of the input): the
no-grad forward's two launches, then torch's input gradient of the convolution and, for Up2, of the
nearest upsampling.

The feed-forward GEMMs (csrc/p2p_linear.hip) run their forward on p2p_linear: ``_LinearGeglu`` has the
launch store the rounded pre-activation and feeds it to p2p_geglu_bwd, ``_LinearResidual`` passes dout
on to the residual; both take the input gradient from a torch matmul against the frozen weight.

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


class _LayerNorm(torch.autograd.Function):
    """(LN(x + add), the rounded sum) from p2p_layer_norm: the bits of the no-grad forward.  The
    library has no LayerNorm backward; the gradient is torch's own, taken through F.layer_norm at the
    saved sum -- what the torch lines compute from the same 16-bit tensor.  Saves the sum only."""

    @staticmethod
    def forward(ctx, x, add, gamma, beta, eps):
        s = torch.empty_like(x) if add is not None else x
        y = _hip.layer_norm(x, gamma, beta, eps, add=add, sum_out=s if add is not None else None)
        if y is None:
            raise _hip.HipError(f"layer_norm under autograd: {tuple(x.shape)} {x.dtype} is not served")
        ctx.save_for_backward(s, gamma, beta)
        ctx.eps, ctx.has_add = eps, add is not None
        if add is None:          # no sum of its own: the caller keeps x
            s = x.new_empty(0)
            ctx.mark_non_differentiable(s)
        return y, s

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, ds):
        s, gamma, beta = ctx.saved_tensors
        with torch.enable_grad():
            leaf = s.detach().requires_grad_(True)
            out = torch.nn.functional.layer_norm(leaf, (s.shape[-1],), gamma, beta, ctx.eps)
            g, = torch.autograd.grad(out, leaf, dy)
        if ctx.has_add:                  # the sum's own gradient reaches both of its operands
            g = g + ds
        return (g if ctx.needs_input_grad[0] else None), (g if ctx.needs_input_grad[1] else None), None, None, None


class _GroupNormConv3x3(torch.autograd.Function):
    """conv3x3(silu(GroupNorm(x + adds))) on the token-major p2p_group_norm and p2p_conv3x3: the bits of
    the no-grad forward.  Backward: torch's input gradient of F.conv2d(., weight, padding=1)
    (aten.convolution_backward with only the input mask set, from the weight and dy), which is NCHW,
    handed to p2p_group_norm_bwd as an NCHW dy -- the gradient of the norm does not depend on the
    layout its output was stored in, so nothing is transposed.  Saves what _GroupNorm saves and the
    weight, not the normalised tokens; the weight gets no gradient (fused_glue_grad declines a
    parameter that requires one)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, chan_add, chan_bias, groups, eps, packed, weight):
        out = _hip.group_norm(x, gamma, beta, groups, eps, silu=True, tokens=True, chan_add=chan_add,
                              chan_bias=chan_bias, return_stats=True)
        y = None if out is None else _hip.conv3x3(out[0], packed, x.shape[2], x.shape[3])
        if y is None:
            raise _hip.HipError(f"group_norm + conv3x3 under autograd: {tuple(x.shape)} {x.dtype} is not served")
        ctx.save_for_backward(x, out[1], gamma, beta, chan_add, chan_bias, weight)
        ctx.groups = groups
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, stats, gamma, beta, chan_add, chan_bias, weight = ctx.saved_tensors
        dh = torch.nn.grad.conv2d_input(tuple(x.shape), weight, dy.contiguous(), stride=1, padding=1)
        dx = _hip.group_norm_bwd(dh.contiguous(), x, stats, gamma, beta, ctx.groups, silu=True, tokens=False,
                                 chan_add=chan_add, chan_bias=chan_bias)
        return dx, None, None, None, None, None, None, None, None


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


def group_norm_conv3x3(x, gamma, beta, groups: int, eps: float, packed, weight, chan_add=None, chan_bias=None):
    """_hip.conv3x3 of the token-major _hip.group_norm (with SiLU) of x, differentiable with respect
    to x; ``weight`` is the [C_out, C_in, 3, 3] tensor ``packed`` was made from.  None where a
    binding does not serve the operands."""
    if not x.requires_grad:
        h = _hip.group_norm(x, gamma, beta, groups, eps, silu=True, tokens=True, chan_add=chan_add, chan_bias=chan_bias)
        return None if h is None else _hip.conv3x3(h, packed, x.shape[2], x.shape[3])
    if not _dense16(x) or packed.dtype != x.dtype or \
            _hip.conv3x3_split(x.shape[0], x.shape[2], x.shape[3], x.shape[1], packed.shape[1]) < 1:
        return None
    return _GroupNormConv3x3.apply(x, gamma, beta, chan_add, chan_bias, int(groups), float(eps), packed, weight)


class _ResampleConv3x3(torch.autograd.Function):
    """Upsample2D's / Downsample2D's convolution on p2p_nchw_to_tokens (``_hip.conv_input_tokens``) and p2p_conv3x3_ex (the Up2 or
    Down2 form, with the bias): the two launches and the bits of the no-grad forward.  Backward:
    torch's input gradient of the convolution (aten.convolution_backward with only the input mask
    set, from the weight and dy) at stride 2 for Down2; for Up2 at stride 1 on the upsampled map,
    followed by the nearest upsampling's backward.  The convolution's input is not saved (its shape
    is); weight and bias get no gradient (fused_glue_grad declines parameters that require one)."""

    @staticmethod
    def forward(ctx, x, packed, weight, bias, form):
        tokens = _hip.conv_input_tokens(x)
        y = None if tokens is None else _hip.conv3x3_ex(tokens, packed, bias, x.shape[2], x.shape[3], form)
        if y is None:
            raise _hip.HipError(f"resampling conv3x3 under autograd: {tuple(x.shape)} {x.dtype} is not served")
        ctx.save_for_backward(weight)
        ctx.form, ctx.x_shape = form, tuple(x.shape)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        weight, = ctx.saved_tensors
        n, c, h, w = ctx.x_shape
        if ctx.form == _hip.CONV_DOWN2:
            dx = torch.nn.grad.conv2d_input((n, c, h, w), weight, dy.contiguous(), stride=2, padding=1)
        else:
            du = torch.nn.grad.conv2d_input((n, c, 2 * h, 2 * w), weight, dy.contiguous(), stride=1, padding=1)
            dx = torch.ops.aten.upsample_nearest2d_backward(du, [2 * h, 2 * w], [n, c, h, w], 2.0, 2.0)
        return dx, None, None, None, None


def resample_conv3x3(x, packed, weight, bias, form: int):
    """_hip.conv3x3_ex of the token-major copy of x [N, C, H, W] in the Up2 or Down2 form,
    differentiable with respect to x; ``weight`` is the [C_out, C_in, 3, 3] tensor ``packed`` was made
    from.  None where a binding does not serve the operands."""
    n, c, h, w = x.shape
    if not _dense16(x) or packed.dtype != x.dtype or (h * w) % 8 or c % 8 or \
            _hip.conv3x3_ex_split(form, n, h, w, c, packed.shape[1]) < 1:
        return None
    if not x.requires_grad:
        tokens = _hip.conv_input_tokens(x)
        return None if tokens is None else _hip.conv3x3_ex(tokens, packed, bias, h, w, form)
    return _ResampleConv3x3.apply(x, packed, weight, bias, form)


def geglu(x):
    """_hip.geglu, differentiable with respect to x."""
    if not x.requires_grad:
        return _hip.geglu(x)
    x2 = x.reshape(-1, x.shape[-1])
    if x.shape[-1] % 2 or x2.stride(-1) != 1 or x2.data_ptr() != x.data_ptr():
        return None
    return _Geglu.apply(x)


class _LinearGeglu(torch.autograd.Function):
    """GEGLU(F.linear(x, weight, bias)) in one p2p_linear launch, which also stores the rounded
    pre-activation p for the backward: the bits of the no-grad forward (asking for p does not change
    them).  Backward: p2p_geglu_bwd at the saved p, then torch's matmul against the frozen weight.
    Weight and bias get no gradient (fused_glue_grad declines parameters that require one)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        out = _hip.linear(x, weight, bias, _hip.LINEAR_GEGLU, want_p=True)
        if out is None:
            raise _hip.HipError(f"linear + geglu under autograd: {tuple(x.shape)} {x.dtype} is not served")
        ctx.save_for_backward(out[1], weight)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        p, weight = ctx.saved_tensors
        return _hip.geglu_bwd(dout.contiguous(), p) @ weight, None, None


class _LinearResidual(torch.autograd.Function):
    """F.linear(x, weight, bias) + res in one p2p_linear launch (with its reduce where K is split): the
    bits of the no-grad forward.  Backward: dout against the frozen weight, and dout itself for the
    residual.  Saves the weight only."""

    @staticmethod
    def forward(ctx, x, weight, bias, res):
        out = _hip.linear(x, weight, bias, _hip.LINEAR_RESIDUAL, res=res)
        if out is None:
            raise _hip.HipError(f"linear + residual under autograd: {tuple(x.shape)} {x.dtype} is not served")
        ctx.save_for_backward(weight)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        weight, = ctx.saved_tensors
        dx = dout @ weight if ctx.needs_input_grad[0] else None
        return dx, None, None, (dout if ctx.needs_input_grad[3] else None)


def _linear_served(form: int, x, weight, res=None) -> bool:
    """Whether _hip.linear takes these operands, decided before an autograd node is made."""
    n = weight.shape[0] // 2 if form == _hip.LINEAR_GEGLU else weight.shape[0]
    if x.shape[-1] != weight.shape[1] or not weight.is_contiguous() or _hip._rows(x) is None:
        return False
    if res is not None and (_hip._rows(res) is None or tuple(res.shape) != tuple(x.shape[:-1]) + (n,)):
        return False
    m = x.numel() // x.shape[-1]
    return m > 0 and _hip.linear_split(form, m, weight.shape[1], n) >= 1


def linear_geglu(x, weight, bias):
    """_hip.linear in the GEGLU form, differentiable with respect to x.  None where not served."""
    if not x.requires_grad:
        return _hip.linear(x, weight, bias, _hip.LINEAR_GEGLU)
    if not _linear_served(_hip.LINEAR_GEGLU, x, weight):
        return None
    return _LinearGeglu.apply(x, weight, bias)


def linear_residual(x, weight, bias, res):
    """_hip.linear in the RESIDUAL form, differentiable with respect to x and res.  None where not served."""
    if not (x.requires_grad or res.requires_grad):
        return _hip.linear(x, weight, bias, _hip.LINEAR_RESIDUAL, res=res)
    if not _linear_served(_hip.LINEAR_RESIDUAL, x, weight, res):
        return None
    return _LinearResidual.apply(x, weight, bias, res)


def layer_norm(x, gamma, beta, eps: float, add=None):
    """(LN(x + add), x + add rounded) on _hip.layer_norm, differentiable with respect to x and add
    (``add`` None: (LN(x), x)).  None where the binding does not serve the operands."""
    if add is not None and (add.shape != x.shape or add.dtype != x.dtype or not add.is_contiguous()):
        return None
    if not (x.requires_grad or (add is not None and add.requires_grad)):
        s = torch.empty_like(x) if add is not None else x
        y = _hip.layer_norm(x, gamma, beta, eps, add=add, sum_out=s if add is not None else None)
        return None if y is None else (y, s)
    C = x.shape[-1]
    if not x.is_cuda or not x.is_contiguous() or x.dtype not in (torch.bfloat16, torch.float16) or C % 8 or \
            C > _hip.LN_MAX_CHANNELS or gamma.dtype != x.dtype or beta.dtype != x.dtype:
        return None
    y, s = _LayerNorm.apply(x, add, gamma, beta, float(eps))
    return y, (s if add is not None else x)


def bias_residual(a_nchw, b, bias=None, bias2=None, tokens: bool = False):
    """_hip.bias_residual, differentiable with respect to a_nchw and b."""
    if not (a_nchw.requires_grad or b.requires_grad):
        return _hip.bias_residual(a_nchw, b, bias, bias2, tokens=tokens)
    if not _dense16(a_nchw) or not b.is_contiguous() or b.dtype != a_nchw.dtype:
        return None
    return _BiasResidual.apply(a_nchw, b, bias, bias2, bool(tokens))
