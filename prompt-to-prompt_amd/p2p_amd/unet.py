"""SD-v1.4-shaped U-Net with patchable ``CrossAttention`` modules (random init).

The reference runs diffusers-0.8.1's ``UNet2DConditionModel`` loaded from the SD-v1.4
checkpoint (main.py:25-30).  Neither is available offline, so this module rebuilds that
topology (block_out_channels 320/640/1280/1280, 2 layers per down block, 3 per up block,
8 heads -- diffusers-0.8.1 passes ``attention_head_dim=8`` as the head count -- cross dim
768, GEGLU feed-forward) with default-initialised weights.  What matters for the hot path is
kept exactly: 32 modules whose class is named ``CrossAttention`` with the 0.8.1 attribute
surface (``heads``, ``scale``, ``to_q/k/v``, ``to_out`` ModuleList,
``reshape_heads_to_batch_dim`` / ``reshape_batch_dim_to_heads``), called as
``attn1(x)`` then ``attn2(x, context=ctx)`` in every transformer block, in the order
down64 x2, down32 x2, down16 x2, mid8, up16 x3, up32 x3, up64 x3.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _hip, unet_grad

# The norm / activation / bias / residual / GEGLU glue between the convolutions and GEMMs runs on
# the HIP kernels of csrc/p2p_unet.hip (A/B switch, read once: 0 = the torch lines everywhere)
FUSE_UNET = os.environ.get("P2P_FUSE_UNET", "1") != "0"


def fused_glue(*tensors: torch.Tensor) -> bool:
    """Whether a module takes its fused path: inference (grad mode off) on GPU tensors in bf16 or
    f16, and the switch on.  Everything else -- CPU, f32, grad mode on -- runs the torch lines,
    unless ``fused_glue_grad`` takes the call (the U-Net's modules under autograd)."""
    if not FUSE_UNET or torch.is_grad_enabled():
        return False
    return all(t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) for t in tensors)


# Under autograd the same glue runs with the HIP backward of its kernels (unet_grad.py): null-text
# inversion's inner steps.  A/B switch, read once: 0 = the torch lines whenever grad mode is on
FUSE_UNET_GRAD = os.environ.get("P2P_FUSE_UNET_GRAD", "1") != "0"
GN_SLAB_LIMIT = 262144      # kGnStatsSplit (csrc/p2p_kernels.h): the backward serves slabs below it


def fused_glue_grad(*tensors: torch.Tensor, params=(), norms=(), tokens: bool = False) -> bool:
    """Whether a module takes its fused path under autograd: grad mode on, both switches on,
    ``tensors`` (the activations the glue differentiates) and ``params`` (the module's parameters and
    per-channel adds; None entries are skipped) on the GPU in bf16 or f16, none of ``params``
    requiring grad -- the kernels compute no gradient for them -- and sizes the backward serves,
    decided here from the sizes alone: a 4-D activation needs H * W % 8 == 0 (and C % 8 == 0 where
    the glue goes through ``tokens``) and, for every GroupNorm of ``norms``, a (sample, group) slab
    below GN_SLAB_LIMIT elements; any other activation is GEGLU's [..., 2 D] with D % 8 == 0 and a
    row stride % 8 == 0."""
    if not (FUSE_UNET and FUSE_UNET_GRAD) or not torch.is_grad_enabled():
        return False
    params = [p for p in params if p is not None]
    if not all(t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) for t in (*tensors, *params)):
        return False
    if any(p.requires_grad for p in params):
        return False
    for t in tensors:
        if t.dim() == 4:
            hw = t.shape[2] * t.shape[3]
            if hw % 8 or (tokens and t.shape[1] % 8):
                return False
            if any(nm.num_channels // nm.num_groups * hw >= GN_SLAB_LIMIT for nm in norms):
                return False
        elif t.shape[-1] % 16 or (t.dim() > 1 and t.stride(-2) % 8):
            return False
    return True


def _norm_act(norm: nn.GroupNorm, x, **kw):
    glue = unet_grad if torch.is_grad_enabled() else _hip
    return glue.group_norm(x, norm.weight, norm.bias, norm.num_groups, norm.eps, **kw)


def _bias_residual(*args, **kw):
    return (unet_grad if torch.is_grad_enabled() else _hip).bias_residual(*args, **kw)


# The resnets' 3x3 convolutions run on conv3x3_kernel (csrc/p2p_conv.hip) where p2p_select.h serves
# the shape (A/B switch, read once: 0 = MIOpen's convolution everywhere)
CONV_HIP = os.environ.get("P2P_CONV", "1") != "0"


def _conv3x3_packed(conv: nn.Conv2d, x):
    """The packed weight of ``conv`` where the HIP kernel takes conv(norm(x)) for x [N, C, H, W], else
    None: the switch off, a map the selection does not serve, or no packed weight to be had (a miss
    of the cache under graph capture)."""
    if not CONV_HIP:
        return None
    N, _, H, W = x.shape
    if _hip.conv3x3_split(N, H, W, conv.in_channels, conv.out_channels) < 1:
        return None
    return _hip.CONV_WEIGHTS.get(conv)


def _norm_act_conv(norm: nn.GroupNorm, conv: nn.Conv2d, x, hip: bool = True, **kw):
    """conv(silu(norm(x))) without conv's bias: the norm token-major into conv3x3_kernel where that
    serves the shape (and ``hip`` allows it), else the NCHW norm and the module's own convolution.
    None where the norm kernel does not serve x."""
    packed = _conv3x3_packed(conv, x) if hip else None
    if packed is not None:
        if torch.is_grad_enabled():
            y = unet_grad.group_norm_conv3x3(x, norm.weight, norm.bias, norm.num_groups, norm.eps, packed, conv.weight, **kw)
        else:
            h = _norm_act(norm, x, silu=True, tokens=True, **kw)
            y = None if h is None else _hip.conv3x3(h, packed, x.shape[2], x.shape[3])
        if y is not None:
            return y
    h = _norm_act(norm, x, silu=True, **kw)
    return None if h is None else conv._conv_forward(h, conv.weight, None)


class CrossAttention(nn.Module):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner = heads * dim_head
        context_dim = context_dim if context_dim is not None else query_dim
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(dropout)])

    def reshape_heads_to_batch_dim(self, t):
        b, n, c = t.shape
        h = self.heads
        return t.reshape(b, n, h, c // h).permute(0, 2, 1, 3).reshape(b * h, n, c // h)

    def reshape_batch_dim_to_heads(self, t):
        bh, n, d = t.shape
        h = self.heads
        return t.reshape(bh // h, h, n, d).permute(0, 2, 1, 3).reshape(bh // h, n, d * h)

    def forward(self, x, context=None, mask=None):
        # unpatched: plain attention on the HIP kernels (register_attention_control replaces this)
        from .attention import plain_attention
        q = self.to_q(x)
        src = x if context is None else context
        out = plain_attention(q, self.to_k(src), self.to_v(src), self.heads, self.scale)
        return self.to_out[1](self.to_out[0](out))


# The transformer blocks' feed-forward GEMMs run on linear_kernel (csrc/p2p_linear.hip), GEGLU and the
# residual add in their epilogues, where p2p_select.h serves the shape (A/B switch, read once: 0 =
# hipBLASLt's GEMMs with the glue kernels behind them everywhere)
LINEAR_HIP = os.environ.get("P2P_LINEAR", "1") != "0"


def _linear_fused(x, lin: nn.Linear) -> bool:
    """Whether ``lin`` of x may run on p2p_linear: the switch, and the conditions of the glue with
    ``lin``'s parameters frozen (the kernel computes no gradient for them)."""
    return LINEAR_HIP and (fused_glue(x, lin.weight) or fused_glue_grad(x, params=(lin.weight, lin.bias)))


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)

    def forward(self, x):
        if _linear_fused(x, self.proj):     # the GEMM, the bias and the gating in one launch
            out = unet_grad.linear_geglu(x, self.proj.weight, self.proj.bias)
            if out is not None:
                return out
        p = self.proj(x)
        if fused_glue(p) or fused_glue_grad(p):
            out = (unet_grad if torch.is_grad_enabled() else _hip).geglu(p)
            if out is not None:
                return out
        h, gate = p.chunk(2, dim=-1)
        return h * F.gelu(gate)


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4, dropout=0.0):
        super().__init__()
        inner = dim * mult
        self.net = nn.Sequential(GEGLU(dim, inner), nn.Dropout(dropout), nn.Linear(inner, dim))

    def forward(self, x):
        return self.net(x)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, context_dim):
        super().__init__()
        self.attn1 = CrossAttention(dim, None, n_heads, d_head)
        self.ff = FeedForward(dim)
        self.attn2 = CrossAttention(dim, context_dim, n_heads, d_head)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.norm3 = nn.LayerNorm(dim)

    def _forward_fused(self, x, context):
        """Each residual add runs inside the LayerNorm that reads it (p2p_layer_norm: the rounded
        sum is stored by the launch that normalises it); the attention modules are called as in the
        torch lines.  The last add has no norm behind it: it runs in the epilogue of the feed-forward's
        second GEMM (``_ff_residual``), or stays torch's where that keeps its lines.  Under autograd the same
        forward runs (unet_grad.layer_norm), so both modes give the same bits."""
        n1, n2, n3 = self.norm1, self.norm2, self.norm3
        out = unet_grad.layer_norm(x, n1.weight, n1.bias, n1.eps)
        if out is None:
            return None
        a = self.attn1(out[0])
        out = unet_grad.layer_norm(x, n2.weight, n2.bias, n2.eps, add=a)
        if out is None:
            raise _hip.HipError("p2p_layer_norm took norm1 and refused norm2 of the same block")
        h, s = out                        # s: the residual stream from here on (x is the caller's)
        c = self.attn2(h, context=context)
        out = unet_grad.layer_norm(s, n3.weight, n3.bias, n3.eps, add=c)
        if out is None:
            raise _hip.HipError("p2p_layer_norm took norm1 and refused norm3 of the same block")
        h, s = out
        return self._ff_residual(h, s)

    def _ff_residual(self, h, s):
        """ff(h) + s: where p2p_linear serves net[2]'s shape the add runs in that GEMM's epilogue,
        else exactly the torch lines."""
        geglu, drop, lin = self.ff.net
        if not _linear_fused(h, lin):
            return self.ff(h) + s
        g = drop(geglu(h))
        out = unet_grad.linear_residual(g, lin.weight, lin.bias, s)
        return out if out is not None else lin(g) + s

    def forward(self, x, context=None):
        norms = (self.norm1, self.norm2, self.norm3)
        if fused_glue(x, self.norm1.weight) or fused_glue_grad(
                x, params=[p for n in norms for p in (n.weight, n.bias)]):
            out = self._forward_fused(x, context)
            if out is not None:
                return out
        x = self.attn1(self.norm1(x)) + x
        x = self.attn2(self.norm2(x), context=context) + x
        return self.ff(self.norm3(x)) + x


class Transformer2DModel(nn.Module):
    def __init__(self, n_heads, d_head, in_channels, context_dim=768, groups=32):
        super().__init__()
        inner = n_heads * d_head
        self.norm = nn.GroupNorm(groups, in_channels, eps=1e-6)
        self.proj_in = nn.Conv2d(in_channels, inner, 1)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, n_heads, d_head, context_dim)])
        self.proj_out = nn.Conv2d(inner, in_channels, 1)

    def _forward_fused(self, x, ctx):
        """norm stores token-major, the 1x1 convs are GEMMs with a fused bias over the tokens, and
        the residual kernel reads the tokens and writes NCHW."""
        t = _norm_act(self.norm, x, tokens=True)
        if t is None:
            return None
        b, c, h, w = x.shape
        pi, po = self.proj_in, self.proj_out
        t = F.linear(t, pi.weight.view(pi.out_channels, pi.in_channels), pi.bias)
        for blk in self.transformer_blocks:
            t = blk(t, context=ctx)
        t = F.linear(t, po.weight.view(po.out_channels, po.in_channels), po.bias)
        out = _bias_residual(x, t, tokens=True)
        # (the blocks have run, controllers included: finish here rather than run them again)
        return out if out is not None else t.reshape(b, h, w, c).permute(0, 3, 1, 2) + x

    def forward(self, x, encoder_hidden_states=None):
        if fused_glue(x, self.proj_in.weight) or fused_glue_grad(
                x, params=(self.norm.weight, self.norm.bias, self.proj_in.weight), norms=(self.norm,), tokens=True):
            out = self._forward_fused(x, encoder_hidden_states)
            if out is not None:
                return out
        b, c, h, w = x.shape
        res = x
        x = self.proj_in(self.norm(x))
        x = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
        for blk in self.transformer_blocks:
            x = blk(x, context=encoder_hidden_states)
        x = x.reshape(b, h, w, c).permute(0, 3, 1, 2)
        return self.proj_out(x) + res


class ResnetBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, temb_ch=1280, groups=32, eps=1e-5):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, in_ch, eps=eps)
        self.conv1 = nn.Conv2d(in_ch, out_ch, 3, padding=1)
        # temb_ch None: the VAE's resnets (vae.py), which take no time embedding and have no projection
        if temb_ch is not None:
            self.time_emb_proj = nn.Linear(temb_ch, out_ch)
        # conv3x3_kernel was measured on the U-Net's shapes only: the VAE's resnets keep MIOpen
        self._conv_hip = temb_ch is not None
        self.norm2 = nn.GroupNorm(groups, out_ch, eps=eps)
        self.conv2 = nn.Conv2d(out_ch, out_ch, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(in_ch, out_ch, 1) if in_ch != out_ch else None

    def _forward_fused(self, x, temb, proj=None):
        """Both norms with their SiLU in one launch each; the convs run without bias: conv1's and
        the time embedding are added on load by norm2, conv2's and the shortcut's by the residual.
        Where conv3x3_kernel serves a convolution's shape the norm in front of it writes token-major
        and the kernel reads that (``_norm_act_conv``); elsewhere the NCHW norm and MIOpen.
        ``proj``: this block's time_emb_proj(F.silu(temb)) where the U-Net has computed it already."""
        c1, c2, sc = self.conv1, self.conv2, self.conv_shortcut
        h = _norm_act_conv(self.norm1, c1, x, hip=self._conv_hip)
        if h is None:
            return None
        if proj is not None:
            chan_add = proj
        else:
            chan_add = self.time_emb_proj(F.silu(temb)) if temb is not None else None
        h = _norm_act_conv(self.norm2, c2, h, hip=self._conv_hip, chan_add=chan_add, chan_bias=c1.bias)
        if h is None:
            return None
        if sc is not None:
            return _bias_residual(sc._conv_forward(x, sc.weight, None), h, c2.bias, sc.bias)
        return _bias_residual(x, h, c2.bias)

    def _glue_params(self, temb):
        """The module's parameters and the time embedding: the glue's backward leaves the norms'
        affine, the biases and the per-channel add without a gradient."""
        return (*self.parameters(), temb)

    def forward(self, x, temb=None):
        proj = None
        if isinstance(temb, TimeProjections):     # from UNet2DConditionModel.forward, fused inference only
            temb, proj = temb.emb, temb.of(self)
        if fused_glue(x, self.conv1.weight, *(() if temb is None else (temb,))) or fused_glue_grad(
                x, params=self._glue_params(temb), norms=(self.norm1, self.norm2)):
            out = self._forward_fused(x, temb, proj)
            if out is not None:
                return out
        h = self.conv1(F.silu(self.norm1(x)))
        if temb is not None:
            h = h + self.time_emb_proj(F.silu(temb))[:, :, None, None]
        h = self.conv2(F.silu(self.norm2(h)))
        if self.conv_shortcut is not None:
            x = self.conv_shortcut(x)
        return x + h


def _resample_conv(conv: nn.Conv2d, x, form: int):
    """``conv`` of x [N, C, H, W] in a sampling form of conv3x3_kernel (Up2: of x's nearest 2x upsampling,
    which is never written; Down2: at stride 2), bias included: one p2p_nchw_to_tokens pass over x (``_hip.conv_input_tokens``) and
    the kernel.  None where the module runs its own lines: the conditions of the resnets'
    convolutions (``fused_glue`` or ``fused_glue_grad``, CONV_HIP, a shape the selection serves, a
    packed weight -- none on a cache miss under graph capture)."""
    if not CONV_HIP or x.dim() != 4:
        return None
    if not (fused_glue(x, conv.weight) or fused_glue_grad(x, params=(conv.weight, conv.bias), tokens=True)):
        return None
    N, C, H, W = x.shape
    if (H * W) % 8 or C % 8 or not x.is_contiguous() or \
            _hip.conv3x3_ex_split(form, N, H, W, conv.in_channels, conv.out_channels) < 1:
        return None
    packed = _hip.CONV_WEIGHTS.get(conv)
    if packed is None:
        return None
    return unet_grad.resample_conv3x3(x, packed, conv.weight, conv.bias, form)


class Downsample2D(nn.Module):
    def __init__(self, ch, conv_hip: bool = False):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=1)
        # conv3x3_kernel's Down2 form was measured on the U-Net's shapes only: the blocks below opt in
        self._conv_hip = conv_hip

    def forward(self, x):
        if self._conv_hip:
            y = _resample_conv(self.conv, x, _hip.CONV_DOWN2)
            if y is not None:
                return y
        return self.conv(x)


class Upsample2D(nn.Module):
    def __init__(self, ch, conv_hip: bool = False):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, padding=1)
        # as Downsample2D: the U-Net's blocks opt in, the VAE (vae.py) keeps MIOpen
        self._conv_hip = conv_hip

    def forward(self, x):
        if self._conv_hip:
            y = _resample_conv(self.conv, x, _hip.CONV_UP2)
            if y is not None:
                return y
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class CrossAttnDownBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, layers=2, heads=8, context_dim=768, downsample=True, temb_ch=1280):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_ch if i == 0 else out_ch, out_ch, temb_ch)
                                      for i in range(layers)])
        self.attentions = nn.ModuleList([Transformer2DModel(heads, out_ch // heads, out_ch, context_dim)
                                         for _ in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(out_ch, conv_hip=True)]) if downsample else None

    def forward(self, x, temb, ctx):
        outs = ()
        for res, att in zip(self.resnets, self.attentions):
            x = att(res(x, temb), encoder_hidden_states=ctx)
            outs += (x,)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
            outs += (x,)
        return x, outs


class DownBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, layers=2, downsample=False, temb_ch=1280):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_ch if i == 0 else out_ch, out_ch, temb_ch)
                                      for i in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(out_ch, conv_hip=True)]) if downsample else None

    def forward(self, x, temb, ctx=None):
        outs = ()
        for res in self.resnets:
            x = res(x, temb)
            outs += (x,)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
            outs += (x,)
        return x, outs


def _up_resnets(in_ch, prev_ch, out_ch, layers, temb_ch=1280):
    mods = []
    for i in range(layers):
        skip = in_ch if i == layers - 1 else out_ch
        r_in = prev_ch if i == 0 else out_ch
        mods.append(ResnetBlock2D(r_in + skip, out_ch, temb_ch))
    return nn.ModuleList(mods)


class UpBlock2D(nn.Module):
    def __init__(self, in_ch, prev_ch, out_ch, layers=3, upsample=True, temb_ch=1280):
        super().__init__()
        self.resnets = _up_resnets(in_ch, prev_ch, out_ch, layers, temb_ch)
        self.upsamplers = nn.ModuleList([Upsample2D(out_ch, conv_hip=True)]) if upsample else None

    def forward(self, x, temb, skips, ctx=None):
        for res in self.resnets:
            x = res(torch.cat([x, skips[-1]], dim=1), temb)
            skips = skips[:-1]
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class CrossAttnUpBlock2D(nn.Module):
    def __init__(self, in_ch, prev_ch, out_ch, layers=3, heads=8, context_dim=768, upsample=True, temb_ch=1280):
        super().__init__()
        self.resnets = _up_resnets(in_ch, prev_ch, out_ch, layers, temb_ch)
        self.attentions = nn.ModuleList([Transformer2DModel(heads, out_ch // heads, out_ch, context_dim)
                                         for _ in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample2D(out_ch, conv_hip=True)]) if upsample else None

    def forward(self, x, temb, skips, ctx=None):
        for res, att in zip(self.resnets, self.attentions):
            x = res(torch.cat([x, skips[-1]], dim=1), temb)
            skips = skips[:-1]
            x = att(x, encoder_hidden_states=ctx)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class UNetMidBlock2DCrossAttn(nn.Module):
    def __init__(self, ch, heads=8, context_dim=768, temb_ch=1280):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, temb_ch), ResnetBlock2D(ch, ch, temb_ch)])
        self.attentions = nn.ModuleList([Transformer2DModel(heads, ch // heads, ch, context_dim)])

    def forward(self, x, temb, ctx):
        x = self.resnets[0](x, temb)
        x = self.attentions[0](x, encoder_hidden_states=ctx)
        return self.resnets[1](x, temb)


def timestep_embedding(timesteps: torch.Tensor, dim: int, max_period: int = 10000) -> torch.Tensor:
    """Sinusoidal embedding, flip_sin_to_cos=True, downscale_freq_shift=0 (SD-v1.4)."""
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(half, dtype=torch.float32, device=timesteps.device) / half
    emb = timesteps[:, None].float() * torch.exp(exponent)[None, :]
    return torch.cat([torch.cos(emb), torch.sin(emb)], dim=-1)


# The fused time path is adopted up to this many rows: measured at N = 8 it takes 96 us against the
# torch lines' 222 us, at N = 64 (--groups-per-call 8) 642 us against 235 us -- the kernels stage the
# activations once per workgroup and 8-row chunk -- so larger batches keep the torch lines
# (profiles/r15/transformer_glue/unet_ln_bench.txt)
TIME_FUSED_MAX_ROWS = 8


class TimeProjections:
    """What UNet2DConditionModel.forward hands its blocks in place of ``emb`` when the time path has
    run on the HIP kernels: ``emb`` itself and, per resnet, its time_emb_proj(F.silu(emb)) -- dense
    [N, C] views of one arena, computed up front in one launch."""

    def __init__(self, emb, by_linear):
        self.emb, self._by_linear = emb, by_linear

    def of(self, resnet):
        return self._by_linear.get(getattr(resnet, "time_emb_proj", None))


class TimestepEmbedding(nn.Module):
    def __init__(self, in_ch, dim):
        super().__init__()
        self.linear_1 = nn.Linear(in_ch, dim)
        self.linear_2 = nn.Linear(dim, dim)

    def forward(self, x):
        return self.linear_2(F.silu(self.linear_1(x)))


class UNet2DConditionModel(nn.Module):
    def __init__(self, in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280),
                 layers_per_block=2, heads=8, cross_attention_dim=768):
        super().__init__()
        self.in_channels = in_channels
        boc = list(block_out_channels)
        temb = boc[0] * 4
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        self.down_blocks = nn.ModuleList()
        out_ch = boc[0]
        for i in range(len(boc)):
            in_ch, out_ch = out_ch, boc[i]
            last = i == len(boc) - 1
            if last:
                self.down_blocks.append(DownBlock2D(in_ch, out_ch, layers_per_block, downsample=False, temb_ch=temb))
            else:
                self.down_blocks.append(CrossAttnDownBlock2D(in_ch, out_ch, layers_per_block, heads,
                                                             cross_attention_dim, downsample=True, temb_ch=temb))
        self.mid_block = UNetMidBlock2DCrossAttn(boc[-1], heads, cross_attention_dim, temb_ch=temb)
        self.up_blocks = nn.ModuleList()
        rev = boc[::-1]
        out_ch = rev[0]
        for i in range(len(rev)):
            prev, out_ch = out_ch, rev[i]
            in_ch = rev[min(i + 1, len(rev) - 1)]
            last = i == len(rev) - 1
            if i == 0:
                self.up_blocks.append(UpBlock2D(in_ch, prev, out_ch, layers_per_block + 1, upsample=True,
                                                temb_ch=temb))
            else:
                self.up_blocks.append(CrossAttnUpBlock2D(in_ch, prev, out_ch, layers_per_block + 1, heads,
                                                         cross_attention_dim, upsample=not last, temb_ch=temb))
        self.conv_norm_out = nn.GroupNorm(32, boc[0], eps=1e-5)
        self.conv_out = nn.Conv2d(boc[0], out_channels, 3, padding=1)
        # the resnets' time projections, in module order: the segments of p2p_time_proj (a plain
        # tuple: the modules are registered where they live)
        self._time_linears = tuple(m.time_emb_proj for m in self.modules() if isinstance(m, ResnetBlock2D))
        self._time_proj_table = None

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    def _time_path_fused(self, timestep):
        """emb and every resnet's time projection in three launches (p2p_time_embed, p2p_time_proj),
        as a TimeProjections; None -- the torch lines -- where a parameter of the path requires grad
        or the kernels do not serve the operands.  The segment table of the projections is built
        once and again whenever a weight has moved (``.to()``; an in-place load_state_dict keeps the
        addresses): a host-side comparison and, to build, one asynchronous copy from pinned memory,
        not under graph capture -- a capture whose model has no valid table runs the torch lines."""
        te = self.time_embedding
        linears = self._time_linears
        pairs = [(m.weight, m.bias) for m in linears]
        params = (*te.parameters(), *(t for pair in pairs for t in pair))
        if any(p.requires_grad for p in params) or timestep.dtype != torch.int64 or not timestep.is_cuda:
            return None
        if timestep.shape[0] > TIME_FUSED_MAX_ROWS:
            return None
        table = self._time_proj_table
        if table is None or not table.valid_for(pairs):
            if torch.cuda.is_current_stream_capturing():
                return None
            table = self._time_proj_table = _hip.TimeProjTable(pairs)
        emb = _hip.time_embed(timestep, te.linear_1.weight, te.linear_1.bias, te.linear_2.weight, te.linear_2.bias)
        if emb is None:
            return None
        outs = _hip.time_proj(emb, table)
        return emb if outs is None else TimeProjections(emb, dict(zip(linears, outs)))

    def forward(self, sample, timestep, encoder_hidden_states):
        if not torch.is_tensor(timestep):
            timestep = torch.tensor([timestep], dtype=torch.int64, device=sample.device)
        elif timestep.dim() == 0:
            timestep = timestep[None].to(sample.device)
        timestep = timestep.expand(sample.shape[0])
        emb = self._time_path_fused(timestep) if fused_glue(self.time_embedding.linear_1.weight) else None
        if emb is None:
            emb = self.time_embedding(timestep_embedding(timestep, self.conv_in.out_channels).to(self.dtype))
        ctx = encoder_hidden_states.to(self.dtype)
        x = self.conv_in(sample.to(self.dtype))
        skips = (x,)
        for blk in self.down_blocks:
            x, outs = blk(x, emb, ctx)
            skips += outs
        x = self.mid_block(x, emb, ctx)
        for blk in self.up_blocks:
            n = len(blk.resnets)
            res, skips = skips[-n:], skips[:-n]
            x = blk(x, emb, res, ctx)
        nout = self.conv_norm_out
        fused = fused_glue(x) or fused_glue_grad(x, params=(nout.weight, nout.bias), norms=(nout,))
        h = _norm_act(nout, x, silu=True) if fused else None
        x = self.conv_out(h if h is not None else F.silu(self.conv_norm_out(x)))
        return {"sample": x}
