"""SD-v1.4-shaped ``AutoencoderKL`` (random init): images in and out of the latent pipeline.

The reference decodes its final latents with the SD-v1.4 VAE (ptp_utils.py:79-85) and null-text
inversion encodes the input image with it (null_text.py:519-529).  As for the U-Net (unet.py), no
checkpoint is available offline, so this module rebuilds diffusers-0.8.1's topology with
default-initialised weights: block_out_channels 128/256/512/512, two resnets per encoder block
and three per decoder block, one single-head attention block of 512 channels in each mid block,
GroupNorm(32, eps 1e-6) + SiLU throughout, 8-channel moments behind a 1x1 ``quant_conv`` and a 1x1
``post_quant_conv`` in front of the decoder.  Parameters are named as diffusers names them
(``encoder.down_blocks.0.resnets.0.conv1.weight``, ``decoder.mid_block.attentions.0.query.weight``,
``quant_conv.bias`` ...) so that a real checkpoint's ``state_dict`` could load; like the U-Net's,
those names are written from memory of that release and are not pinned against it here.

Every module decides per call (``unet.fused_glue``) between its torch lines -- f32, the CPU, grad
mode, ``P2P_FUSE_UNET=0``; they are also the reference of the tests -- and the fused path: the norm
/ SiLU / bias / residual glue of csrc/p2p_unet.hip around the convolutions, and for the attention
block the wide-head kernel of csrc/p2p_selfwide.hip (d = 512) through ``_hip.self_attn``, which
never writes the tokens x tokens probability matrix (64 MB per image in f32 at 64 x 64 latents).
Prompt-to-Prompt does not touch the VAE: nothing here is named ``CrossAttention`` or hooked.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _hip
from . import unet as _unet
from .unet import ResnetBlock2D, Upsample2D

VAE_EPS = 1e-6
# A/B switch of tools/vae_bench.py: False keeps the fused glue but sends the attention proper
# through the torch lines (the tokens x tokens matrix and all)
FUSED_ATTENTION = True


def _resnet(in_ch, out_ch, groups):
    return ResnetBlock2D(in_ch, out_ch, temb_ch=None, groups=groups, eps=VAE_EPS)


def _norm_silu(norm: nn.GroupNorm, x):
    """SiLU(GroupNorm(x)) in front of a conv_out."""
    h = _unet._norm_act(norm, x, silu=True) if _unet.fused_glue(x) else None
    return h if h is not None else F.silu(norm(x))


class AttentionBlock(nn.Module):
    """diffusers-0.8.1 ``AttentionBlock`` with one head: GroupNorm, q / k / v projections with bias,
    softmax(q k^T C^-1/2) v (diffusers scales q and k by C^-1/4 each: the same product), output
    projection, residual add."""

    def __init__(self, channels, groups=32, eps=VAE_EPS):
        super().__init__()
        self.channels = channels
        self.group_norm = nn.GroupNorm(groups, channels, eps=eps)
        self.query = nn.Linear(channels, channels)
        self.key = nn.Linear(channels, channels)
        self.value = nn.Linear(channels, channels)
        self.proj_attn = nn.Linear(channels, channels)
        self._qkv = None

    @property
    def scale(self):
        return self.channels ** -0.5

    def attend(self, q, k, v):
        """The torch lines of the attention proper on [N, tokens, C] operands (strided views too)."""
        scores = torch.matmul(q, k.transpose(1, 2)) * self.scale
        probs = scores.float().softmax(dim=-1).to(q.dtype)
        return torch.matmul(probs, v)

    def _stacked(self):
        """query / key / value as one [3C, C] weight and [3C] bias: one GEMM, whose output the kernel
        reads as three strided views (row stride 3C).  Rebuilt when a parameter changed."""
        ps = (self.query.weight, self.key.weight, self.value.weight, self.query.bias, self.key.bias, self.value.bias)
        key = tuple((p.data_ptr(), p._version, p.dtype) for p in ps)
        if self._qkv is None or self._qkv[0] != key:
            self._qkv = (key, torch.cat(ps[:3]), torch.cat(ps[3:]))
        return self._qkv[1], self._qkv[2]

    def _forward_fused(self, x):
        t = _unet._norm_act(self.group_norm, x, tokens=True)      # [N, HW, C]
        if t is None:
            return None
        C = self.channels
        w, b = self._stacked()
        qkv = F.linear(t, w, b)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        o = None
        if FUSED_ATTENTION:
            o = torch.empty_like(t)
            try:
                _hip.self_attn(q, k, v, o, 1, self.scale)
            except _hip.HipError as e:
                # a width or dtype without a kernel: the torch lines, on the same projections
                if e.code not in (_hip.P2P_E_HEAD_DIM, _hip.P2P_E_DTYPE):
                    raise
                o = None
        if o is None:
            o = self.attend(q, k, v)
        t = F.linear(o, self.proj_attn.weight, self.proj_attn.bias)
        out = _hip.bias_residual(x, t, tokens=True)
        if out is not None:
            return out
        n, c, h, wd = x.shape
        return t.reshape(n, h, wd, c).permute(0, 3, 1, 2) + x

    def forward(self, x):
        if _unet.fused_glue(x, self.query.weight):
            out = self._forward_fused(x)
            if out is not None:
                return out
        n, c, h, w = x.shape
        t = self.group_norm(x).reshape(n, c, h * w).transpose(1, 2)
        t = self.attend(self.query(t), self.key(t), self.value(t))
        t = self.proj_attn(t)
        return t.transpose(1, 2).reshape(n, c, h, w) + x


class Downsample2D(nn.Module):
    """The VAE's downsampler: one zero row / column on the bottom / right, then a stride-2 3x3 conv
    without padding (the U-Net's pads symmetrically instead)."""

    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class DownEncoderBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, layers, groups, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([_resnet(in_ch if i == 0 else out_ch, out_ch, groups) for i in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(out_ch)]) if downsample else None

    def forward(self, x):
        for res in self.resnets:
            x = res(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        return x


class UpDecoderBlock2D(nn.Module):
    def __init__(self, in_ch, out_ch, layers, groups, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([_resnet(in_ch if i == 0 else out_ch, out_ch, groups) for i in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample2D(out_ch)]) if upsample else None

    def forward(self, x):
        for res in self.resnets:
            x = res(x)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class UNetMidBlock2D(nn.Module):
    def __init__(self, ch, groups):
        super().__init__()
        self.attentions = nn.ModuleList([AttentionBlock(ch, groups)])
        self.resnets = nn.ModuleList([_resnet(ch, ch, groups), _resnet(ch, ch, groups)])

    def forward(self, x):
        x = self.resnets[0](x)
        x = self.attentions[0](x)
        return self.resnets[1](x)


class Encoder(nn.Module):
    def __init__(self, in_channels, out_channels, block_out_channels, layers_per_block, groups):
        super().__init__()
        boc = list(block_out_channels)
        self.conv_in = nn.Conv2d(in_channels, boc[0], 3, padding=1)
        self.down_blocks = nn.ModuleList()
        out_ch = boc[0]
        for i in range(len(boc)):
            in_ch, out_ch = out_ch, boc[i]
            self.down_blocks.append(DownEncoderBlock2D(in_ch, out_ch, layers_per_block, groups,
                                                       downsample=i != len(boc) - 1))
        self.mid_block = UNetMidBlock2D(boc[-1], groups)
        self.conv_norm_out = nn.GroupNorm(groups, boc[-1], eps=VAE_EPS)
        self.conv_out = nn.Conv2d(boc[-1], 2 * out_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for blk in self.down_blocks:
            x = blk(x)
        x = self.mid_block(x)
        return self.conv_out(_norm_silu(self.conv_norm_out, x))


class Decoder(nn.Module):
    def __init__(self, in_channels, out_channels, block_out_channels, layers_per_block, groups):
        super().__init__()
        rev = list(block_out_channels)[::-1]
        self.conv_in = nn.Conv2d(in_channels, rev[0], 3, padding=1)
        self.mid_block = UNetMidBlock2D(rev[0], groups)
        self.up_blocks = nn.ModuleList()
        out_ch = rev[0]
        for i in range(len(rev)):
            prev, out_ch = out_ch, rev[i]
            self.up_blocks.append(UpDecoderBlock2D(prev, out_ch, layers_per_block + 1, groups,
                                                   upsample=i != len(rev) - 1))
        self.conv_norm_out = nn.GroupNorm(groups, rev[-1], eps=VAE_EPS)
        self.conv_out = nn.Conv2d(rev[-1], out_channels, 3, padding=1)

    def forward(self, z):
        x = self.conv_in(z)
        x = self.mid_block(x)
        for blk in self.up_blocks:
            x = blk(x)
        return self.conv_out(_norm_silu(self.conv_norm_out, x))


class DiagonalGaussianDistribution:
    """The encoder's posterior: ``mean`` and a log-variance clamped to [-30, 20]."""

    def __init__(self, moments: torch.Tensor):
        self.mean, logvar = moments.chunk(2, dim=1)
        self.logvar = logvar.clamp(-30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self) -> torch.Tensor:
        return self.mean


class AutoencoderKL(nn.Module):
    def __init__(self, in_channels=3, out_channels=3, latent_channels=4,
                 block_out_channels: Sequence[int] = (128, 256, 512, 512), layers_per_block=2, norm_num_groups=32):
        super().__init__()
        self.encoder = Encoder(in_channels, latent_channels, block_out_channels, layers_per_block, norm_num_groups)
        self.decoder = Decoder(latent_channels, out_channels, block_out_channels, layers_per_block, norm_num_groups)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)

    @property
    def dtype(self):
        return self.quant_conv.weight.dtype

    def encode(self, x):
        """x: [N, 3, H, W] in [-1, 1] -> {"latent_dist": DiagonalGaussianDistribution} at H/8 (SD shape)."""
        moments = self.quant_conv(self.encoder(x.to(self.dtype)))
        return {"latent_dist": DiagonalGaussianDistribution(moments)}

    def decode(self, z):
        """z: [N, 4, h, w] -> {"sample": image [N, 3, 8h, 8w] (SD shape)} in the module's dtype."""
        return {"sample": self.decoder(self.post_quant_conv(z.to(self.dtype)))}

    def forward(self, x, generator=None):
        return self.decode(self.encode(x)["latent_dist"].sample(generator))
