"""SD-v1.4-shaped CLIP text encoder (random init): the ``model.text_encoder`` of the pipeline.

The reference encodes its prompts with the CLIP ViT-L/14 text transformer of Stable Diffusion v1.4
(ptp_utils.py:151,156; null_text.py through ``model.text_encoder``) and reads ``[0]``, the hidden
states behind the final LayerNorm.  As for the U-Net and the VAE, no checkpoint is available
offline, so this module rebuilds the topology with random weights: learned token and position
embeddings, 12 pre-LN layers of 12-head causal self-attention (head dim 64, no padding mask: the
pad id is the EOS id and causality keeps it out of every earlier row) and a quick-GELU MLP, a
final LayerNorm.  Parameters are named as the SD-v1.4 checkpoint names them
(``text_model.encoder.layers.3.self_attn.q_proj.bias`` ...), so its ``text_encoder`` state dict
loads (older checkpoints also carry a ``text_model.embeddings.position_ids`` buffer, which is not a
parameter here: load those with ``strict=False``).  Written from that description, not from any
library's source.

Every block decides per call (``unet.fused_glue``) between its torch lines -- f32, the CPU, grad
mode, ``P2P_FUSE_UNET=0``; they are also the reference of the tests -- and the fused path on the
kernels of csrc/p2p_text.hip.  A fused layer is eight launches:

  1. add + LayerNorm 1 (the previous layer's fc2 output and bias join the residual stream here)
  2. one stacked QKV GEMM
  3. the causal attention kernel, on three strided views of that GEMM's output
  4. out_proj without its bias
  5. add + LayerNorm 2 (out_proj's bias goes in here)
  6. fc1 without its bias
  7. bias + quick-GELU, in place
  8. fc2 without its bias: it is handed on, with its bias, to the next add + LayerNorm

The GEMMs are torch's.  The tokens x tokens matrix is never written on the fused path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _hip
from . import unet as _unet

# A/B switch of tools/text_bench.py: False keeps the fused glue but sends the attention proper
# through the torch lines (the tokens x tokens matrix and all)
FUSED_ATTENTION = True

# what a fused layer hands on instead of adding it: (fc2's output without its bias, fc2's bias)
Pending = Optional[Tuple[torch.Tensor, torch.Tensor]]


def quick_gelu(h):
    return h * torch.sigmoid(1.702 * h)


def _settle(x, pending: Pending):
    """The residual stream with a handed-on GEMM output added (the torch lines)."""
    return x if pending is None else x + (pending[0] + pending[1])


class TextEncoderOutput(tuple):
    """``(last_hidden_state, pooler_output)``: ``[0]`` is what the reference reads."""

    @property
    def last_hidden_state(self):
        return self[0]

    @property
    def pooler_output(self):
        return self[1]


class CLIPAttention(nn.Module):
    def __init__(self, hidden_size, num_heads):
        super().__init__()
        if hidden_size % num_heads:
            raise ValueError(f"hidden_size {hidden_size} not divisible by {num_heads} heads")
        self.num_heads = num_heads
        self.head_dim = hidden_size // num_heads
        self.scale = self.head_dim ** -0.5
        self.k_proj = nn.Linear(hidden_size, hidden_size)
        self.v_proj = nn.Linear(hidden_size, hidden_size)
        self.q_proj = nn.Linear(hidden_size, hidden_size)
        self.out_proj = nn.Linear(hidden_size, hidden_size)
        self._qkv = None

    def attend(self, q, k, v):
        """The torch lines of the attention proper on [N, T, C] operands (strided views too):
        token i attends to tokens <= i."""
        N, T, C = q.shape
        H, d = self.num_heads, self.head_dim
        q, k, v = (t.reshape(N, T, H, d).permute(0, 2, 1, 3) for t in (q, k, v))
        scores = torch.matmul(q, k.transpose(-1, -2)) * self.scale
        future = torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
        probs = scores.float().masked_fill(future, float("-inf")).softmax(dim=-1).to(q.dtype)
        return torch.matmul(probs, v).permute(0, 2, 1, 3).reshape(N, T, C)

    def _stacked(self):
        """q / k / v as one [3C, C] weight and [3C] bias: one GEMM, whose output the kernel reads as
        three strided views (row stride 3C).  Rebuilt when a parameter changed."""
        ps = (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight, self.q_proj.bias, self.k_proj.bias,
              self.v_proj.bias)
        key = tuple((p.data_ptr(), p._version, p.dtype) for p in ps)
        if self._qkv is None or self._qkv[0] != key:
            self._qkv = (key, torch.cat(ps[:3]), torch.cat(ps[3:]))
        return self._qkv[1], self._qkv[2]

    def forward_fused(self, h):
        """out_proj(attention(h)) WITHOUT out_proj's bias (the caller's add + LayerNorm takes it)."""
        C = h.shape[-1]
        w, b = self._stacked()
        qkv = F.linear(h, w, b)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        o = _hip.causal_attn(q, k, v, self.num_heads, self.scale) if FUSED_ATTENTION else None
        if o is None:      # the switch, or a head dim / token count without a kernel
            o = self.attend(q, k, v)
        return F.linear(o, self.out_proj.weight)

    def forward(self, h):
        return self.out_proj(self.attend(self.q_proj(h), self.k_proj(h), self.v_proj(h)))


class CLIPMLP(nn.Module):
    def __init__(self, hidden_size, intermediate_size):
        super().__init__()
        self.fc1 = nn.Linear(hidden_size, intermediate_size)
        self.fc2 = nn.Linear(intermediate_size, hidden_size)

    def forward(self, h):
        return self.fc2(quick_gelu(self.fc1(h)))


class CLIPEncoderLayer(nn.Module):
    """``x += out_proj(attn(LN1(x)))``, then ``x += fc2(quick_gelu(fc1(LN2(x))))``."""

    def __init__(self, hidden_size, intermediate_size, num_heads, eps):
        super().__init__()
        self.self_attn = CLIPAttention(hidden_size, num_heads)
        self.layer_norm1 = nn.LayerNorm(hidden_size, eps=eps)
        self.mlp = CLIPMLP(hidden_size, intermediate_size)
        self.layer_norm2 = nn.LayerNorm(hidden_size, eps=eps)
        self.fused_calls = 0     # forwards that took the fused path (the tests read it)

    def _forward_fused(self, x, pending: Pending):
        """x is this forward's own residual stream (never a caller's tensor): updated in place."""
        ln1, ln2 = self.layer_norm1, self.layer_norm2
        if pending is None:
            h = _hip.layer_norm(x, ln1.weight, ln1.bias, ln1.eps)
        else:
            h = _hip.layer_norm(x, ln1.weight, ln1.bias, ln1.eps, add=pending[0], add_bias=pending[1], sum_out=x)
        if h is None:
            return None
        a = self.self_attn.forward_fused(h)
        h = _hip.layer_norm(x, ln2.weight, ln2.bias, ln2.eps, add=a, add_bias=self.self_attn.out_proj.bias, sum_out=x)
        if h is None:
            raise _hip.HipError("p2p_layer_norm took layer_norm1 and refused layer_norm2 of the same layer")
        h = F.linear(h, self.mlp.fc1.weight)
        if _hip.bias_quick_gelu(h, self.mlp.fc1.bias, out=h) is None:
            h = quick_gelu(h + self.mlp.fc1.bias)
        self.fused_calls += 1
        return x, (F.linear(h, self.mlp.fc2.weight), self.mlp.fc2.bias)

    def forward(self, x, pending: Pending = None):
        """Returns (x, pending): the residual stream and, from the fused path, fc2's output and bias
        still to be added to it (by the next layer's, or the final, add + LayerNorm)."""
        if _unet.fused_glue(x, self.layer_norm1.weight):
            out = self._forward_fused(x, pending)
            if out is not None:
                return out
        x = _settle(x, pending)
        x = x + self.self_attn(self.layer_norm1(x))
        x = x + self.mlp(self.layer_norm2(x))
        return x, None


class CLIPEncoder(nn.Module):
    def __init__(self, hidden_size, intermediate_size, num_layers, num_heads, eps):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(hidden_size, intermediate_size, num_heads, eps)
                                     for _ in range(num_layers)])


class CLIPTextEmbeddings(nn.Module):
    def __init__(self, vocab_size, hidden_size, max_positions):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab_size, hidden_size)
        self.position_embedding = nn.Embedding(max_positions, hidden_size)

    def forward(self, ids):
        T = ids.shape[1]
        if T > self.position_embedding.num_embeddings:
            raise ValueError(f"{T} tokens, {self.position_embedding.num_embeddings} positions")
        return self.token_embedding(ids) + self.position_embedding.weight[:T]


class CLIPTextTransformer(nn.Module):
    def __init__(self, vocab_size, hidden_size, intermediate_size, num_layers, num_heads, max_positions, eps,
                 eos_token_id):
        super().__init__()
        self.eos_token_id = eos_token_id
        self.embeddings = CLIPTextEmbeddings(vocab_size, hidden_size, max_positions)
        self.encoder = CLIPEncoder(hidden_size, intermediate_size, num_layers, num_heads, eps)
        self.final_layer_norm = nn.LayerNorm(hidden_size, eps=eps)

    def forward(self, ids):
        x, pending = self.embeddings(ids), None     # a new tensor: the fused layers update it in place
        for layer in self.encoder.layers:
            x, pending = layer(x, pending)
        ln = self.final_layer_norm
        last = None
        if pending is not None and _unet.fused_glue(x, ln.weight):
            last = _hip.layer_norm(x, ln.weight, ln.bias, ln.eps, add=pending[0], add_bias=pending[1])
        if last is None:
            last = ln(_settle(x, pending))
        # the row at the first EOS (a row without one pools position 0, as argmax of all-zero does)
        eos = (ids == self.eos_token_id).int().argmax(dim=-1)
        pooled = last[torch.arange(last.shape[0], device=last.device), eos]
        return TextEncoderOutput((last, pooled))


class CLIPTextModel(nn.Module):
    """``forward(ids)`` -> ``TextEncoderOutput``: ``[0]`` / ``.last_hidden_state`` [N, T, C] behind the
    final LayerNorm, ``.pooler_output`` [N, C] its row at the first EOS.  The defaults are the
    SD-v1.4 shape.  ``generator``: draw every weight from it (embeddings N(0, 0.02^2), Linear weights
    N(0, 1 / fan_in), biases N(0, 0.02^2), LayerNorms at (1, 0)) and leave torch's global generator
    where it was; None keeps torch's default initialisation."""

    def __init__(self, vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                 num_attention_heads=12, max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=49407,
                 generator: Optional[torch.Generator] = None):
        super().__init__()
        args = (vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
                max_position_embeddings, layer_norm_eps, eos_token_id)
        if generator is None:
            self.text_model = CLIPTextTransformer(*args)
        else:
            with torch.random.fork_rng(devices=[]):
                self.text_model = CLIPTextTransformer(*args)
            self._init_from(generator)

    @torch.no_grad()
    def _init_from(self, g):
        for m in self.modules():
            if isinstance(m, nn.Embedding):
                m.weight.normal_(0.0, 0.02, generator=g)
            elif isinstance(m, nn.Linear):
                m.weight.normal_(0.0, m.in_features ** -0.5, generator=g)
                m.bias.normal_(0.0, 0.02, generator=g)

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    def forward(self, input_ids):
        return self.text_model(input_ids)
