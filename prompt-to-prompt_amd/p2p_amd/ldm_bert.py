"""LDM-256-shaped LDMBert text encoder (random init): the ``model.bert`` of the LDM pipeline.

The reference encodes its LDM-256 prompts with the LDMBert of ldm-text2im-large-256
(ptp_utils.py:113,116 through ``model.bert``, no attention mask) and reads ``[0]``, the hidden
states behind the final LayerNorm.  Neither that library nor a checkpoint is available offline, so
this module rebuilds the topology with random weights from its description: learned token and
position embeddings, 32 pre-LN layers of 8-head BIDIRECTIONAL self-attention whose width (8 heads x
64 = 512) is not the hidden size (1280) -- q / k / v projections without a bias, an output
projection with one -- and an exact (erf) GELU MLP of 5120, a final LayerNorm, and a ``to_logits``
head that the pipeline never evaluates (kept for the state dict).  Parameters carry the names of
that description (``model.layers.3.self_attn.q_proj.weight`` ...).  The shape is external
knowledge, written down from the description and not from any library's source, and its parity is
unpinned: no second implementation is available offline, so no test compares it with one.

Every layer decides per call (``unet.fused_glue``) between its torch lines -- f32, the CPU, grad
mode, ``P2P_FUSE_UNET=0``, an attention mask that is not a prefix of ones; they are also the
reference of the tests -- and the fused path on the kernels of csrc/p2p_text.hip, the eight
launches of text_encoder.CLIPEncoderLayer:

  1. add + LayerNorm (the previous layer's fc2 output and bias join the residual stream here)
  2. one stacked [3 x 512, 1280] QKV GEMM
  3. the bidirectional attention kernel, on three strided views of that GEMM's output
  4. out_proj without its bias
  5. add + LayerNorm (out_proj's bias goes in here)
  6. fc1 without its bias
  7. bias + erf-GELU, in place
  8. fc2 without its bias: it is handed on, with its bias, to the next add + LayerNorm

The GEMMs are torch's.  The tokens x tokens matrix is never written on the fused path.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _hip
from . import unet as _unet
from .text_encoder import Pending, _settle

# A/B switch of tools/text_bench.py: False keeps the fused glue but sends the attention proper
# through the torch lines (the tokens x tokens matrix and all)
FUSED_ATTENTION = True


class LDMBertAttention(nn.Module):
    def __init__(self, d_model, num_heads, head_dim):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = head_dim
        self.scale = head_dim ** -0.5
        inner = num_heads * head_dim
        self.k_proj = nn.Linear(d_model, inner, bias=False)
        self.v_proj = nn.Linear(d_model, inner, bias=False)
        self.q_proj = nn.Linear(d_model, inner, bias=False)
        self.out_proj = nn.Linear(inner, d_model)
        self._qkv = None

    def attend(self, q, k, v, key_mask=None):
        """The torch lines of the attention proper on [N, T, heads * head_dim] operands (strided views
        too): every token attends to every token, or to those ``key_mask`` [N, T] (bool) keeps."""
        N, T, C = q.shape
        H, d = self.num_heads, self.head_dim
        q, k, v = (t.reshape(N, T, H, d).permute(0, 2, 1, 3) for t in (q, k, v))
        scores = (torch.matmul(q, k.transpose(-1, -2)) * self.scale).float()
        if key_mask is not None:
            scores = scores.masked_fill(~key_mask[:, None, None, :], float("-inf"))
        probs = scores.softmax(dim=-1).to(q.dtype)
        return torch.matmul(probs, v).permute(0, 2, 1, 3).reshape(N, T, C)

    def _stacked(self):
        """q / k / v as one [3 * heads * head_dim, d_model] weight: one GEMM, whose output the kernel
        reads as three strided views.  Rebuilt when a parameter changed."""
        ps = (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight)
        key = tuple((p.data_ptr(), p._version, p.dtype) for p in ps)
        if self._qkv is None or self._qkv[0] != key:
            self._qkv = (key, torch.cat(ps))
        return self._qkv[1]

    def forward_fused(self, h, key_mask, key_counts):
        """out_proj(attention(h)) WITHOUT out_proj's bias (the caller's add + LayerNorm takes it)."""
        C = self.num_heads * self.head_dim
        qkv = F.linear(h, self._stacked())
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        o = _hip.text_attn(q, k, v, self.num_heads, self.scale, key_counts) if FUSED_ATTENTION else None
        if o is None:      # the switch, or a head dim / token count without a kernel
            o = self.attend(q, k, v, key_mask)
        return F.linear(o, self.out_proj.weight)

    def forward(self, h, key_mask=None):
        return self.out_proj(self.attend(self.q_proj(h), self.k_proj(h), self.v_proj(h), key_mask))


class LDMBertEncoderLayer(nn.Module):
    """``x += out_proj(attn(LN(x)))``, then ``x += fc2(gelu(fc1(LN(x))))``."""

    def __init__(self, d_model, num_heads, head_dim, ffn_dim, eps):
        super().__init__()
        self.self_attn = LDMBertAttention(d_model, num_heads, head_dim)
        self.self_attn_layer_norm = nn.LayerNorm(d_model, eps=eps)
        self.fc1 = nn.Linear(d_model, ffn_dim)
        self.fc2 = nn.Linear(ffn_dim, d_model)
        self.final_layer_norm = nn.LayerNorm(d_model, eps=eps)
        self.fused_calls = 0     # forwards that took the fused path (the tests read it)

    def _forward_fused(self, x, pending: Pending, key_mask, key_counts):
        """x is this forward's own residual stream (never a caller's tensor): updated in place."""
        ln1, ln2 = self.self_attn_layer_norm, self.final_layer_norm
        if pending is None:
            h = _hip.layer_norm(x, ln1.weight, ln1.bias, ln1.eps)
        else:
            h = _hip.layer_norm(x, ln1.weight, ln1.bias, ln1.eps, add=pending[0], add_bias=pending[1], sum_out=x)
        if h is None:
            return None
        a = self.self_attn.forward_fused(h, key_mask, key_counts)
        h = _hip.layer_norm(x, ln2.weight, ln2.bias, ln2.eps, add=a, add_bias=self.self_attn.out_proj.bias, sum_out=x)
        if h is None:
            raise _hip.HipError("p2p_layer_norm took the first LayerNorm and refused the second of the same layer")
        h = F.linear(h, self.fc1.weight)
        if _hip.bias_gelu(h, self.fc1.bias, out=h) is None:
            h = F.gelu(h + self.fc1.bias)
        self.fused_calls += 1
        return x, (F.linear(h, self.fc2.weight), self.fc2.bias)

    def forward(self, x, pending: Pending = None, key_mask=None, key_counts=None):
        """Returns (x, pending): the residual stream and, from the fused path, fc2's output and bias
        still to be added to it (by the next layer's, or the final, add + LayerNorm).  ``key_mask``
        [N, T] (bool) or None; ``key_counts`` int32 [N]: that mask as counts where its rows are
        prefixes of ones, else None -- and a mask without counts runs the torch lines."""
        if (key_mask is None or key_counts is not None) and _unet.fused_glue(x, self.self_attn_layer_norm.weight):
            out = self._forward_fused(x, pending, key_mask, key_counts)
            if out is not None:
                return out
        x = _settle(x, pending)
        x = x + self.self_attn(self.self_attn_layer_norm(x), key_mask)
        x = x + self.fc2(F.gelu(self.fc1(self.final_layer_norm(x))))
        return x, None


class LDMBertEncoder(nn.Module):
    def __init__(self, vocab_size, d_model, num_layers, num_heads, head_dim, ffn_dim, max_positions, eps):
        super().__init__()
        self.embed_tokens = nn.Embedding(vocab_size, d_model)
        self.embed_positions = nn.Embedding(max_positions, d_model)
        self.layers = nn.ModuleList([LDMBertEncoderLayer(d_model, num_heads, head_dim, ffn_dim, eps)
                                     for _ in range(num_layers)])
        self.layer_norm = nn.LayerNorm(d_model, eps=eps)

    @staticmethod
    def _keys(attention_mask, ids):
        """(key_mask, key_counts) of an [N, T] 0 / 1 mask: the mask as bool and, where every row is a
        prefix of at least one 1 (right padding), its row sums as int32 -- one host read per forward."""
        if attention_mask is None:
            return None, None
        if attention_mask.shape != ids.shape:
            raise ValueError(f"attention_mask {tuple(attention_mask.shape)} for ids {tuple(ids.shape)}")
        key_mask = attention_mask.to(ids.device) != 0
        counts = key_mask.sum(dim=-1, dtype=torch.int32)
        prefix = key_mask == (torch.arange(ids.shape[1], device=ids.device) < counts[:, None])
        if int(counts.min()) < 1:
            raise ValueError("attention_mask: a row without a 1 attends to nothing")
        return key_mask, (counts if bool(prefix.all()) else None)

    def forward(self, ids, attention_mask=None):
        T = ids.shape[1]
        if T > self.embed_positions.num_embeddings:
            raise ValueError(f"{T} tokens, {self.embed_positions.num_embeddings} positions")
        key_mask, key_counts = self._keys(attention_mask, ids)
        # a new tensor: the fused layers update it in place
        x, pending = self.embed_tokens(ids) + self.embed_positions.weight[:T], None
        for layer in self.layers:
            x, pending = layer(x, pending, key_mask, key_counts)
        ln = self.layer_norm
        last = None
        if pending is not None and _unet.fused_glue(x, ln.weight):
            last = _hip.layer_norm(x, ln.weight, ln.bias, ln.eps, add=pending[0], add_bias=pending[1])
        if last is None:
            last = ln(_settle(x, pending))
        return last


class LDMBertModel(nn.Module):
    """``forward(input_ids, attention_mask=None)`` -> ``(last_hidden_state,)``: ``[0]`` [N, T, d_model]
    behind the final LayerNorm, which is what the reference reads.  ``attention_mask``: None (the
    reference passes none: every token attends to all T) or [N, T] of 0 / 1, a 0 hiding that key
    from every row of its entry; all T rows are computed either way.  The defaults are the
    ldm-text2im-large-256 shape.  ``generator``: draw every weight from it (embeddings
    N(0, 0.02^2), Linear weights N(0, 1 / fan_in), biases N(0, 0.02^2), LayerNorms at (1, 0)) and
    leave torch's global generator where it was; None keeps torch's default initialisation."""

    def __init__(self, vocab_size=30522, d_model=1280, encoder_layers=32, encoder_attention_heads=8, head_dim=64,
                 encoder_ffn_dim=5120, max_position_embeddings=77, layer_norm_eps=1e-5,
                 generator: Optional[torch.Generator] = None):
        super().__init__()
        args = (vocab_size, d_model, encoder_layers, encoder_attention_heads, head_dim, encoder_ffn_dim,
                max_position_embeddings, layer_norm_eps)
        if generator is None:
            self.model = LDMBertEncoder(*args)
            self.to_logits = nn.Linear(d_model, vocab_size)
        else:
            with torch.random.fork_rng(devices=[]):
                self.model = LDMBertEncoder(*args)
                self.to_logits = nn.Linear(d_model, vocab_size)
            self._init_from(generator)

    @torch.no_grad()
    def _init_from(self, g):
        for m in self.modules():
            if isinstance(m, nn.Embedding):
                m.weight.normal_(0.0, 0.02, generator=g)
            elif isinstance(m, nn.Linear):
                m.weight.normal_(0.0, m.in_features ** -0.5, generator=g)
                if m.bias is not None:
                    m.bias.normal_(0.0, 0.02, generator=g)

    @property
    def dtype(self):
        return self.model.layer_norm.weight.dtype

    def forward(self, input_ids, attention_mask=None):
        return (self.model(input_ids, attention_mask),)
