"""Prompt-to-Prompt attention controllers -- the reference API, fused underneath.

Public surface of ``main.py:33-307`` (same class names, constructor arguments, attributes
and ``__call__`` / ``forward`` / ``step_callback`` / ``between_steps`` / ``reset`` /
``get_average_attention`` protocol).  The difference is underneath: when the patched
``CrossAttention.forward`` (ptp_utils.register_attention_control) finds one of these
controllers, it calls :meth:`AttentionControl.attention`, which launches ONE HIP kernel per
call that computes the attention with the controller's edit and store fused in:

* self-attention: flash kernel; source-map injection as a batch index remap;
* cross-attention: exact-softmax kernel; Replace / Refine / Reweight as a device edit
  program (programs.py) applied between softmax and PV;
* AttentionStore: probabilities written (step 0) or added (later steps) to the running-sum
  tensors in the kernel epilogue, only for the maps the reference keeps (P <= 32**2).

A subclass that overrides any method the fused kernel encodes (``forward``,
``replace_cross_attention``, ``replace_self_attention``, ``__call__``) gets the reference
protocol instead: the probabilities are materialised by a HIP kernel, handed to
``controller(attn, is_cross, place_in_unet)`` and multiplied by V by a second HIP kernel.
"""
from __future__ import annotations

import abc
import os
from collections import defaultdict
from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from . import _hip
from . import config
from . import programs
from . import seq_aligner
from .attention import materialized_attention, plain_attention
from .ptp_words import get_time_words_attention_alpha, get_word_inds
from .tokenizer import default_tokenizer

NUM_DIFFUSION_STEPS = 100   # main.py:19
GUIDANCE_SCALE = 7.5        # main.py:20
MAX_NUM_WORDS = 77          # main.py:21
MAX_STORED_QUERIES = 32 ** 2  # main.py:131

_tokenizer = None


def set_tokenizer(tokenizer):
    """The reference reads a module-global ``tokenizer`` (main.py:30); this sets ours."""
    global _tokenizer
    _tokenizer = tokenizer


def get_tokenizer():
    return _tokenizer if _tokenizer is not None else default_tokenizer()


def default_device() -> torch.device:
    return torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")


def _low_resource() -> bool:
    return bool(config.LOW_RESOURCE)


class NotFusable(Exception):
    """Raised while planning a fused call that the kernels cannot express."""


# ============================================================================ LocalBlend
def _blend_maps(attention_store, alpha_flat, workspace=True):
    """The five 16x16 cross maps LocalBlend reads (main.py:37-38) as dense f32, their heads per
    prompt and (``workspace``) the word-sum workspace p2p_localblend fills from them."""
    maps = list(attention_store["down_cross"][2:4]) + list(attention_store["up_cross"][:3])
    B = alpha_flat.shape[0]
    if len(maps) != 5:
        raise ValueError(f"LocalBlend needs 2 down and 3 up 16x16 cross maps, store has {len(maps)}")
    heads = maps[0].shape[0] // B
    maps = [m if (m.dtype == torch.float32 and m.is_contiguous()) else m.float().contiguous() for m in maps]
    if not workspace:
        return maps, heads, None
    return maps, heads, torch.empty(B * 2 * len(maps) * heads * maps[0].shape[1], dtype=torch.float32,
                                    device=maps[0].device)


def fused_local_blend(x_t, attention_store, alpha_flat, sub_flat, th_pool, th_sub):
    """LocalBlend on the running-sum store with the HIP blend kernels (returns a new x_t)."""
    maps, heads, ws = _blend_maps(attention_store, alpha_flat)
    out = x_t.to(torch.float32).contiguous().clone()
    _hip.localblend(maps, heads, alpha_flat, sub_flat, th_pool, th_sub, out, ws)
    return out.to(x_t.dtype)


class FoldedBlendMask:
    """One prompt group's LocalBlend mask in the form it is built from: the running word sums
    [B, 2, lh, res^2] that the cross-attention store epilogue folded (AttentionControlEdit.
    _blend_fold).  p2p_latent_step builds the mask from them inside the latent-update launch --
    LocalBlend and the CFG/DDIM step are one kernel per denoising step (null_text.py:41-70,
    ptp_utils.py:72-75).  materialize() builds the same mask as a uint8 [B, H, W] tensor with
    p2p_localblend (mixed prompt-group batches, tests)."""

    def __init__(self, maps, heads, alpha_flat, sub_flat, th_pool, th_sub, size, sums):
        self._maps, self._heads, self._alpha, self._sub = maps, heads, alpha_flat, sub_flat
        self.th_pool, self.th_sub, self.size, self.sums = float(th_pool), float(th_sub), tuple(size), sums

    def latent_entry(self):
        """The per-group entry of _hip.latent_step(blend=...)."""
        return self.sums, self.th_pool, self.th_sub, self._sub is not None

    def materialize(self) -> torch.Tensor:
        mask = torch.empty(self._alpha.shape[0], *self.size, dtype=torch.uint8, device=self.sums.device)
        _hip.localblend(self._maps, self._heads, self._alpha, self._sub, self.th_pool, self.th_sub, None, self.sums,
                        mask_out=mask, word_sums_ready=True)
        return mask


def as_mask(m):
    """A step mask as a uint8 tensor (materialising a FoldedBlendMask), or None."""
    return m.materialize() if isinstance(m, FoldedBlendMask) else m


class StepMask(NamedTuple):
    """What fused_step_mask()'s mask_fn(size) returns: per prompt group None (no blend this step), a
    uint8 mask [B, H, W] or a FoldedBlendMask; group_size 0 = a single controller (one group, the
    whole batch).  ptp_utils._launch_latent_step turns it into the latent step's arguments."""
    entries: list
    group_size: int


def group_mask_tensor(masks, B, size):
    """Per-group step masks (None = the group does not blend) as the mask-reading latent step's
    (mask [G*B, H, W] uint8, group size, groups that blend [G] uint8) triple."""
    masks = [as_mask(mk) for mk in masks]
    dev = next(mk for mk in masks if mk is not None).device
    out = torch.zeros(len(masks) * B, *size, dtype=torch.uint8, device=dev)
    blend = torch.zeros(len(masks), dtype=torch.uint8)
    for g, mk in enumerate(masks):
        if mk is not None:
            out[g * B:(g + 1) * B] = mk
            blend[g] = 1
    return out, B, blend.to(dev)


def fused_blend_mask(attention_store, alpha_flat, sub_flat, th_pool, th_sub, size, folded=None):
    """LocalBlend's final mask [B, H, W] (uint8) only; the latent blend itself then runs inside
    p2p_latent_step together with the CFG combine and the DDIM step.  ``folded``: the running word
    sums [B, 2, 5 * heads, 256] that the cross-attention store epilogue accumulated
    (AttentionControlEdit._blend_fold) -- then the 12.6 MB of maps are not re-read, and the mask
    is returned as a FoldedBlendMask that p2p_latent_step builds in the same launch."""
    if folded is not None:
        maps, heads, _ = _blend_maps(attention_store, alpha_flat, workspace=False)
        return FoldedBlendMask(maps, heads, alpha_flat, sub_flat, th_pool, th_sub, size, folded)
    maps, heads, ws = _blend_maps(attention_store, alpha_flat)
    mask = torch.empty(alpha_flat.shape[0], *size, dtype=torch.uint8, device=ws.device)
    _hip.localblend(maps, heads, alpha_flat, sub_flat, th_pool, th_sub, None, ws, mask_out=mask)
    return mask


def _owned(obj, name) -> bool:
    """True when ``name`` resolves to a method this library defines (not a user override)."""
    for owner in type(obj).__mro__:
        if name in owner.__dict__:
            return bool(owner.__dict__.get("_P2P_LIB", False))
    return False


def _word_alpha_layers(prompts, words, tokenizer, n_words=MAX_NUM_WORDS):
    a = torch.zeros(len(prompts), 1, 1, 1, 1, n_words)
    for i, (prompt, ws) in enumerate(zip(prompts, words)):
        for word in ([ws] if type(ws) is str else ws):
            a[i, :, :, :, :, get_word_inds(prompt, word, tokenizer)] = 1
    return a


class LocalBlend:
    """main.py:33-66.  Valid for two prompts only, as in the reference (its mask
    ``mask[:1] + mask[1:]`` does not broadcast for more); use null_text.LocalBlend for B > 2."""

    def __call__(self, x_t, attention_store):
        if self.alpha_layers.shape[0] != 2:
            raise ValueError("main-form LocalBlend broadcasts only for 2 prompts (see null_text.LocalBlend)")
        return fused_local_blend(x_t, attention_store, self._alpha_flat, None, self.threshold, self.threshold)

    def step_mask(self, attention_store, size, folded=None):
        """The blend mask __call__ would apply this step (fused latent-step protocol)."""
        if self.alpha_layers.shape[0] != 2:
            raise ValueError("main-form LocalBlend broadcasts only for 2 prompts (see null_text.LocalBlend)")
        return fused_blend_mask(attention_store, self._alpha_flat, None, self.threshold, self.threshold, size,
                                folded)

    def _fold_tables(self):
        """(alpha [B, W], substruct [B, W] or None) the store epilogue folds the word sums with."""
        return self._alpha_flat, None

    def __init__(self, prompts: List[str], words, threshold=.3, tokenizer=None, device=None):
        tokenizer = tokenizer or get_tokenizer()
        device = device or default_device()
        self.alpha_layers = _word_alpha_layers(prompts, words, tokenizer).to(device)
        self._alpha_flat = self.alpha_layers.reshape(len(prompts), -1).contiguous()
        self.threshold = threshold


LocalBlend._P2P_LIB = True


# ============================================================================ controllers
class AttentionControl(abc.ABC):
    """main.py:69-107 -- step/layer counters and the cond-half dispatch."""

    _NATIVE = ("__call__",)

    def step_callback(self, x_t):
        return x_t

    def fused_step_mask(self):
        """Fused latent-step protocol (ptp_utils.diffusion_step): (True, mask_fn) when this
        step's step_callback is this library's own -- mask_fn (None: nothing to do) then has the
        callback's side effects and returns the step's StepMask -- else (False, None)."""
        if not _owned(self, "step_callback"):
            return False, None
        try:
            entry_fn = self._step_mask_entry()
        except NotFusable:
            return False, None
        return True, (None if entry_fn is None else lambda size: StepMask([entry_fn(size)], 0))

    def _step_mask_entry(self):
        """None, or fn(size) -> this controller's StepMask entry."""
        return None

    def between_steps(self):
        return

    @property
    def num_uncond_att_layers(self):
        return self.num_att_layers if _low_resource() else 0

    @abc.abstractmethod
    def forward(self, attn, is_cross: bool, place_in_unet: str):
        raise NotImplementedError

    def __call__(self, attn, is_cross: bool, place_in_unet: str):
        if self.cur_att_layer >= self.num_uncond_att_layers:
            if _low_resource():
                attn = self.forward(attn, is_cross, place_in_unet)
            else:
                half = attn.shape[0] // 2
                attn[half:] = self.forward(attn[half:], is_cross, place_in_unet)
        self._advance_layer()
        return attn

    def _advance_layer(self):
        self.cur_att_layer += 1
        if self.cur_att_layer == self.num_att_layers + self.num_uncond_att_layers:
            self.cur_att_layer = 0
            self.cur_step += 1
            self.between_steps()
            self._fused_calls = defaultdict(int)

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0
        self._fused_calls, self._fused_sums = defaultdict(int), {}

    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0
        # the fused store's bookkeeping (_fused_attention): stored calls so far this step per
        # "<place>_<kind>" key, and the running-sum tensor of each (key, call)
        self._fused_calls, self._fused_sums = defaultdict(int), {}

    # ------------------------------------------------------------------ fused protocol
    def fused_supported(self) -> bool:
        """True when every method the fused kernels encode is this library's own."""
        cls = type(self)
        names = set()
        for owner in cls.__mro__:
            names.update(owner.__dict__.get("_NATIVE", ()))
        for name in names:
            # the class that resolves `name` must be one of ours
            for owner in cls.__mro__:
                if name in owner.__dict__:
                    if not owner.__dict__.get("_P2P_LIB", False):
                        return False
                    break
        return True

    def _fused_forward(self, q, k, v, heads, scale, is_cross, place_in_unet):
        raise NotFusable

    def attention(self, q, k, v, heads, scale, is_cross, place_in_unet, mask=None):
        """Called by the patched CrossAttention.forward with the projections q, k, v."""
        if mask is None and self.fused_supported():
            try:
                if self.cur_att_layer >= self.num_uncond_att_layers:
                    out = self._fused_forward(q, k, v, heads, scale, is_cross, place_in_unet)
                else:
                    out = plain_attention(q, k, v, heads, scale)
                self._advance_layer()
                return out
            except NotFusable:
                pass
        return materialized_attention(self, q, k, v, heads, scale, is_cross, place_in_unet, mask)

    def _cond_start(self, n_batch: int) -> int:
        return 0 if _low_resource() else n_batch // 2

    # What a controller contributes to its prompt group of a fused call.  A plain controller
    # contributes nothing; AttentionStore adds its stores (step_store, attention_store,
    # store_self_maps), AttentionControlEdit its edit (batch_size, _cross_alpha, _cross_step,
    # _blend_fold, _injects_source).  GroupBatch drives its members through these and
    # _advance_layer only.
    def _cross_alpha(self):
        """This step's cross_replace_alpha row; None: no cross-attention edit."""
        return None

    def _injects_source(self, K: int) -> bool:
        """Whether this step's self-attention over K keys gives the edits the source's Q and K."""
        return False

    def _mutual_source(self, layer: int) -> bool:
        """Whether self-attention call ``layer`` of this step gives the edits the source's K and V
        (MutualSelfAttentionControl)."""
        return False

    def _folds_words(self) -> bool:
        """Whether a controller WITHOUT a cross edit folds word sums in the stored cross launches."""
        return False

    def _fused_attention(self, members, group_size, q, k, v, heads, scale, is_cross, place_in_unet):
        """ONE kernel launch for the prompt groups that share this U-Net call: ``members`` holds one
        controller per group, each owning ``group_size`` prompts of the conditional half -- or, with
        group_size 0, the single controller ``[self]`` whose group is the conditional half whatever
        its size.  Translates the members' state into the kernels' terms: the AttentionStore target
        (allocated on the first step, accumulated into afterwards; every member's step_store gets its
        view of the one running-sum tensor per layer) and slots, the p2p_group tuples of
        _hip.cross_attn, the qk_src remap of _hip.self_attn.  ``self`` keeps the store bookkeeping."""
        N, P, K = q.shape[0], q.shape[1], k.shape[1]
        batched = group_size > 0
        if batched:
            B, n0 = group_size, len(members) * group_size
            if N != 2 * n0:
                raise ValueError(f"GroupBatch of {len(members)} x {B} prompts got a U-Net batch of {N}")
        else:
            n0 = self._cond_start(N)
            B = N - n0
        for m in members:
            if getattr(m, "batch_size", B) != B:
                raise ValueError(f"controller built for {m.batch_size} prompts got a batch of {B}")
        cross = is_cross and K <= _hip.MAX_KEYS_CROSS
        edits = [None] * len(members)       # per member None or its cross edit (alpha row, program, hints)
        if is_cross:
            alphas = [m._cross_alpha() for m in members]
            fit = cross and all(a is None or (a.shape[-1] == K and a.device == q.device) for a in alphas)
            if not batched and alphas[0] is not None and not fit:
                raise NotFusable        # a single edit controller falls back to the materialised protocol
            if cross and not fit:
                raise ValueError("edit tables do not match this attention call")
            if cross:   # (before the store is touched: a program the tables cannot hold raises NotFusable)
                edits = [None if a is None else (a.contiguous(),) + m._cross_step(q.device, K)
                         for m, a in zip(members, alphas)]
        self_maps = {bool(m.store_self_maps) for m in members if isinstance(m, AttentionStore)}
        if not is_cross and len(self_maps) > 1:
            raise ValueError("GroupBatch members disagree on store_self_maps")
        store, acc, slots, store_key = None, False, None, None
        if self_maps and P <= MAX_STORED_QUERIES and (is_cross or True in self_maps):
            key = f"{place_in_unet}_{'cross' if is_cross else 'self'}"
            store_key = (key, self._fused_calls[key])
            self._fused_calls[key] += 1
            if len(members[0].attention_store) == 0:
                rows = B * heads
                store = self._fused_sums[store_key] = torch.empty(len(members) * rows, P, K, dtype=torch.float32,
                                                                  device=q.device)
                for g, m in enumerate(members):
                    m.step_store[key].append(store[g * rows:(g + 1) * rows])
            else:
                store, acc = self._fused_sums.get(store_key), True
                if store is None:       # this layer's sum was not made here (a materialised first step)
                    raise NotFusable
            slots = [-1] * n0 + [(n - n0) * heads for n in range(n0, N)]
        out = torch.empty_like(q)
        if not cross:
            # self-attention calls so far this step: the layer index of _mutual_source
            layer = None if is_cross else self._fused_calls["self_layer"]
            if layer is not None:
                self._fused_calls["self_layer"] += 1
                mutual = [m._mutual_source(layer) for m in members]
                if any(mutual):
                    if store is not None or any(m._injects_source(K) for m in members):
                        raise ValueError("mutual self-attention shares a launch neither with kept self maps nor with "
                                         "an AttentionControlEdit's source injection")
                    return _mutual_attention(self, members, mutual, B, n0, q, k, v, out, heads, scale)
            qk_src = None                   # (the identity)
            for g, m in enumerate(members):
                if not is_cross and m._injects_source(K):
                    first = n0 + g * B      # P_edit <- P_source, V stays the edit's own
                    qk_src = qk_src or list(range(N))
                    qk_src[first + 1:first + B] = [first] * (B - 1)
            _hip.self_attn(q, k, v, out, heads, scale, compute=config.COMPUTE, qk_src=qk_src, store=store,
                           store_slot=slots, accumulate=acc)
            return out
        # a controller without a cross edit may still fold word sums (the mutual one's token classes)
        folds = [m._blend_fold(store_key, P, K, heads, q.device) if edit is None and store is not None and m._folds_words()
                 else None for m, edit in zip(members, edits)]
        if batched or edits[0] is not None or folds[0] is not None:
            # the uncond rows ("" prompts) share their K / V: staged once per workgroup (SHARED_KV)
            groups = [(0, n0, None, None, None, _hip.shared_kv_hint(k, v, 0, n0))] if n0 else []
            for g, (m, edit) in enumerate(zip(members, edits)):
                if edit is None:
                    groups.append((n0 + g * B, B, None, None) if folds[g] is None else
                                  (n0 + g * B, B, None, None, folds[g], 0))
                    continue
                alpha, prog, hints = edit
                blend = m._blend_fold(store_key, P, K, heads, q.device) if store is not None else None
                groups.append((n0 + g * B, B, prog, alpha, blend, hints))
        else:
            groups = [(0, N, None, None)]       # a plain controller: one group over the whole batch
        _hip.cross_attn(q, k, v, out, heads, scale, groups, compute=config.COMPUTE, store=store, store_slot=slots,
                        accumulate=acc)
        return out


AttentionControl._P2P_LIB = True


class EmptyControl(AttentionControl):
    """main.py:110-113."""

    _NATIVE = ("forward",)

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        return attn

    def _fused_forward(self, q, k, v, heads, scale, is_cross, place_in_unet):
        return plain_attention(q, k, v, heads, scale)


EmptyControl._P2P_LIB = True


class AttentionStore(AttentionControl):
    """main.py:116-159.  ``store_self_maps = False`` keeps only the cross maps (the ones
    LocalBlend and ``show_cross_attention`` read); the default matches the reference."""

    _NATIVE = ("forward", "between_steps")
    store_self_maps = True

    @staticmethod
    def get_empty_store():
        return {"down_cross": [], "mid_cross": [], "up_cross": [],
                "down_self": [], "mid_self": [], "up_self": []}

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        key = f"{place_in_unet}_{'cross' if is_cross else 'self'}"
        if attn.shape[1] <= MAX_STORED_QUERIES:
            self.step_store[key].append(attn)
        return attn

    def between_steps(self):
        if len(self.attention_store) == 0:
            self.attention_store = self.step_store
        else:
            # fused calls already added their maps in the kernel epilogue; only maps handed
            # over through the materialised protocol are still pending here
            for key, items in self.step_store.items():
                for i, item in enumerate(items):
                    self.attention_store[key][i] += item
        self.step_store = self.get_empty_store()

    def get_average_attention(self):
        def avg(item):
            if item.is_cuda and item.dtype == torch.float32 and item.is_contiguous():
                return _hip.store_scale(item, float(self.cur_step))
            return item / self.cur_step
        return {key: [avg(item) for item in self.attention_store[key]] for key in self.attention_store}

    def reset(self):
        super().reset()
        self.step_store = self.get_empty_store()
        self.attention_store = {}

    def __init__(self):
        super().__init__()
        self.step_store = self.get_empty_store()
        self.attention_store = {}

    def _fused_forward(self, q, k, v, heads, scale, is_cross, place_in_unet):
        return self._fused_attention([self], 0, q, k, v, heads, scale, is_cross, place_in_unet)


AttentionStore._P2P_LIB = True


class AttentionControlEdit(AttentionStore, abc.ABC):
    """main.py:162-212."""

    _NATIVE = ("forward", "replace_self_attention", "_replace_self")
    SELF_REPLACE_MAX_KEYS = 16 ** 2   # main.py:170 (null_text.py:225 uses 32 ** 2)

    def step_callback(self, x_t):
        if self.local_blend is not None:
            x_t = self.local_blend(x_t, self.attention_store)
        return x_t

    def _step_mask_entry(self):
        lb = self.local_blend
        if lb is None:
            return None
        if not (_owned(lb, "__call__") and hasattr(lb, "step_mask")):
            raise NotFusable
        return lambda size: lb.step_mask(self.attention_store, size,
                                         folded=self._blend_sums if self._blend_valid else None)

    # LocalBlend's word reduction folded into the cross-attention store epilogue: the five 16x16
    # cross layers it reads (main.py:37-38, down_cross[2:4] + up_cross[:3]) get their running word
    # sums accumulated by the kernel that writes their maps, so the blend reads ~0.3 MB instead
    # of the 12.6 MB of maps every step.  Valid only while EVERY step folded all five layers.
    BLEND_SLOTS = {("down_cross", 2): 0, ("down_cross", 3): 1, ("up_cross", 0): 2, ("up_cross", 1): 3,
                   ("up_cross", 2): 4}
    # The fold sums each step's word sums (sum over steps of sum over words) where the reference
    # takes the word sums of the summed maps (main.py:37-44): equal in exact arithmetic, a
    # different f32 summation order in practice, so a pixel sitting on the threshold can flip
    # (tests/test_gpu_blend_fold.py pins the agreement).  False = strict parity: the blend reads
    # the stored maps as the reference does.
    fold_local_blend = True

    def _blend_fold(self, key_idx, P, K, heads, device):
        """The p2p_group.blend_* tuple for this stored cross layer, or None."""
        lb = self.local_blend
        slot = self.BLEND_SLOTS.get(key_idx)
        if not self.fold_local_blend or slot is None or lb is None or P != 256 or not (_owned(lb, "__call__") and hasattr(lb, "_fold_tables")):
            return None
        alpha, sub = lb._fold_tables()
        if alpha.shape != (self.batch_size, K) or alpha.device != device:
            return None
        lh = len(self.BLEND_SLOTS) * heads
        if len(self.attention_store) == 0 and slot == 0:
            self._blend_sums = torch.empty(self.batch_size, 2, lh, P, dtype=torch.float32, device=device)
            self._blend_valid = False
            self._blend_step = set()
        if self._blend_sums is None or self._blend_sums.shape != (self.batch_size, 2, lh, P):
            return None
        self._blend_step.add(slot)
        return self._blend_sums, alpha, sub, slot * heads, lh

    def between_steps(self):
        # a step in which some blend layer did not fold (materialised protocol, a new run) ends
        # the folded sums' validity until the next reset
        first = len(self.attention_store) == 0
        complete = self._blend_sums is not None and len(self._blend_step) == len(self.BLEND_SLOTS)
        self._blend_valid = complete and (first or self._blend_valid)
        self._blend_step = set()
        super().between_steps()

    def reset(self):
        super().reset()
        self._blend_sums, self._blend_valid, self._blend_step = None, False, set()

    def replace_self_attention(self, attn_base, att_replace):
        if att_replace.shape[2] <= self.SELF_REPLACE_MAX_KEYS:
            return attn_base.unsqueeze(0).expand(att_replace.shape[0], *attn_base.shape)
        return att_replace

    @abc.abstractmethod
    def replace_cross_attention(self, attn_base, att_replace):
        raise NotImplementedError

    def _in_self_window(self) -> bool:
        return self.num_self_replace[0] <= self.cur_step < self.num_self_replace[1]

    def _injects_source(self, K):
        return self._in_self_window() and K <= self.SELF_REPLACE_MAX_KEYS

    def _cross_alpha(self):
        return self.cross_replace_alpha[self.cur_step]

    def _replace_self(self, attn_base, att_replace, place_in_unet):
        return self.replace_self_attention(attn_base, att_replace)

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        """Reference protocol on a materialised [B*H, P, K] tensor (main.py:180-197)."""
        AttentionStore.forward(self, attn, is_cross, place_in_unet)
        if not (is_cross or self._in_self_window()):
            return attn
        per_prompt = attn.reshape(self.batch_size, attn.shape[0] // self.batch_size, *attn.shape[1:])
        base, edits = per_prompt[0], per_prompt[1:]
        if is_cross:
            a = self.cross_replace_alpha[self.cur_step]
            per_prompt[1:] = self.replace_cross_attention(base, edits) * a + (1 - a) * edits
        else:
            per_prompt[1:] = self._replace_self(base, edits, place_in_unet)
        return per_prompt.reshape(attn.shape[0], *attn.shape[1:])

    def __init__(self, prompts, num_steps: int,
                 cross_replace_steps: Union[float, Tuple[float, float], Dict[str, Tuple[float, float]]],
                 self_replace_steps: Union[float, Tuple[float, float]],
                 local_blend: Optional[LocalBlend], tokenizer=None, device=None):
        super().__init__()
        self.tokenizer = tokenizer or get_tokenizer()
        self.device = device or default_device()
        self.batch_size = len(prompts)
        self.cross_replace_alpha = get_time_words_attention_alpha(
            prompts, num_steps, cross_replace_steps, self.tokenizer).to(self.device)
        if type(self_replace_steps) is float:
            self_replace_steps = 0, self_replace_steps
        self.num_self_replace = int(num_steps * self_replace_steps[0]), int(num_steps * self_replace_steps[1])
        self.local_blend = local_blend
        self._program_cache = {}
        self._program_host = None
        self._alpha_host = None
        self._step_cache = {}
        self._blend_sums, self._blend_valid, self._blend_step = None, False, set()

    # ------------------------------------------------------------------ fused edits
    def _edit_program(self) -> programs.EditProgram:
        raise NotFusable

    def _device_program(self, device):
        key = str(device)
        if key not in self._program_cache:
            try:
                host = self._edit_program()
                self._program_cache[key] = host.to_device(device)
                self._program_host = host
            except ValueError as err:      # beyond the program tables: materialised protocol
                raise NotFusable from err
        return self._program_cache[key]

    def _cross_step(self, device, K):
        """The cross-attention edit of this step as (program or None, p2p_group hint flags), from
        the host copy of cross_replace_alpha[cur_step] (main.py:189) and the program's c_rep / post:
        with B = alpha post and A = alpha post c_rep + 1 - alpha on every word of every edit,
          * B = 0 and A = 1 everywhere (past cross_replace_steps): P' = R * 0 + P_e = P_e exactly,
            the group runs unedited (no program: the kernels load no mapper, no source rows);
          * A = 0 everywhere (a Replace / Reweight step inside the window): P' = R B, the edits'
            own softmax, Q and K are dead -- GROUP_F_R_ONLY.
        Decided once per step (the alpha table is copied to the host once)."""
        prog = self._device_program(device)
        alpha = self.cross_replace_alpha
        # (the tensor itself, its version, host copy): identity, not id().  A tensor made under
        # torch.inference_mode() has no version counter: its storage address stands in for it
        version = ("ptr", alpha.data_ptr()) if alpha.is_inference() else alpha._version
        held = self._alpha_host
        if held is None or held[0] is not alpha or held[1] != version:
            held = self._alpha_host = (alpha, version, alpha.detach().to("cpu", torch.float64).numpy())
            self._step_cache = {}
        key = (self.cur_step, K)
        hit = self._step_cache.get(key)
        if hit is not None:
            return (None if hit[0] else prog), hit[1]
        host = self._program_host
        a = held[2][self.cur_step].reshape(host.n_edits, -1)[:, :K]
        post = host.post[:, :K].astype(np.float64)
        crep = host.c_rep[:, :K].astype(np.float64)
        B = a * post
        A = B * crep + (1.0 - a)
        plain = bool(np.all(B == 0.0) and np.all(A == 1.0))
        hints = _hip.GROUP_F_R_ONLY if np.all(A == 0.0) else 0
        self._step_cache[key] = (plain, hints)
        return (None if plain else prog), hints


AttentionControlEdit._P2P_LIB = True


class AttentionReplace(AttentionControlEdit):
    """main.py:215-230."""

    _NATIVE = ("replace_cross_attention",)

    def replace_cross_attention(self, attn_base, att_replace):
        return torch.einsum('hpw,bwn->bhpn', attn_base, self.mapper)

    def _edit_program(self):
        return programs.replace_program(self.mapper)

    def __init__(self, prompts, num_steps: int, cross_replace_steps: float, self_replace_steps: float,
                 local_blend: Optional[LocalBlend] = None, tokenizer=None, device=None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend,
                         tokenizer, device)
        self.mapper = seq_aligner.get_replacement_mapper(prompts, self.tokenizer).to(self.device)


AttentionReplace._P2P_LIB = True


class AttentionRefine(AttentionControlEdit):
    """main.py:233-253."""

    _NATIVE = ("replace_cross_attention",)

    def replace_cross_attention(self, attn_base, att_replace):
        gathered = attn_base[:, :, self.mapper].permute(2, 0, 1, 3)
        return gathered * self.alphas + att_replace * (1 - self.alphas)

    def _edit_program(self):
        return programs.refine_program(self.mapper, self.alphas)

    def __init__(self, prompts, num_steps: int, cross_replace_steps: float, self_replace_steps: float,
                 local_blend: Optional[LocalBlend] = None, tokenizer=None, device=None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend,
                         tokenizer, device)
        mapper, alphas = seq_aligner.get_refinement_mapper(prompts, self.tokenizer)
        self.mapper, alphas = mapper.to(self.device), alphas.to(self.device)
        self.alphas = alphas.reshape(alphas.shape[0], 1, 1, alphas.shape[1])


AttentionRefine._P2P_LIB = True


class AttentionReweight(AttentionControlEdit):
    """main.py:256-278 (optionally chained on a Replace / Refine controller)."""

    _NATIVE = ("replace_cross_attention",)

    def replace_cross_attention(self, attn_base, att_replace):
        if self.prev_controller is not None:
            attn_base = self.prev_controller.replace_cross_attention(attn_base, att_replace)
        return attn_base[None, :, :, :] * self.equalizer[:, None, None, :]

    def _edit_program(self):
        inner = None
        prev = self.prev_controller
        if prev is not None:
            if not (isinstance(prev, AttentionControlEdit) and prev.fused_supported()):
                raise NotFusable
            inner = prev._edit_program()
            if not np.all(inner.post == 1.0):
                raise NotFusable
        return programs.reweight_program(self.equalizer, self.batch_size - 1, inner)

    def __init__(self, prompts, num_steps: int, cross_replace_steps: float, self_replace_steps: float,
                 equalizer, local_blend: Optional[LocalBlend] = None,
                 controller: Optional[AttentionControlEdit] = None, tokenizer=None, device=None):
        super().__init__(prompts, num_steps, cross_replace_steps, self_replace_steps, local_blend,
                         tokenizer, device)
        self.equalizer = equalizer.to(self.device)
        self.prev_controller = controller


AttentionReweight._P2P_LIB = True


# ============================================================================ mutual self-attention
# MasaCtrl (Cao et al., ICCV 2023, §3.2-3.3): the opposite of replace_self_attention.  An edit row
# keeps its own queries and reads the SOURCE row's keys and values, which keeps the content and
# lets the layout move; with ``ref_words`` a foreground query reads only the source's foreground
# keys and a background query its background keys (the mask-guided form).
MUTUAL_KERNELS = os.environ.get("P2P_MUTUAL", "1") != "0"    # 0: the torch lines below instead of p2p_mutual_attn_fwd
MUTUAL_MAX_SIDES = 3                                         # resolutions per p2p_token_classes launch


def mutual_attention_torch(q, k, v, heads, scale, kv_src, token_class, out):
    """The mathematics of p2p_mutual_attn_fwd in torch lines (f32): out[n] = softmax(q[n] k[s]^T *
    scale + M) v[s], s = kv_src[n]; s < 0 leaves out[n] alone.  With ``token_class`` (uint8 [N, P])
    and s != n a query reads the keys of its own class in entry s, every key where s has none."""
    N, P, C = q.shape
    d = C // heads

    def split(x, n):
        return x[n].float().reshape(P, heads, d).transpose(0, 1)          # [H, P, d]
    for n in range(N):
        s = int(kv_src[n])
        if s < 0:
            continue
        logits = torch.einsum("hpd,hjd->hpj", split(q, n), split(k, s)) * scale
        if token_class is not None and s != n:
            cq, ck = token_class[n].bool(), token_class[s].bool()
            has = torch.stack([(~ck).any(), ck.any()])
            admitted = (cq[:, None] == ck[None, :]) | ~has[cq.long()][:, None]
            logits = logits.masked_fill(~admitted[None], float("-inf"))
        o = torch.einsum("hpj,hjd->hpd", logits.softmax(-1), split(v, s))
        out[n] = o.transpose(0, 1).reshape(P, C).to(out.dtype)
    return out


def token_classes_torch(sums, threshold, sides, cfg=True):
    """The torch lines of p2p_token_classes: ``sums`` one [B, 2, lh, res^2] f32 tensor per prompt
    group; per side a uint8 [rows, side^2] tensor, the uncond rows (cfg) a copy of the cond rows."""
    cls = []
    for s in sums:
        m = s[:, 0].float().sum(1) / s.shape[2]                           # mean over the lh maps
        mn, mx = m.min(1, keepdim=True).values, m.max(1, keepdim=True).values
        rng = mx - mn
        cls.append(torch.where(rng > 0, (m - mn) / rng >= threshold, torch.zeros_like(m, dtype=torch.bool)))
    cls = torch.cat(cls, 0)
    res = int(round(cls.shape[1] ** 0.5))
    cls = cls.reshape(-1, res, res)
    outs = []
    for side in sides:
        idx = (torch.arange(side, device=cls.device) * res) // side      # nearest: floor(dst * res / side)
        up = cls[:, idx][:, :, idx].reshape(cls.shape[0], side * side).to(torch.uint8)
        outs.append(torch.cat([up, up], 0) if cfg else up)
    return outs


def _mutual_classes(owner, members, B, N, P, device):
    """The uint8 [N, P] token classes of this step for a mutual layer of P tokens, or None (unmasked:
    no member has ref_words, or the word sums are not complete yet).  Built once per step, at the
    step's first mutual layer, for every resolution a mutual layer has had so far -- one
    p2p_token_classes launch, into tensors allocated once -- and kept on ``owner``."""
    masked = {m._ref_alpha is not None for m in members}
    if masked == {False}:
        return None
    if len(masked) > 1 or len({float(m.mask_threshold) for m in members}) > 1:
        raise ValueError("the mutual controllers of one U-Net batch must agree on ref_words (all or none) and on mask_threshold")
    side = int(round(P ** 0.5))
    if side * side != P:
        raise ValueError(f"mask-guided mutual self-attention needs a square token grid, got {P} tokens")
    if not all(m._sums_usable() for m in members):
        return None
    cache = owner.__dict__.setdefault("_mutual_cls", {"step": -1, "built": set(), "sides": [], "rows": {}})
    step = members[0].cur_step
    if side not in cache["sides"]:
        cache["sides"].append(side)
    if cache["step"] != step or side not in cache["built"]:
        sums = [m._blend_sums for m in members]
        lh, res2 = sums[0].shape[2], sums[0].shape[3]
        res = int(round(res2 ** 0.5))
        for s in cache["sides"]:
            if s not in cache["rows"] or cache["rows"][s].shape[0] != N or cache["rows"][s].device != device:
                cache["rows"][s] = torch.empty(N, s * s, dtype=torch.uint8, device=device)
        for i in range(0, len(cache["sides"]), MUTUAL_MAX_SIDES):
            sides = cache["sides"][i:i + MUTUAL_MAX_SIDES]
            outs = [cache["rows"][s] for s in sides]
            done = None
            if MUTUAL_KERNELS and device.type == "cuda":
                done = _hip.token_classes(sums, B, lh, res, float(members[0].mask_threshold), sides, outs, cfg=True)
            if done is None:
                for o, t in zip(outs, token_classes_torch(sums, float(members[0].mask_threshold), sides, cfg=True)):
                    o.copy_(t)
        cache["step"], cache["built"] = step, set(cache["sides"])
    return cache["rows"][side]


def _mutual_attention(owner, members, mutual, B, n0, q, k, v, out, heads, scale):
    """One mutual layer for the prompt groups of a U-Net call (AttentionControl._fused_attention):
    in both halves the edit rows of every active group read their source row's K and V.  The source
    rows -- with every group active the stride-B view 0, B, 2B, ... of the batch -- keep the kernel
    a plain AttentionStore launches for them (p2p_self_attn_fwd), so the source image has the bits
    it has without the controller; the edit rows run p2p_mutual_attn_fwd (or, with P2P_MUTUAL=0 or
    a shape it does not take, the torch lines)."""
    N, P = q.shape[0], q.shape[1]
    kv_src = list(range(N))
    for g, on in enumerate(mutual):
        if on:
            for half in (0, n0):
                first = half + g * B
                kv_src[first + 1:first + B] = [first] * (B - 1)
    active = [m for m, on in zip(members, mutual) if on]
    classes = _mutual_classes(owner, active, B, N, P, q.device) if len(active) == len(members) else None
    if len(active) != len(members) and any(m._ref_alpha is not None for m in active):
        raise ValueError("mask-guided mutual controllers of one U-Net batch must share start_step and start_layer")
    if all(mutual) and q.is_cuda:
        # the sources alone, on the plain kernel; the mutual launch skips them
        _hip.self_attn(q[::B], k[::B], v[::B], out[::B], heads, scale, compute=config.COMPUTE)
        edit_src = [-1 if s == n else s for n, s in enumerate(kv_src)]
    else:
        edit_src = kv_src
    obs = MUTUAL_OBSERVER
    if obs is not None:
        obs(dict(q=q, k=k, v=v, out=out, heads=heads, scale=scale, kv_src=list(kv_src), edit_src=list(edit_src),
                 token_class=classes, step=members[0].cur_step))
    if MUTUAL_KERNELS and q.is_cuda and _hip.mutual_attn(q, k, v, out, heads, scale, edit_src, token_class=classes,
                                           compute=config.COMPUTE) is not None:
        return out
    return mutual_attention_torch(q, k, v, heads, scale, edit_src, classes, out)


# Optional: called with the operands of every mutual launch before it runs (tests record them)
MUTUAL_OBSERVER = None


class MutualSelfAttentionControl(AttentionStore):
    """Mutual self-attention control (MasaCtrl): from denoising step ``start_step`` on, in the
    self-attention layers ``start_layer`` .. (layer = self-attention calls so far in the step, 0..15
    on the SD U-Net; the defaults are the paper's: the decoder's 32x32 and 64x64 layers), the edit
    prompts attend to the source prompt's keys and values with their own queries, in the uncond
    half (uncond edit rows read the uncond source row) and the cond half alike.  ``ref_words``: one
    word or tuple of words per prompt naming its object; the cross maps of those words give each
    token a foreground / background class (the running word sums of the five 16x16 cross layers,
    mean over layers and heads, min-max normalised, >= ``mask_threshold``) and an edit query then
    reads only the source keys of its own class.  None: unmasked mutual attention.

    Runs on the fused kernels (one launch per layer, also for a GroupBatch of these), on the torch
    lines for CPU tensors or with P2P_MUTUAL=0.  The probability-only ``forward(attn, ...)``
    protocol cannot express the edit: a ``forward`` call in an active layer raises."""

    _NATIVE = ("forward", "between_steps", "attention")
    store_self_maps = False

    def __init__(self, prompts, num_steps: int, start_step: int = 4, start_layer: int = 10, ref_words=None,
                 mask_threshold: float = 0.1, tokenizer=None, device=None):
        super().__init__()
        self.tokenizer = tokenizer or get_tokenizer()
        self.device = device or default_device()
        self.batch_size = len(prompts)
        self.num_steps, self.start_step, self.start_layer = int(num_steps), int(start_step), int(start_layer)
        self.ref_words, self.mask_threshold = ref_words, float(mask_threshold)
        self._ref_alpha = None
        if ref_words is not None:
            if len(ref_words) != len(prompts):
                raise ValueError("ref_words needs one word (or tuple of words) per prompt")
            alpha = _word_alpha_layers(prompts, ref_words, self.tokenizer)
            self._ref_alpha = alpha.reshape(len(prompts), -1).contiguous().to(self.device)
        self._blend_sums, self._blend_step, self._fold_steps = None, set(), 0

    # ------------------------------------------------------------------ window
    def _mutual_source(self, layer: int) -> bool:
        return self.batch_size > 1 and self.cur_step >= self.start_step and layer >= self.start_layer

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        if not is_cross:
            layer = self._fused_calls["self_layer"]
            self._fused_calls["self_layer"] += 1
            if self._mutual_source(layer):
                raise RuntimeError("mutual self-attention replaces keys and values: the probability-only "
                                   "forward(attn, ...) protocol cannot express it (use attention(q, k, v, ...))")
            return attn                     # (store_self_maps = False)
        return super().forward(attn, is_cross, place_in_unet)

    # ------------------------------------------------------------------ word sums -> classes
    def _folds_words(self) -> bool:
        return self._ref_alpha is not None

    def _blend_fold(self, key_idx, P, K, heads, device):
        """The p2p_group.blend_* tuple of this stored cross layer (AttentionControlEdit._blend_fold's
        layers and layout, one-hot alpha rows on ref_words, no substruct plane), or None."""
        slots = AttentionControlEdit.BLEND_SLOTS
        slot = slots.get(key_idx)
        alpha = self._ref_alpha
        if slot is None or alpha is None or P != 256 or alpha.shape != (self.batch_size, K):
            return None
        if alpha.device != device:
            alpha = self._ref_alpha = alpha.to(device)
        lh = len(slots) * heads
        shape = (self.batch_size, 2, lh, P)
        if self._blend_sums is None or self._blend_sums.shape != shape or self._blend_sums.device != device:
            self._blend_sums = torch.empty(shape, dtype=torch.float32, device=device)
            self._fold_steps = 0
        self._blend_step.add(slot)
        return self._blend_sums, alpha, None, slot * heads, lh

    def _sums_usable(self) -> bool:
        """Every layer of the sums holds maps: a complete earlier step, or this step's five folds."""
        n = len(AttentionControlEdit.BLEND_SLOTS)
        return self._blend_sums is not None and (self._fold_steps > 0 or len(self._blend_step) == n)

    def between_steps(self):
        first = len(self.attention_store) == 0
        complete = len(self._blend_step) == len(AttentionControlEdit.BLEND_SLOTS)
        self._fold_steps = (1 if first else self._fold_steps + 1) if complete and (first or self._fold_steps > 0) else 0
        self._blend_step = set()
        super().between_steps()

    def reset(self):
        super().reset()
        self._blend_step, self._fold_steps = set(), 0
        self.__dict__.pop("_mutual_cls", None)

    # ------------------------------------------------------------------ attention
    def attention(self, q, k, v, heads, scale, is_cross, place_in_unet, mask=None):
        if mask is not None:
            raise ValueError("MutualSelfAttentionControl does not take an attention mask")
        if _low_resource():
            raise ValueError("MutualSelfAttentionControl does not run with LOW_RESOURCE (it edits both CFG halves "
                             "of one U-Net call)")
        if q.is_cuda:
            return super().attention(q, k, v, heads, scale, is_cross, place_in_unet)
        out = self._torch_attention(q, k, v, heads, scale, is_cross, place_in_unet)
        self._advance_layer()
        return out

    def _torch_attention(self, q, k, v, heads, scale, is_cross, place_in_unet):
        """The whole call in torch lines (CPU tensors): plain attention with the AttentionStore's
        cross maps and word sums outside the window, the mutual edit inside it."""
        N, P, C = q.shape
        K, d = k.shape[1], C // heads
        n0 = N // 2
        B = N - n0
        if B != self.batch_size:
            raise ValueError(f"controller built for {self.batch_size} prompts got a batch of {B}")
        out = torch.empty_like(q)
        if not is_cross:
            layer = self._fused_calls["self_layer"]
            self._fused_calls["self_layer"] += 1
            if self._mutual_source(layer):
                return _mutual_attention(self, [self], [True], B, n0, q, k, v, out, heads, scale)
            return mutual_attention_torch(q, k, v, heads, scale, list(range(N)), None, out)
        qh = q.float().reshape(N, P, heads, d).transpose(1, 2)
        kh = k.float().reshape(N, K, heads, d).transpose(1, 2)
        vh = v.float().reshape(N, K, heads, d).transpose(1, 2)
        probs = (torch.einsum("nhpd,nhjd->nhpj", qh, kh) * scale).softmax(-1)
        if P <= MAX_STORED_QUERIES:
            key = f"{place_in_unet}_cross"
            idx = self._fused_calls[key]
            self._fused_calls[key] += 1
            cond = probs[n0:].reshape(B * heads, P, K)
            first = len(self.attention_store) == 0
            if first:
                self.step_store[key].append(cond.clone())
            else:
                self.attention_store[key][idx] += cond
            fold = self._blend_fold((key, idx), P, K, heads, q.device)
            if fold is not None:
                sums, alpha, _, col, _ = fold
                words = torch.einsum("bhpw,bw->bhp", probs[n0:], alpha)
                if first:
                    sums[:, 0, col:col + heads] = words
                else:
                    sums[:, 0, col:col + heads] += words
        return torch.einsum("nhpj,nhjd->nhpd", probs, vh).transpose(1, 2).reshape(N, P, C).to(q.dtype)


MutualSelfAttentionControl._P2P_LIB = True


# ============================================================================ prompt-group batching
class GroupBatch(AttentionControl):
    """Several prompt groups -- one controller each, built exactly as for a single group -- in
    ONE U-Net batch (BASELINE.json configs[2]: a batch of edit groups).  The reference runs one
    group per pipeline call (``self.batch_size = len(prompts)``, main.py:205); this build
    extension runs G of them per call: the U-Net batch is ``[uncond g0..gG-1 | cond g0..gG-1]``
    and every attention call is still ONE kernel launch, with one prompt-group descriptor per
    member (its edit program, its ``cross_replace_alpha[cur_step]`` row, its self-injection
    source, its AttentionStore slots).  Each member keeps its own counters and its own
    ``attention_store`` (views into one running-sum tensor per layer), so
    ``member.get_average_attention()``, ``aggregate_attention`` and LocalBlend work per group
    unchanged.  Members must take the fused path (library controllers, no LOW_RESOURCE)."""

    _NATIVE = ("__call__", "forward", "between_steps", "step_callback")

    def __init__(self, controllers, group_size: Optional[int] = None):
        super().__init__()
        self.members = list(controllers)
        if not self.members:
            raise ValueError("GroupBatch needs at least one controller")
        sizes = {getattr(m, "batch_size", None) for m in self.members}
        if group_size is None:
            if len(sizes) != 1 or None in sizes:
                raise ValueError("pass group_size= (members disagree on / do not know their batch size)")
            group_size = sizes.pop()
        self.group_size = int(group_size)
        for m in self.members:
            if not (isinstance(m, AttentionControl) and m.fused_supported()):
                raise ValueError(f"{type(m).__name__}: GroupBatch members must take the fused kernel path")
            # an edit controller's tables (program records, alpha rows, LocalBlend slices) are
            # sized by its own prompt count: it must equal the group size the kernels get
            if isinstance(m, AttentionControlEdit) and m.batch_size != self.group_size:
                raise ValueError(f"{type(m).__name__} was built for {m.batch_size} prompts, "
                                 f"GroupBatch groups have {self.group_size}")
        kinds = {isinstance(m, MutualSelfAttentionControl) for m in self.members}
        if kinds == {True, False} and any(isinstance(m, AttentionControlEdit) for m in self.members):
            raise ValueError("GroupBatch does not mix MutualSelfAttentionControl with AttentionControlEdit members: "
                             "a self-attention launch takes the source's probabilities or its keys and values, not both")
        storing = {isinstance(m, AttentionStore) for m in self.members}
        if len(storing) != 1:
            raise ValueError("mix of storing and non-storing controllers")
        if storing.pop() and len({bool(m.store_self_maps) for m in self.members}) != 1:
            raise ValueError("GroupBatch members disagree on store_self_maps")

    # counters: the composite counts like any controller and moves every member in lockstep
    @property
    def num_att_layers(self):
        return self._num_att_layers

    @num_att_layers.setter
    def num_att_layers(self, n):
        self._num_att_layers = n
        for m in getattr(self, "members", ()):
            m.num_att_layers = n

    def forward(self, attn, is_cross: bool, place_in_unet: str):
        raise NotImplementedError("GroupBatch runs only on the fused kernels (no materialised protocol)")

    def reset(self):
        super().reset()
        self.__dict__.pop("_mutual_cls", None)
        for m in getattr(self, "members", ()):
            m.reset()

    def step_callback(self, x_t):
        B = self.group_size
        return torch.cat([m.step_callback(x_t[g * B:(g + 1) * B]) for g, m in enumerate(self.members)])

    def fused_step_mask(self):
        fns = []
        for m in self.members:
            ok, fn = m.fused_step_mask()
            if not ok:
                return False, None
            fns.append(fn)
        if all(fn is None for fn in fns):
            return True, None
        B = self.group_size
        return True, lambda size: StepMask([fn(size).entries[0] if fn is not None else None for fn in fns], B)

    def attention(self, q, k, v, heads, scale, is_cross, place_in_unet, mask=None):
        if mask is not None:
            raise ValueError("GroupBatch does not take an attention mask")
        if _low_resource():
            raise ValueError("GroupBatch does not run with LOW_RESOURCE (one U-Net call per CFG half)")
        out = self._fused_attention(self.members, self.group_size, q, k, v, heads, scale, is_cross, place_in_unet)
        for m in self.members:
            m._advance_layer()
        self._advance_layer()
        return out


GroupBatch._P2P_LIB = True


def get_equalizer(text: str, word_select: Union[int, Tuple[int, ...]],
                  values: Union[List[float], Tuple[float, ...]], tokenizer=None):
    """main.py:281-290: one row per value, every selected word's columns set to ``values``."""
    tokenizer = tokenizer or get_tokenizer()
    if type(word_select) is int or type(word_select) is str:
        word_select = (word_select,)
    eq = torch.ones(len(values), MAX_NUM_WORDS)
    vals = torch.tensor(values, dtype=torch.float32)
    for word in word_select:
        eq[:, get_word_inds(text, word, tokenizer)] = vals
    return eq


def aggregate_attention(attention_store: AttentionStore, res: int, from_where: List[str], is_cross: bool,
                        select: int, prompts: Optional[List[str]] = None):
    """main.py:293-307 (``prompts`` is the reference's module global; defaults to the
    controller's batch size -- a plain AttentionStore has none, so pass ``prompts=`` there)."""
    n_prompts = len(prompts) if prompts is not None else getattr(attention_store, "batch_size", None)
    if n_prompts is None:
        raise ValueError(f"{type(attention_store).__name__} does not know its prompt count: pass prompts=")
    maps = attention_store.get_average_attention()
    picked = []
    for location in from_where:
        for item in maps[f"{location}_{'cross' if is_cross else 'self'}"]:
            if item.shape[1] == res ** 2:
                picked.append(item.reshape(n_prompts, -1, res, res, item.shape[-1])[select])
    out = torch.cat(picked, dim=0)
    return (out.sum(0) / out.shape[0]).cpu()


def reduce_maps(attention_store: AttentionStore, res: int, from_where: List[str], is_cross: bool,
                n_prompts: int) -> torch.Tensor:
    """aggregate_attention for every prompt at once, left on the device: the average over the
    stored layers at ``res`` and their heads of the step-averaged maps, [n_prompts, res, res, K]
    (main.py:296-307 with ``select`` = each prompt in turn; same sum order per prompt)."""
    maps = attention_store.get_average_attention()
    picked = []
    for location in from_where:
        for item in maps[f"{location}_{'cross' if is_cross else 'self'}"]:
            if item.shape[1] == res ** 2:
                picked.append(item.reshape(n_prompts, -1, res, res, item.shape[-1]))
    if not picked:
        raise ValueError(f"no stored {'cross' if is_cross else 'self'} maps at {res}x{res} in {from_where}")
    out = torch.cat(picked, dim=1)
    return out.sum(1) / out.shape[1]


# ============================================================================ the figures
def _picked_stores(attention_store: AttentionStore, res: int, from_where, is_cross: bool):
    """The running sums aggregate_attention would pick, in its order."""
    kind = "cross" if is_cross else "self"
    picked = []
    for location in from_where:
        for item in attention_store.attention_store.get(f"{location}_{kind}", ()):
            if item.shape[1] == res ** 2:
                picked.append(item)
    if not picked:
        why = " (the controller has store_self_maps = False)" if not (is_cross or attention_store.store_self_maps) else ""
        raise ValueError(f"no stored {kind} maps at {res}x{res} in {tuple(from_where)}{why}")
    return picked


def aggregate_attention_device(attention_store: AttentionStore, res: int, from_where: List[str], is_cross: bool,
                               select: int, prompts: Optional[List[str]] = None) -> torch.Tensor:
    """aggregate_attention (main.py:293-307) left on the stores' device, [res, res, K].  Stores that
    are f32, dense and on the GPU are read by one kernel (p2p_maps_aggregate): only the selected
    prompt's slabs, each term sum / cur_step, added in aggregate_attention's order -- no scaled copy
    of every stored map is made.  Anything else runs the torch lines on the picked maps."""
    n_prompts = len(prompts) if prompts is not None else getattr(attention_store, "batch_size", None)
    if n_prompts is None:
        raise ValueError(f"{type(attention_store).__name__} does not know its prompt count: pass prompts=")
    if not 0 <= select < n_prompts:
        raise IndexError(f"select {select} outside the {n_prompts} prompts")
    picked = _picked_stores(attention_store, res, from_where, is_cross)
    steps = attention_store.cur_step
    if steps >= 1:
        out = _hip.maps_aggregate(picked, n_prompts, select, steps)
        if out is not None:
            return out.reshape(res, res, out.shape[-1])

    def avg(item):     # get_average_attention's, on the picked maps only
        if item.is_cuda and item.dtype == torch.float32 and item.is_contiguous():
            return _hip.store_scale(item, float(steps))
        return item / steps
    out = torch.cat([avg(item).reshape(n_prompts, -1, res, res, item.shape[-1])[select] for item in picked], dim=0)
    return out.sum(0) / out.shape[0]


def _panel_expression(x: np.ndarray, size: int, minmax: bool) -> np.ndarray:
    """One map [res, res] as the reference draws it (main.py:320-324, :342-348), on the host."""
    from PIL import Image
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if minmax:
        x = x - x.min()
    m = x.max()
    if bool(torch.isnan(x).any()) or float(m) == 0.0 or bool(torch.isnan(m)):
        return np.zeros((size, size, 3), dtype=np.uint8)      # as the kernel: the reference's result is undefined
    grey = (255 * x / m).unsqueeze(-1).expand(*x.shape, 3).numpy().astype(np.uint8)
    return np.array(Image.fromarray(grey).resize((size, size)))


def cross_attention_panels(attention_store: AttentionStore, res: int, from_where: List[str], select: int = 0,
                           prompts: Optional[List[str]] = None, tokenizer=None, size: int = 256) -> np.ndarray:
    """The panels of show_cross_attention before their captions: for every token of
    ``prompts[select]``, its aggregated cross map as 255 * map / map.max(), grey RGB uint8, resized
    to ``size`` (main.py:314-324), [n_tokens, size, size, 3].  On the GPU one kernel renders all of
    them from the device aggregate (p2p_map_panels), byte for byte the NumPy + PIL result."""
    if prompts is None:
        raise ValueError("cross_attention_panels reads the tokens of prompts[select]: pass prompts=")
    tokenizer = tokenizer or get_tokenizer()
    n_tokens = len(tokenizer.encode(prompts[select]))
    maps = aggregate_attention_device(attention_store, res, from_where, True, select, prompts)
    K = maps.shape[-1]
    n_tokens = min(n_tokens, K)
    if maps.is_cuda:
        out = _hip.map_panels(maps.contiguous(), n_tokens, res, size, _hip.PANEL_MAX, 1, K)
        if out is not None:
            return out.cpu().numpy()
    maps = maps.float().cpu().numpy()
    return np.stack([_panel_expression(maps[:, :, i], size, False) for i in range(n_tokens)], axis=0)


def show_cross_attention(attention_store: AttentionStore, res: int, from_where: List[str], select: int = 0,
                         prompts: Optional[List[str]] = None, tokenizer=None):
    """main.py:310-327: the per-token cross-attention strip, each panel with its token's text under
    it.  Returns the PIL image (ptp_utils.view_images shows it in a notebook)."""
    from . import ptp_utils
    tokenizer = tokenizer or get_tokenizer()
    panels = cross_attention_panels(attention_store, res, from_where, select, prompts, tokenizer)
    tokens = tokenizer.encode(prompts[select])
    images = [ptp_utils.text_under_image(panel, tokenizer.decode([int(tokens[i])])) for i, panel in enumerate(panels)]
    return ptp_utils.view_images(np.stack(images, axis=0))


def self_attention_components(attention_store: AttentionStore, res: int, from_where: List[str], max_com: int = 10,
                              select: int = 0, prompts: Optional[List[str]] = None) -> np.ndarray:
    """The first ``max_com`` right singular vectors of the aggregated self-attention map
    [res^2, res^2] with every row centred by its mean (main.py:335-339), f32 [max_com, res^2].  The
    aggregate is made on the device; the SVD runs on the host (np.linalg.svd), as the reference's."""
    maps = aggregate_attention_device(attention_store, res, from_where, False, select, prompts)
    maps = maps.float().cpu().numpy().reshape((res ** 2, res ** 2))
    u, s, vh = np.linalg.svd(maps - np.mean(maps, axis=1, keepdims=True))
    return vh[:max_com]


def show_self_attention_comp(attention_store: AttentionStore, res: int, from_where: List[str], max_com: int = 10,
                             select: int = 0, prompts: Optional[List[str]] = None, size: int = 256):
    """main.py:330-350: the leading components of the self-attention map side by side, each as
    255 * (v - v.min()) / (v - v.min()).max(), grey RGB uint8, resized to ``size``.  With the stores
    on the GPU the strip [size, size * n, 3] is written by one kernel (p2p_map_panels, through its
    output strides).  Returns the PIL image.  Raises ValueError where no self map at ``res`` is
    stored (store_self_maps = False, or no such layer)."""
    from . import ptp_utils
    picked = _picked_stores(attention_store, res, from_where, False)
    vh = self_attention_components(attention_store, res, from_where, max_com, select, prompts)
    n = vh.shape[0]
    strip = None
    if picked[0].is_cuda:
        dev = picked[0].device
        canvas = torch.empty((size, size * n, 3), dtype=torch.uint8, device=dev)
        rows = torch.from_numpy(np.ascontiguousarray(vh, dtype=np.float32)).to(dev)
        out = _hip.map_panels(rows, n, res, size, _hip.PANEL_MINMAX, res * res, 1, out=canvas,
                              out_row_stride=3 * size * n, out_panel_stride=3 * size)
        if out is not None:
            strip = out.cpu().numpy()
    if strip is None:
        strip = np.concatenate([_panel_expression(vh[i].reshape(res, res), size, True) for i in range(n)], axis=1)
    return ptp_utils.view_images(strip)
