"""ctypes binding of ``libp2p_hip.so`` (C ABI: ``include/p2p_hip.h``).

This module is the only place the product talks to the device kernels.  There is no
fallback: if the shared library is missing or a call is rejected, it raises.  (The U-Net glue
functions at the end report a dtype or alignment the kernels do not take as None, so that the
module keeps its torch lines for f32 and odd shapes; everything else they are refused raises too.)
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import Optional, Sequence

import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libp2p_hip.so")
# A/B timing tools load the experiments build (make EXPERIMENTS=1 -> p2p_amd/exp/) instead; it is
# built from the same sources and stamped "<hash>-exp" (check_source_hash accepts it only here)
if os.environ.get("P2P_EXPERIMENTS_LIB") == "1":
    _LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exp", "libp2p_hip.so")
_lib = None

# Optional launch observer (bench.py times the dominant kernel and the map-store launches with HIP
# events through it): an object with before(kind, tensors, info) / after(kind, tensors, info),
# called around each launch; info = {"stored": entries whose maps are kept, "accumulate": bool}.
LAUNCH_OBSERVER = None

P2P_DTYPE_F32 = 0
P2P_DTYPE_BF16 = 1
P2P_DTYPE_F16 = 2
P2P_COMPUTE_BF16 = 0
P2P_COMPUTE_F32 = 1
MAX_BATCH = 64
MAX_GROUPS = 32
MAX_KEYS_CROSS = 96
PROGRAM_COLS = 128
PROGRAM_TMAX = 8
ABI_VERSION = 16
GROUP_F_R_ONLY = 2      # p2p_group.flags: every edit's blend coefficient A is 0 this call (P' = R)
GROUP_F_SHARED_KV = 4   # p2p_group.flags: every entry of the group has the first entry's K and V


class HipError(RuntimeError):
    """``code``: the library's P2P_E_* (or HIP) code, where a rejected call raised this."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class AttnTensors(ctypes.Structure):
    _fields_ = [
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("o", ctypes.c_void_p),
        ("q_row_stride", ctypes.c_int64), ("k_row_stride", ctypes.c_int64),
        ("v_row_stride", ctypes.c_int64), ("o_row_stride", ctypes.c_int64),
        ("q_batch_stride", ctypes.c_int64), ("k_batch_stride", ctypes.c_int64),
        ("v_batch_stride", ctypes.c_int64), ("o_batch_stride", ctypes.c_int64),
        ("n_batch", ctypes.c_int32), ("n_query", ctypes.c_int32), ("n_key", ctypes.c_int32),
        ("n_heads", ctypes.c_int32), ("head_dim", ctypes.c_int32),
        ("io_dtype", ctypes.c_int32), ("compute", ctypes.c_int32),
        ("scale", ctypes.c_float),
    ]


class Group(ctypes.Structure):
    _fields_ = [("first", ctypes.c_int32), ("count", ctypes.c_int32),
                ("program", ctypes.c_void_p), ("alpha", ctypes.c_void_p), ("flags", ctypes.c_int32),
                ("n_edits", ctypes.c_int32), ("blend_sums", ctypes.c_void_p), ("blend_alpha", ctypes.c_void_p),
                ("blend_sub", ctypes.c_void_p), ("blend_col", ctypes.c_int32), ("blend_lh", ctypes.c_int32)]


class BlendArgs(ctypes.Structure):
    _fields_ = [
        ("maps", ctypes.c_void_p * 8), ("n_maps", ctypes.c_int32), ("heads_per_map", ctypes.c_int32),
        ("n_prompts", ctypes.c_int32), ("n_words", ctypes.c_int32), ("map_res", ctypes.c_int32),
        ("alpha_layers", ctypes.c_void_p), ("substruct_layers", ctypes.c_void_p),
        ("th_pool", ctypes.c_float), ("th_sub", ctypes.c_float),
        ("x_t", ctypes.c_void_p), ("channels", ctypes.c_int32), ("lat_h", ctypes.c_int32),
        ("lat_w", ctypes.c_int32), ("word_sums", ctypes.c_void_p), ("mask_out", ctypes.c_void_p),
        ("word_sums_ready", ctypes.c_int32),
    ]


class TokenClassesArgs(ctypes.Structure):
    _fields_ = [
        ("sums", ctypes.c_void_p * MAX_GROUPS), ("n_groups", ctypes.c_int32), ("group_size", ctypes.c_int32),
        ("lh", ctypes.c_int32), ("res", ctypes.c_int32), ("threshold", ctypes.c_float), ("cfg", ctypes.c_int32),
        ("n_res", ctypes.c_int32), ("side", ctypes.c_int32 * 3), ("out", ctypes.c_void_p * 3),
    ]


# The five step argument structs (include/p2p_hip.h) share their head and their LocalBlend fields; the
# DDIM family carries its four factors between the two, the multistep forms their history after.
_STEP_HEAD = [
    ("eps", ctypes.c_void_p), ("eps_dtype", ctypes.c_int32), ("cfg", ctypes.c_int32),
    ("guidance", ctypes.c_float), ("x", ctypes.c_void_p), ("out", ctypes.c_void_p),
    ("n_prompts", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32),
    ("width", ctypes.c_int32),
]
_DDIM_FACTORS = [
    ("sqrt_beta_t", ctypes.c_float), ("sqrt_alpha_t", ctypes.c_float),
    ("sqrt_alpha_prev", ctypes.c_float), ("sqrt_one_minus_alpha_prev", ctypes.c_float),
]
_STEP_BLEND = [
    ("mask", ctypes.c_void_p), ("group_size", ctypes.c_int32), ("group_blend", ctypes.c_void_p),
    ("blend_sums", ctypes.c_void_p * MAX_GROUPS), ("blend_lh", ctypes.c_int32), ("blend_res", ctypes.c_int32),
    ("blend_th_pool", ctypes.c_float), ("blend_th_sub", ctypes.c_float), ("blend_sub", ctypes.c_int32),
]


class LatentArgs(ctypes.Structure):
    _fields_ = _STEP_HEAD + _DDIM_FACTORS + _STEP_BLEND


class PlmsArgs(ctypes.Structure):
    _fields_ = _STEP_HEAD + _STEP_BLEND + [
        ("hist", ctypes.c_void_p * 4), ("n_hist", ctypes.c_int32), ("w", ctypes.c_float * 5),
        ("hist_out", ctypes.c_void_p),
        ("sample_coeff", ctypes.c_float), ("eps_num", ctypes.c_float), ("eps_den", ctypes.c_float),
    ]


class DpmArgs(ctypes.Structure):
    _fields_ = _STEP_HEAD + _STEP_BLEND + [
        ("hist", ctypes.c_void_p * 1), ("n_hist", ctypes.c_int32), ("hist_out", ctypes.c_void_p),
        ("sigma_s", ctypes.c_float), ("alpha_s", ctypes.c_float), ("x_coeff", ctypes.c_float),
        ("m0_coeff", ctypes.c_float), ("diff_coeff", ctypes.c_float),
    ]


class DirectStepArgs(ctypes.Structure):
    _fields_ = LatentArgs._fields_ + [("offset", ctypes.c_void_p)]


class DdpmStepArgs(ctypes.Structure):
    _fields_ = LatentArgs._fields_ + [("sigma", ctypes.c_float), ("noise", ctypes.c_void_p)]


def _row_args_fields(out_name):
    """p2p_direct_offset_args / p2p_ddpm_noise_args: the same struct up to the name of its output."""
    return [
        ("eps", ctypes.c_void_p), ("eps_dtype", ctypes.c_int32), ("guidance", ctypes.c_float),
        ("x", ctypes.c_void_p), ("target", ctypes.c_void_p), ("coef", ctypes.c_void_p), (out_name, ctypes.c_void_p),
        ("R", ctypes.c_int32), ("n", ctypes.c_int32),
    ]


class DirectOffsetArgs(ctypes.Structure):
    _fields_ = _row_args_fields("offset")


class DdpmNoiseArgs(ctypes.Structure):
    _fields_ = _row_args_fields("noise")


class GroupNormArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("chan_add", ctypes.c_void_p), ("chan_add_stride", ctypes.c_int64),
        ("chan_bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
        ("y", ctypes.c_void_p), ("stats", ctypes.c_void_p),
        ("n", ctypes.c_int32), ("channels", ctypes.c_int32), ("hw", ctypes.c_int32), ("groups", ctypes.c_int32),
        ("eps", ctypes.c_float), ("act", ctypes.c_int32), ("y_layout", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class BiasResidualArgs(ctypes.Structure):
    _fields_ = [
        ("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("bias2", ctypes.c_void_p),
        ("out", ctypes.c_void_p), ("n", ctypes.c_int32), ("channels", ctypes.c_int32), ("hw", ctypes.c_int32),
        ("b_layout", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class Conv3x3Args(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("y", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("n", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("c_in", ctypes.c_int32),
        ("c_out", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class Conv3x3ExArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p),
        ("n", ctypes.c_int32), ("in_height", ctypes.c_int32), ("in_width", ctypes.c_int32), ("c_in", ctypes.c_int32),
        ("c_out", ctypes.c_int32), ("dtype", ctypes.c_int32), ("form", ctypes.c_int32),
    ]


class LinearArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p),
        ("y", ctypes.c_void_p), ("p_out", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("x_row_stride", ctypes.c_int64), ("res_row_stride", ctypes.c_int64),
        ("m", ctypes.c_int32), ("k", ctypes.c_int32), ("n", ctypes.c_int32), ("form", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
    ]


class Conv3x3PackArgs(ctypes.Structure):
    _fields_ = [
        ("weight", ctypes.c_void_p), ("packed", ctypes.c_void_p), ("c_in", ctypes.c_int32), ("c_out", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
    ]


class GegluArgs(ctypes.Structure):
    _fields_ = [
        ("inp", ctypes.c_void_p), ("out", ctypes.c_void_p), ("in_row_stride", ctypes.c_int64),
        ("out_row_stride", ctypes.c_int64), ("rows", ctypes.c_int32), ("d", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class GroupNormBwdArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("chan_add", ctypes.c_void_p), ("chan_add_stride", ctypes.c_int64),
        ("chan_bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
        ("dy", ctypes.c_void_p), ("stats", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("n", ctypes.c_int32), ("channels", ctypes.c_int32), ("hw", ctypes.c_int32), ("groups", ctypes.c_int32),
        ("act", ctypes.c_int32), ("dy_layout", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class GegluBwdArgs(ctypes.Structure):
    _fields_ = [
        ("inp", ctypes.c_void_p), ("dout", ctypes.c_void_p), ("din", ctypes.c_void_p),
        ("in_row_stride", ctypes.c_int64), ("rows", ctypes.c_int32), ("d", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class NchwToTokensArgs(ctypes.Structure):
    _fields_ = [
        ("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_int32), ("channels", ctypes.c_int32),
        ("hw", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class TimeEmbedArgs(ctypes.Structure):
    _fields_ = [
        ("timesteps", ctypes.c_void_p), ("timestep_stride", ctypes.c_int64), ("w1", ctypes.c_void_p),
        ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
        ("emb", ctypes.c_void_p), ("n", ctypes.c_int32), ("in_channels", ctypes.c_int32), ("d", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
    ]


class TimeProjArgs(ctypes.Structure):
    _fields_ = [
        ("emb", ctypes.c_void_p), ("table", ctypes.c_void_p), ("out", ctypes.c_void_p), ("n", ctypes.c_int32),
        ("d", ctypes.c_int32), ("segments", ctypes.c_int32), ("tiles", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class LayerNormArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("add", ctypes.c_void_p), ("add_bias", ctypes.c_void_p), ("gamma", ctypes.c_void_p),
        ("beta", ctypes.c_void_p), ("sum_out", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("rows", ctypes.c_int32), ("channels", ctypes.c_int32), ("eps", ctypes.c_float), ("dtype", ctypes.c_int32),
    ]


class BiasActArgs(ctypes.Structure):
    _fields_ = [
        ("inp", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("in_row_stride", ctypes.c_int64), ("out_row_stride", ctypes.c_int64),
        ("rows", ctypes.c_int32), ("d", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class ImageU8Args(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("out", ctypes.c_void_p), ("n", ctypes.c_int32), ("height", ctypes.c_int32),
        ("width", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


class ImageToModelArgs(ctypes.Structure):
    _fields_ = [
        ("img", ctypes.c_void_p), ("out", ctypes.c_void_p), ("n", ctypes.c_int32), ("height", ctypes.c_int32),
        ("width", ctypes.c_int32), ("dtype", ctypes.c_int32),
    ]


MAX_AGG_LAYERS = 16
RESIZE_TAPS = 5
PANEL_MAX_RES = 64
PANEL_MAX_SIDE = 512
PANEL_MAX, PANEL_MINMAX = 0, 1


class MapsAggregateArgs(ctypes.Structure):
    _fields_ = [
        ("stores", ctypes.c_void_p * MAX_AGG_LAYERS), ("heads", ctypes.c_int32 * MAX_AGG_LAYERS),
        ("n_layers", ctypes.c_int32), ("n_prompts", ctypes.c_int32), ("select", ctypes.c_int32),
        ("P", ctypes.c_int32), ("K", ctypes.c_int32), ("steps", ctypes.c_int32), ("out", ctypes.c_void_p),
    ]


class MapPanelsArgs(ctypes.Structure):
    _fields_ = [
        ("inp", ctypes.c_void_p), ("panel_stride", ctypes.c_int64), ("pixel_stride", ctypes.c_int64),
        ("coeffs", ctypes.c_void_p), ("bounds", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("out_row_stride", ctypes.c_int64), ("out_panel_stride", ctypes.c_int64),
        ("res", ctypes.c_int32), ("n", ctypes.c_int32), ("S", ctypes.c_int32), ("mode", ctypes.c_int32),
    ]


class NullLossArgs(ctypes.Structure):
    _fields_ = [
        ("eps_u", ctypes.c_void_p), ("eps_c", ctypes.c_void_p), ("eps_dtype", ctypes.c_int32),
        ("guidance", ctypes.c_float), ("x", ctypes.c_void_p), ("target", ctypes.c_void_p), ("coef", ctypes.c_void_p),
        ("active", ctypes.c_void_p), ("loss", ctypes.c_void_p), ("grad_eps_u", ctypes.c_void_p),
        ("B", ctypes.c_int32), ("n", ctypes.c_int32),
    ]


class NullAdamArgs(ctypes.Structure):
    _fields_ = [
        ("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
        ("exp_avg_sq", ctypes.c_void_p), ("lr", ctypes.c_void_p), ("step", ctypes.c_void_p),
        ("active", ctypes.c_void_p), ("loss", ctypes.c_void_p), ("threshold", ctypes.c_void_p),
        ("steps_run", ctypes.c_void_p), ("B", ctypes.c_int32), ("m", ctypes.c_int32),
        ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
    ]


def library_path() -> str:
    return _LIB_PATH


def lib():
    """Load the HIP library (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise HipError(f"{_LIB_PATH} is missing: run __graft_entry__.build() (make -C prompt-to-prompt_amd/csrc)")
        L = ctypes.CDLL(_LIB_PATH)
        i32, vp, f32, i64 = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_int64
        # every export returns int, but for these
        other = {"p2p_error_string": ctypes.c_char_p, "p2p_source_hash": ctypes.c_char_p,
                 "p2p_self_attn_kernel": ctypes.c_char_p, "p2p_cross_attn_kernel": ctypes.c_char_p,
                 "p2p_mutual_attn_kernel": ctypes.c_char_p,
                 "p2p_attn_bwd_workspace": ctypes.c_int64, "p2p_group_norm_stats_floats": ctypes.c_int64,
                 "p2p_group_norm_bwd_workspace_floats": ctypes.c_int64,
                 "p2p_conv3x3_workspace_floats": ctypes.c_int64,
                 "p2p_conv3x3_ex_workspace_floats": ctypes.c_int64,
                 "p2p_linear_workspace_floats": ctypes.c_int64}
        for fn in EXPORTED_SYMBOLS:
            getattr(L, fn).restype = other.get(fn, ctypes.c_int)
        L.p2p_error_string.argtypes = [ctypes.c_int]
        L.p2p_self_attn_kernel.argtypes = [ctypes.POINTER(AttnTensors), i32, i32]
        L.p2p_cross_attn_kernel.argtypes = [ctypes.POINTER(AttnTensors), vp, i32, i32]
        L.p2p_self_attn_fwd.argtypes = [ctypes.POINTER(AttnTensors), vp, vp, vp, i32, vp, vp]
        L.p2p_mutual_attn_fwd.argtypes = [ctypes.POINTER(AttnTensors), vp, vp, vp]
        L.p2p_mutual_attn_kernel.argtypes = [ctypes.POINTER(AttnTensors), i32]
        L.p2p_token_classes.argtypes = [ctypes.POINTER(TokenClassesArgs), vp]
        L.p2p_cross_attn_fwd.argtypes = [ctypes.POINTER(AttnTensors), vp, i32, vp, vp, i32, vp]
        L.p2p_attn_probs.argtypes = [ctypes.POINTER(AttnTensors), vp, vp, vp]
        L.p2p_attn_pv.argtypes = [ctypes.POINTER(AttnTensors), vp, vp]
        L.p2p_localblend.argtypes = [ctypes.POINTER(BlendArgs), vp]
        L.p2p_store_scale.argtypes = [vp, vp, f32, i64, vp]
        L.p2p_latent_step.argtypes = [ctypes.POINTER(LatentArgs), vp]
        L.p2p_plms_step.argtypes = [ctypes.POINTER(PlmsArgs), vp]
        L.p2p_dpm_step.argtypes = [ctypes.POINTER(DpmArgs), vp]
        L.p2p_direct_step.argtypes = [ctypes.POINTER(DirectStepArgs), vp]
        L.p2p_direct_offset.argtypes = [ctypes.POINTER(DirectOffsetArgs), vp]
        L.p2p_ddpm_step.argtypes = [ctypes.POINTER(DdpmStepArgs), vp]
        L.p2p_ddpm_noise.argtypes = [ctypes.POINTER(DdpmNoiseArgs), vp]
        L.p2p_attn_fwd_lse.argtypes = [ctypes.POINTER(AttnTensors), vp, vp]
        L.p2p_attn_bwd.argtypes = [ctypes.POINTER(AttnTensors), vp, vp, vp, vp, vp, vp, i32, vp, i64, vp]
        L.p2p_attn_bwd_workspace.argtypes = [ctypes.POINTER(AttnTensors)]
        L.p2p_group_norm.argtypes = [ctypes.POINTER(GroupNormArgs), vp]
        L.p2p_group_norm_stats_floats.argtypes = [i32, i32, i32, i32]
        L.p2p_bias_residual.argtypes = [ctypes.POINTER(BiasResidualArgs), vp]
        L.p2p_geglu.argtypes = [ctypes.POINTER(GegluArgs), vp]
        L.p2p_conv3x3.argtypes = [ctypes.POINTER(Conv3x3Args), vp]
        L.p2p_conv3x3_split.argtypes = [i32, i32, i32, i32, i32]
        L.p2p_conv3x3_workspace_floats.argtypes = [i32, i32, i32, i32, i32]
        L.p2p_conv3x3_pack.argtypes = [ctypes.POINTER(Conv3x3PackArgs), vp]
        L.p2p_conv3x3_ex.argtypes = [ctypes.POINTER(Conv3x3ExArgs), vp]
        L.p2p_conv3x3_ex_split.argtypes = [i32, i32, i32, i32, i32, i32]
        L.p2p_conv3x3_ex_workspace_floats.argtypes = [i32, i32, i32, i32, i32, i32]
        L.p2p_conv3x3_set_loop.argtypes = [i32]
        L.p2p_linear.argtypes = [ctypes.POINTER(LinearArgs), vp]
        L.p2p_linear_split.argtypes = [i32, i32, i32, i32]
        L.p2p_linear_workspace_floats.argtypes = [i32, i32, i32, i32]
        L.p2p_group_norm_bwd.argtypes = [ctypes.POINTER(GroupNormBwdArgs), vp]
        L.p2p_group_norm_bwd_workspace_floats.argtypes = [i32, i32, i32, i32]
        L.p2p_geglu_bwd.argtypes = [ctypes.POINTER(GegluBwdArgs), vp]
        L.p2p_nchw_to_tokens.argtypes = [ctypes.POINTER(NchwToTokensArgs), vp]
        L.p2p_time_embed.argtypes = [ctypes.POINTER(TimeEmbedArgs), vp]
        L.p2p_time_proj.argtypes = [ctypes.POINTER(TimeProjArgs), vp]
        L.p2p_causal_attn_fwd.argtypes = [ctypes.POINTER(AttnTensors), vp]
        L.p2p_layer_norm.argtypes = [ctypes.POINTER(LayerNormArgs), vp]
        L.p2p_bias_quick_gelu.argtypes = [ctypes.POINTER(BiasActArgs), vp]
        L.p2p_text_attn_fwd.argtypes = [ctypes.POINTER(AttnTensors), vp, vp]
        L.p2p_bias_gelu.argtypes = [ctypes.POINTER(BiasActArgs), vp]
        L.p2p_image_u8.argtypes = [ctypes.POINTER(ImageU8Args), vp]
        L.p2p_image_to_model.argtypes = [ctypes.POINTER(ImageToModelArgs), vp]
        L.p2p_maps_aggregate.argtypes = [ctypes.POINTER(MapsAggregateArgs), vp]
        L.p2p_map_panels.argtypes = [ctypes.POINTER(MapPanelsArgs), vp]
        L.p2p_null_loss.argtypes = [ctypes.POINTER(NullLossArgs), vp]
        L.p2p_null_adam.argtypes = [ctypes.POINTER(NullAdamArgs), vp]
        L.p2p_clock_probe.argtypes = [vp, i32, i32, vp]
        L.p2p_set_launch_events.argtypes = [vp, vp]
        if L.p2p_abi_version() != ABI_VERSION:
            raise HipError(f"libp2p_hip.so ABI {L.p2p_abi_version()} != {ABI_VERSION}")
        if not CONV_PIPE:
            L.p2p_conv3x3_set_loop(CONV_LOOP_TILE)
        _lib = L
    return _lib


def check_source_hash() -> str:
    """Raise unless the loaded library was built from the HIP sources in this tree (the Makefile
    stamps _srchash.source_hash() into it).  smoke() and the GPU tests call this, so a stale
    prebuilt libp2p_hip.so cannot pass for the current sources."""
    from . import _srchash
    built = lib().p2p_source_hash().decode()
    tree = _srchash.source_hash()
    if os.environ.get("P2P_EXPERIMENTS_LIB") == "1":
        tree += "-exp"   # the experiments build stamps its flavour (a production process refuses it)
    if built != tree:
        raise HipError(f"libp2p_hip.so was built from sources {built}, the tree has {tree}: rebuild "
                       f"(make -C prompt-to-prompt_amd/csrc)")
    return built


EXPORTED_SYMBOLS = ("p2p_abi_version", "p2p_source_hash", "p2p_error_string", "p2p_self_attn_fwd", "p2p_cross_attn_fwd",
                    "p2p_attn_probs", "p2p_attn_pv", "p2p_localblend", "p2p_store_scale", "p2p_latent_step",
                    "p2p_attn_fwd_lse", "p2p_attn_bwd", "p2p_attn_bwd_workspace", "p2p_clock_probe",
                    "p2p_set_launch_events", "p2p_group_norm", "p2p_bias_residual", "p2p_geglu",
                    "p2p_self_attn_kernel", "p2p_cross_attn_kernel", "p2p_plms_step", "p2p_image_u8",
                    "p2p_image_to_model", "p2p_group_norm_stats_floats", "p2p_causal_attn_fwd", "p2p_layer_norm",
                    "p2p_bias_quick_gelu", "p2p_text_attn_fwd", "p2p_bias_gelu", "p2p_maps_aggregate",
                    "p2p_map_panels", "p2p_null_loss", "p2p_null_adam", "p2p_group_norm_bwd",
                    "p2p_group_norm_bwd_workspace_floats", "p2p_geglu_bwd", "p2p_nchw_to_tokens", "p2p_time_embed",
                    "p2p_time_proj", "p2p_conv3x3", "p2p_conv3x3_split", "p2p_conv3x3_workspace_floats",
                    "p2p_conv3x3_pack", "p2p_dpm_step", "p2p_direct_step", "p2p_direct_offset",
                    "p2p_ddpm_step", "p2p_ddpm_noise", "p2p_mutual_attn_fwd", "p2p_mutual_attn_kernel",
                    "p2p_token_classes", "p2p_conv3x3_ex", "p2p_conv3x3_ex_split",
                    "p2p_conv3x3_ex_workspace_floats", "p2p_linear", "p2p_linear_split",
                    "p2p_linear_workspace_floats", "p2p_conv3x3_set_loop")


def clock_probe(out: torch.Tensor, ticks: int = 1000):
    """Measurement only (bench.py): one p2p_clock_probe launch on the current stream, one one-wave
    workgroup per row of ``out`` (int64 [n, 2] on the GPU: shader cycles, 100 MHz ticks); the
    shader clock of row w is out[w, 0] / out[w, 1] x 100 MHz, read after a synchronise."""
    _require_cuda(out)
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[1] != 2 or not out.is_contiguous():
        raise HipError("clock_probe needs a contiguous int64 [n, 2] tensor")
    _check(lib().p2p_clock_probe(out.data_ptr(), out.shape[0], int(ticks), _stream(out.device)), "p2p_clock_probe")
    return out


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().p2p_error_string(rc).decode()
        raise HipError(f"{what} failed: {msg} (code {rc})", rc)


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return P2P_DTYPE_F32
    if t.dtype == torch.bfloat16:
        return P2P_DTYPE_BF16
    if t.dtype == torch.float16:
        return P2P_DTYPE_F16
    raise HipError(f"unsupported attention dtype {t.dtype} (float32, bfloat16 or float16)")


_COMPUTE = {"bf16": P2P_COMPUTE_BF16, "f32": P2P_COMPUTE_F32}


def _require_cuda(*ts: Optional[torch.Tensor]):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise HipError("p2p_amd kernels need GPU tensors (no CPU path in the product)")


def make_tensors(q, k, v, o, heads: int, scale: float, compute: str) -> AttnTensors:
    """q/o: [N, P, H*d]; k/v: [N, K, H*d]; last dim contiguous."""
    ref = q if q is not None else v
    _require_cuda(q, k, v, o)
    for t in (q, k, v, o):
        if t is not None and (t.dim() != 3 or t.stride(-1) != 1):
            raise HipError("attention operands must be [batch, tokens, heads*dim] with a unit last stride")
    C = ref.shape[-1]
    if C % heads:
        raise HipError(f"channels {C} not divisible by heads {heads}")
    t = AttnTensors()

    def ptr(x):
        return x.data_ptr() if x is not None else None

    t.q, t.k, t.v, t.o = ptr(q), ptr(k), ptr(v), ptr(o)
    z = lambda x, i: x.stride(i) if x is not None else 0  # noqa: E731
    t.q_row_stride, t.k_row_stride, t.v_row_stride, t.o_row_stride = z(q, 1), z(k, 1), z(v, 1), z(o, 1)
    t.q_batch_stride, t.k_batch_stride, t.v_batch_stride, t.o_batch_stride = z(q, 0), z(k, 0), z(v, 0), z(o, 0)
    t.n_batch = ref.shape[0]
    t.n_query = (q if q is not None else o).shape[1]
    t.n_key = (k if k is not None else v).shape[1]
    t.n_heads = heads
    t.head_dim = C // heads
    t.io_dtype = _dtype_code(ref)
    t.compute = _COMPUTE[compute]
    t.scale = float(scale)
    return t


def _i32_array(vals: Sequence[int]):
    arr = (ctypes.c_int32 * len(vals))(*[int(x) for x in vals])
    return arr


def _lse_workspace(device, numel):
    """f32 scratch for the row log-sum-exp of a self launch that keeps maps: allocated per call
    from torch's caching allocator on the current stream (cheap), so launches on different
    streams -- or replays of a captured graph -- never share it; the allocator's stream
    ordering keeps it alive until the launch that reads it has run."""
    return torch.empty(numel, dtype=torch.float32, device=device)


def self_attn(q, k, v, o, heads, scale, compute="bf16", qk_src=None, store=None, store_slot=None,
              accumulate=False):
    t = make_tensors(q, k, v, o, heads, scale, compute)
    src = _i32_array(qk_src) if qk_src is not None else None
    slots = _i32_array(store_slot) if store_slot is not None else None
    if store is not None:
        _require_cuda(store)
        assert store.dtype == torch.float32 and store.is_contiguous()
    ws = None
    if store is not None and store_slot is not None and any(int(s) >= 0 for s in store_slot):
        ws = _lse_workspace(q.device, t.n_batch * t.n_heads * t.n_query).data_ptr()
    obs = LAUNCH_OBSERVER
    if obs is not None:
        info = {"stored": sum(1 for x in store_slot if int(x) >= 0) if ws is not None else 0,
                "accumulate": bool(accumulate)}
        obs.before("self", t, info)
    rc = lib().p2p_self_attn_fwd(ctypes.byref(t), src, store.data_ptr() if store is not None else None,
                                 slots, int(bool(accumulate)), ws, _stream(q.device))
    if obs is not None:
        obs.after("self", t, info)
    _check(rc, "p2p_self_attn_fwd")


def self_attn_kernel(t: AttnTensors, keeps_maps: bool = False, wants_lse: bool = False) -> Optional[str]:
    """The kernel p2p_self_attn_fwd (or, wants_lse, p2p_attn_fwd_lse) launches for these tensors, as
    the library names it (csrc/p2p_select.h), or None where it rejects them.  Launches nothing."""
    name = lib().p2p_self_attn_kernel(ctypes.byref(t), int(bool(keeps_maps)), int(bool(wants_lse)))
    return name.decode() if name is not None else None


def mutual_attn_kernel(t: AttnTensors, masked: bool = False) -> Optional[str]:
    """The same for p2p_mutual_attn_fwd; ``masked``: the call carries token classes."""
    name = lib().p2p_mutual_attn_kernel(ctypes.byref(t), int(bool(masked)))
    return name.decode() if name is not None else None


def mutual_attn(q, k, v, o, heads, scale, kv_src, token_class=None, compute="bf16"):
    """Mutual self-attention (p2p_mutual_attn_fwd): o[n] = softmax(q[n] k[s]^T * scale + M) v[s], s =
    kv_src[n] (None: the identity; s < 0: o[n] is left alone).  ``token_class``: None, or a contiguous
    uint8 [N, P] tensor of 0 / 1 on the operands' device -- for s != n a query reads only the keys of
    its own class in entry s (every key where s holds none of that class).  Returns ``o``, or None
    for what the library does not take (CPU tensors, a head dim without a kernel, a dtype or
    alignment it refuses): the caller then runs its torch lines.  Any other rejection raises."""
    if not (q.is_cuda and k.is_cuda and v.is_cuda and o.is_cuda):
        return None
    if q.dtype not in (torch.float32, torch.bfloat16, torch.float16) or q.shape[1] != k.shape[1]:
        return None
    if token_class is not None:
        if (token_class.dtype != torch.uint8 or token_class.shape != (q.shape[0], q.shape[1])
                or not token_class.is_contiguous() or token_class.device != q.device):
            raise HipError(f"mutual_attn: token_class must be a contiguous uint8 {tuple(q.shape[:2])} tensor on {q.device}")
    t = make_tensors(q, k, v, o, heads, scale, compute)
    src = _i32_array(kv_src) if kv_src is not None else None
    if src is not None and len(src) != t.n_batch:
        raise HipError(f"mutual_attn: kv_src has {len(src)} entries for a batch of {t.n_batch}")
    obs = LAUNCH_OBSERVER
    if obs is not None:
        info = {"stored": 0, "accumulate": False}
        obs.before("mutual", t, info)
    rc = lib().p2p_mutual_attn_fwd(ctypes.byref(t), src, token_class.data_ptr() if token_class is not None else None,
                                   _stream(q.device))
    if obs is not None:
        obs.after("mutual", t, info)
    if rc in (P2P_E_HEAD_DIM, P2P_E_DTYPE, P2P_E_ALIGN):
        return None
    _check(rc, "p2p_mutual_attn_fwd")
    return o


def token_classes(sums, group_size: int, lh: int, res: int, threshold: float, sides, outs, cfg: bool = True):
    """The token classes of mutual_attn from the running word sums (p2p_token_classes).  ``sums``:
    one contiguous f32 [group_size, 2, lh, res^2] tensor per prompt group (plane 0 is read);
    ``outs``: one contiguous uint8 [n_batch, side^2] tensor per side of ``sides`` (up to three),
    n_batch = groups * group_size * (2 if cfg else 1).  Fills and returns ``outs``; None for CPU
    tensors.  One launch, no host read, no allocation."""
    sums, sides, outs = list(sums), [int(s) for s in sides], list(outs)
    if not all(t.is_cuda for t in sums + outs):
        return None
    rows = len(sums) * group_size * (2 if cfg else 1)
    for s in sums:
        if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() != group_size * 2 * lh * res * res:
            raise HipError(f"token_classes: sums must be contiguous f32 [{group_size}, 2, {lh}, {res * res}]")
    if len(sides) != len(outs) or not 1 <= len(sides) <= 3 or len(sums) > MAX_GROUPS:
        raise HipError("token_classes: one output per side, one to three sides")
    for side, o in zip(sides, outs):
        if o.dtype != torch.uint8 or not o.is_contiguous() or o.shape != (rows, side * side):
            raise HipError(f"token_classes: the output of side {side} must be a contiguous uint8 [{rows}, {side * side}]")
    a = TokenClassesArgs()
    for g, s in enumerate(sums):
        a.sums[g] = s.data_ptr()
    a.n_groups, a.group_size, a.lh, a.res = len(sums), int(group_size), int(lh), int(res)
    a.threshold, a.cfg, a.n_res = float(threshold), int(bool(cfg)), len(sides)
    for r, (side, o) in enumerate(zip(sides, outs)):
        a.side[r], a.out[r] = side, o.data_ptr()
    _check(lib().p2p_token_classes(ctypes.byref(a), _stream(outs[0].device)), "p2p_token_classes")
    return outs


def cross_attn_kernel(t: AttnTensors, G, any_store: bool = False) -> Optional[str]:
    """The same for p2p_cross_attn_fwd with the Group array G."""
    name = lib().p2p_cross_attn_kernel(ctypes.byref(t), G, len(G), int(bool(any_store)))
    return name.decode() if name is not None else None


def _group_array(t: AttnTensors, groups):
    """The p2p_group array of cross_attn's group tuples."""
    G = (Group * len(groups))()
    for i, grp in enumerate(groups):
        first, count, prog, alpha = grp[:4]
        blend = grp[4] if len(grp) > 4 else None
        hints = int(grp[5]) if len(grp) > 5 else 0
        G[i].first, G[i].count = int(first), int(count)
        G[i].program = prog.data_ptr() if prog is not None else None
        G[i].alpha = alpha.data_ptr() if alpha is not None else None
        G[i].flags = (int(getattr(prog, "p2p_flags", 0)) | hints) if prog is not None else (hints & GROUP_F_SHARED_KV)
        G[i].n_edits = int(getattr(prog, "p2p_n_edits", 0)) if prog is not None else 0
        if blend is not None:
            sums, balpha, bsub, col, lh = blend
            _require_cuda(sums, balpha, bsub)
            assert sums.dtype == torch.float32 and sums.is_contiguous() and sums.numel() == count * 2 * lh * t.n_query
            assert balpha.dtype == torch.float32 and balpha.is_contiguous() and balpha.shape == (count, t.n_key)
            assert bsub is None or (bsub.dtype == torch.float32 and bsub.is_contiguous() and bsub.shape == balpha.shape)
            G[i].blend_sums, G[i].blend_alpha = sums.data_ptr(), balpha.data_ptr()
            G[i].blend_sub = bsub.data_ptr() if bsub is not None else None
            G[i].blend_col, G[i].blend_lh = int(col), int(lh)
    return G


def cross_group_dispatch(t: AttnTensors, groups) -> bool:
    """Whether p2p_cross_attn_fwd runs cross_group_kernel for these arguments (cross_attn's group
    tuples): the library's own answer (p2p_cross_attn_kernel; the rule is csrc/p2p_select.h's)."""
    G = _group_array(t, groups)
    # folded LocalBlend sums need every entry to store; the group / per-entry choice ignores stores
    any_store = any(len(grp) > 4 and grp[4] is not None for grp in groups)
    return (cross_attn_kernel(t, G, any_store) or "").startswith("cross_group_kernel")


SHARED_KV_HINTS = os.environ.get("P2P_SHARED_KV", "1") != "0"   # (A/B switch: 0 = never hint)


def shared_kv_hint(k, v, first: int, count: int) -> int:
    """GROUP_F_SHARED_KV when the K and V rows first .. first + count - 1 are bit-identical, as
    recorded on the projection views by ptp_utils._project (kv_row_classes); else 0."""
    rows = getattr(k, "_p2p_rows", None)
    if not SHARED_KV_HINTS or count < 2 or rows is None or getattr(v, "_p2p_rows", None) is not rows or len(rows) != k.shape[0]:
        return 0
    return GROUP_F_SHARED_KV if all(r == rows[first] for r in rows[first:first + count]) else 0


def cross_attn(q, k, v, o, heads, scale, groups, compute="bf16", store=None, store_slot=None,
               accumulate=False):
    """groups: list of (first, count, program_tensor|None, alpha_tensor|None[, blend[, hints]]) with
    blend = None or (sums [count, 2, lh, n_query] f32, alpha [count, n_key] f32, sub [count, n_key] |
    None, col, lh): LocalBlend's word sums folded into the store epilogue (p2p_group.blend_*); hints:
    per-call p2p_group.flags bits OR'ed onto the program's (GROUP_F_R_ONLY)."""
    t = make_tensors(q, k, v, o, heads, scale, compute)
    G = _group_array(t, groups)
    slots = _i32_array(store_slot) if store_slot is not None else None
    if store is not None:
        _require_cuda(store)
        assert store.dtype == torch.float32 and store.is_contiguous()
    obs = LAUNCH_OBSERVER
    if obs is not None:
        info = {"stored": sum(1 for x in store_slot if int(x) >= 0) if (store is not None and store_slot is not None)
                else 0, "accumulate": bool(accumulate), "n_groups": len(groups),
                "group_kernel": cross_group_dispatch(t, groups)}
        obs.before("cross", t, info)
    rc = lib().p2p_cross_attn_fwd(ctypes.byref(t), G, len(groups),
                                  store.data_ptr() if store is not None else None, slots,
                                  int(bool(accumulate)), _stream(q.device))
    if obs is not None:
        obs.after("cross", t, info)
    _check(rc, "p2p_cross_attn_fwd")


def attn_probs(q, k, heads, scale, probs, compute="bf16", key_mask=None):
    t = make_tensors(q, k, None, None, heads, scale, compute)
    _require_cuda(probs, key_mask)
    assert probs.dtype == torch.float32 and probs.is_contiguous()
    rc = lib().p2p_attn_probs(ctypes.byref(t), key_mask.data_ptr() if key_mask is not None else None,
                              probs.data_ptr(), _stream(q.device))
    _check(rc, "p2p_attn_probs")


def attn_pv(probs, v, o, heads, compute="bf16"):
    t = make_tensors(None, None, v, o, heads, 1.0, compute)
    t.n_query = o.shape[1]
    _require_cuda(probs)
    assert probs.dtype == torch.float32 and probs.is_contiguous()
    rc = lib().p2p_attn_pv(ctypes.byref(t), probs.data_ptr(), _stream(v.device))
    _check(rc, "p2p_attn_pv")


def localblend(maps, heads_per_map, alpha_layers, substruct_layers, th_pool, th_sub, x_t, word_sums,
               mask_out=None, word_sums_ready=False):
    """LocalBlend on device; x_t None with mask_out given = mask only (no blend).  word_sums_ready:
    word_sums already holds the folded word reductions (cross_attn blend); the maps are not read."""
    _require_cuda(x_t, alpha_layers, word_sums, substruct_layers, mask_out, *maps)
    a = BlendArgs()
    for i, m in enumerate(maps):
        assert m.dtype == torch.float32 and m.is_contiguous()
        a.maps[i] = m.data_ptr()
    B, W = alpha_layers.shape
    a.n_maps = len(maps)
    a.heads_per_map = heads_per_map
    a.n_prompts = B
    a.n_words = W
    a.map_res = int(round((maps[0].shape[1]) ** 0.5))
    a.alpha_layers = alpha_layers.data_ptr()
    a.substruct_layers = substruct_layers.data_ptr() if substruct_layers is not None else None
    a.th_pool, a.th_sub = float(th_pool), float(th_sub)
    if x_t is not None:
        assert x_t.dtype == torch.float32 and x_t.is_contiguous()
        a.x_t = x_t.data_ptr()
        a.channels, a.lat_h, a.lat_w = x_t.shape[1], x_t.shape[2], x_t.shape[3]
    else:
        assert mask_out is not None and mask_out.dtype == torch.uint8 and mask_out.is_contiguous()
        a.x_t = None
        a.channels, a.lat_h, a.lat_w = 0, mask_out.shape[-2], mask_out.shape[-1]
    a.word_sums = word_sums.data_ptr()
    a.mask_out = mask_out.data_ptr() if mask_out is not None else None
    a.word_sums_ready = int(bool(word_sums_ready))
    obs = LAUNCH_OBSERVER
    if obs is not None and hasattr(obs, "before_aux"):
        # algorithmic bytes: the word sums (or the maps) read, the mask written, x_t read + written
        LH, R2 = len(maps) * heads_per_map, a.map_res * a.map_res
        nbytes = (B * 2 * LH * R2 * 4 if word_sums_ready else sum(m.numel() * 4 for m in maps) + B * 2 * LH * R2 * 8)
        nbytes += B * a.lat_h * a.lat_w + (2 * x_t.numel() * 4 if x_t is not None else 0)
        obs.before_aux("localblend", nbytes)
    rc = lib().p2p_localblend(ctypes.byref(a), _stream((x_t if x_t is not None else mask_out).device))
    if obs is not None and hasattr(obs, "after_aux"):
        obs.after_aux("localblend")
    _check(rc, "p2p_localblend")


def store_scale(src: torch.Tensor, divisor: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _require_cuda(src)
    assert src.dtype == torch.float32 and src.is_contiguous()
    out = torch.empty_like(src) if out is None else out
    rc = lib().p2p_store_scale(src.data_ptr(), out.data_ptr(), float(divisor), src.numel(), _stream(src.device))
    _check(rc, "p2p_store_scale")
    return out


def _latent_common(a, eps, x, out, guidance, mask, group_size, group_blend, blend, what):
    """The fields the five step argument structs share (_STEP_HEAD and _STEP_BLEND), checked and
    filled; returns the bytes of folded word sums the launch reads (0: no ``blend``)."""
    _require_cuda(eps, x, out, mask)
    for t in (eps, x, out):
        assert t.is_contiguous()
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.shape == out.shape
    B, C, H, W = x.shape
    assert eps.shape[1:] == x.shape[1:] and eps.shape[0] == (2 * B if guidance is not None else B)
    a.eps, a.eps_dtype = eps.data_ptr(), _dtype_code(eps)
    a.cfg = 1 if guidance is not None else 0
    a.guidance = float(guidance) if guidance is not None else 0.0
    a.x, a.out = x.data_ptr(), out.data_ptr()
    a.n_prompts, a.channels, a.height, a.width = B, C, H, W
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape[-2:] == (H, W)
        a.mask = mask.data_ptr()
    else:
        a.mask = None
    a.group_size = int(group_size)
    if group_blend is not None:
        _require_cuda(group_blend)
        assert group_blend.dtype == torch.uint8 and group_blend.numel() * max(group_size, B) >= B
        a.group_blend = group_blend.data_ptr()
    else:
        a.group_blend = None
    sums_bytes = 0
    if blend is not None and any(e is not None for e in blend):
        if mask is not None or group_blend is not None or out.data_ptr() == x.data_ptr():
            raise HipError(f"{what}: blend (folded sums) excludes mask / group_blend and out aliasing x")
        gs = group_size if group_size > 0 else B
        if len(blend) != B // gs or len(blend) > MAX_GROUPS:
            raise HipError(f"{what}: {len(blend)} blend entries for {B // gs} prompt groups")
        ref = next(e for e in blend if e is not None)
        _, th_pool, th_sub, use_sub = ref
        lh, r2 = ref[0].shape[2], ref[0].shape[3]
        for g, e in enumerate(blend):
            if e is None:
                continue
            sums = e[0]
            _require_cuda(sums)
            if (sums.dtype != torch.float32 or not sums.is_contiguous() or tuple(sums.shape) != (gs, 2, lh, r2)
                    or tuple(e[1:]) != (th_pool, th_sub, use_sub)):
                raise HipError(f"{what}: blend sums must be f32 [group, 2, lh, res^2] with one threshold set")
            a.blend_sums[g] = sums.data_ptr()
            sums_bytes += sums.numel() * 4
        a.blend_lh, a.blend_res = int(lh), int(round(r2 ** 0.5))
        a.blend_th_pool, a.blend_th_sub, a.blend_sub = float(th_pool), float(th_sub), int(bool(use_sub))
    return sums_bytes


def _launch(fn, entry, a, device, kind=None, moved=(), more_bytes=0):
    """fn(a, the current stream) -- ``fn`` the library's ``entry`` -- checked; with ``kind`` and a
    LAUNCH_OBSERVER, reported to it as ``kind`` with the call's algorithmic bytes: every tensor of
    ``moved`` once per read or write (None entries skipped) plus ``more_bytes``.  One frame and no
    byte count without an observer: the call is on the host's path between two launches."""
    obs = LAUNCH_OBSERVER if kind is not None else None
    if obs is not None and hasattr(obs, "before_aux"):
        obs.before_aux(kind, sum(t.numel() * t.element_size() for t in moved if t is not None) + more_bytes)
    rc = fn(ctypes.byref(a), _stream(device))
    if obs is not None and hasattr(obs, "after_aux"):
        obs.after_aux(kind)
    _check(rc, entry)


def _group_rows(what, name, rows, x, group_size):
    """The data pointer of a per-group row tensor (direct_step's offset, ddpm_step's noise), checked:
    contiguous f32 [B / group_size, C, H, W], one row with group_size = 0."""
    _require_cuda(rows)
    groups = x.shape[0] // group_size if group_size > 0 else 1
    if rows.dtype != torch.float32 or not rows.is_contiguous() or tuple(rows.shape) != (groups, *x.shape[1:]):
        raise HipError(f"{what}: {name} must be contiguous f32 {(groups, *x.shape[1:])}, got "
                       f"{rows.dtype} {tuple(rows.shape)}")
    return rows.data_ptr()


def _set_history(what, a, x, hist, hist_out):
    """The multistep forms' history fields (a: PlmsArgs or DpmArgs), checked and filled: ``hist`` the
    stored tensors the plan reads, ``hist_out`` None or the tensor that receives this call's."""
    _require_cuda(hist_out, *hist)
    for h in tuple(hist) + ((hist_out,) if hist_out is not None else ()):
        if h.dtype != torch.float32 or not h.is_contiguous() or h.shape != x.shape:
            raise HipError(f"{what}: history tensors must be contiguous f32 of the latent's shape")
    for i, h in enumerate(hist):
        a.hist[i] = h.data_ptr()
    a.n_hist = len(hist)
    a.hist_out = hist_out.data_ptr() if hist_out is not None else None


def latent_step(eps, x, out, coeffs, guidance=None, mask=None, group_size=0, group_blend=None, blend=None):
    """Fused CFG + DDIM step + LocalBlend blend (p2p_latent_step).  eps: [2B or B, C, H, W]
    (f32/bf16/f16, uncond block first when guidance is given); x, out: f32 [B, C, H, W] (out may be
    x unless ``blend`` is given); coeffs: (sqrt_beta_t, sqrt_alpha_t, sqrt_alpha_prev,
    sqrt_one_minus_alpha_prev) floats; mask: uint8 [B, H, W] or None; group_size: prompts per
    prompt group (0 = one group), with group_blend (uint8 [B / group_size] or None = every group)
    selecting the groups that blend.  blend: instead of ``mask``, one entry per prompt group --
    None (no blend) or (sums f32 [group prompts, 2, lh, res^2], th_pool, th_sub, use_substruct):
    the folded LocalBlend word sums the mask is built from in the same launch."""
    a = LatentArgs()
    sums_bytes = _latent_common(a, eps, x, out, guidance, mask, group_size, group_blend, blend, "latent_step")
    a.sqrt_beta_t, a.sqrt_alpha_t, a.sqrt_alpha_prev, a.sqrt_one_minus_alpha_prev = [float(c) for c in coeffs]
    _launch(lib().p2p_latent_step, "p2p_latent_step", a, x.device, "latent_blend" if sums_bytes else "latent_step",
            (eps, x, out, mask), sums_bytes)
    return out


def plms_step(eps, x, out, plan, guidance=None, mask=None, group_size=0, group_blend=None, blend=None,
              hist=(), hist_out=None):
    """Fused CFG + PLMS step + LocalBlend blend (p2p_plms_step): latent_step's arguments with, in
    place of the DDIM coefficients, ``plan`` -- a pndm.StepPlan (weights, n_hist, sample_coeff,
    eps_num, eps_den) -- and the scheduler's history: ``hist`` the stored f32 [B, C, H, W] model
    outputs the plan reads, newest first, ``hist_out`` None or the f32 tensor that receives this
    call's CFG-combined eps.  x is the sample the plan steps from."""
    a = PlmsArgs()
    sums_bytes = _latent_common(a, eps, x, out, guidance, mask, group_size, group_blend, blend, "plms_step")
    n_hist = int(plan.n_hist)
    if n_hist != len(hist) or len(plan.weights) != n_hist + 1 or n_hist > 4:
        raise HipError(f"plms_step: {len(hist)} history tensors for a plan of {n_hist} (weights {len(plan.weights)})")
    _set_history("plms_step", a, x, hist, hist_out)
    for i, w in enumerate(plan.weights):
        a.w[i] = float(w)
    a.sample_coeff, a.eps_num, a.eps_den = float(plan.sample_coeff), float(plan.eps_num), float(plan.eps_den)
    _launch(lib().p2p_plms_step, "p2p_plms_step", a, x.device, "plms_blend" if sums_bytes else "plms_step",
            (eps, x, out, mask, *hist, hist_out), sums_bytes)
    return out


def dpm_step(eps, x, out, plan, guidance=None, mask=None, group_size=0, group_blend=None, blend=None,
             hist=(), hist_out=None):
    """Fused CFG + DPM-Solver++ (2M) step + LocalBlend blend (p2p_dpm_step): latent_step's arguments
    with, in place of the DDIM coefficients, ``plan`` -- a dpm.StepPlan (n_hist, sigma_s, alpha_s,
    x_coeff, m0_coeff, diff_coeff) -- and the scheduler's history: ``hist`` empty or the previous
    call's f32 [B, C, H, W] data prediction, ``hist_out`` None or the f32 tensor that receives this
    call's."""
    a = DpmArgs()
    sums_bytes = _latent_common(a, eps, x, out, guidance, mask, group_size, group_blend, blend, "dpm_step")
    n_hist = int(plan.n_hist)
    if n_hist != len(hist) or n_hist > 1:
        raise HipError(f"dpm_step: {len(hist)} history tensors for a plan of {n_hist}")
    _set_history("dpm_step", a, x, hist, hist_out)
    a.sigma_s, a.alpha_s, a.x_coeff = float(plan.sigma_s), float(plan.alpha_s), float(plan.x_coeff)
    a.m0_coeff, a.diff_coeff = float(plan.m0_coeff), float(plan.diff_coeff)
    _launch(lib().p2p_dpm_step, "p2p_dpm_step", a, x.device, "dpm_blend" if sums_bytes else "dpm_step",
            (eps, x, out, mask, *hist, hist_out), sums_bytes)
    return out


def direct_step(eps, x, out, coeffs, offset, guidance=None, mask=None, group_size=0, group_blend=None, blend=None):
    """latent_step for Direct Inversion's edit loop (p2p_direct_step): the same arguments and, after
    the blend, ``offset`` -- f32 [B / group_size, C, H, W], one row with group_size = 0 -- added to
    each prompt group's first prompt.  The other prompts blend towards the un-offset source."""
    a = DirectStepArgs()
    sums_bytes = _latent_common(a, eps, x, out, guidance, mask, group_size, group_blend, blend, "direct_step")
    a.sqrt_beta_t, a.sqrt_alpha_t, a.sqrt_alpha_prev, a.sqrt_one_minus_alpha_prev = [float(c) for c in coeffs]
    a.offset = _group_rows("direct_step", "offset", offset, x, group_size)
    _launch(lib().p2p_direct_step, "p2p_direct_step", a, x.device, "direct_blend" if sums_bytes else "direct_step",
            (eps, x, out, mask, offset), sums_bytes)
    return out


def ddpm_step(eps, x, out, coeffs, noise, guidance=None, mask=None, group_size=0, group_blend=None, blend=None):
    """latent_step with a variance noise, for the DDPM-inversion edit loop (p2p_ddpm_step): the same
    arguments with ``coeffs`` the five of DDIMScheduler.ddpm_coeffs -- (sqrt(1 - a_t), sqrt(a_t),
    sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma) -- and ``noise`` f32 [B / group_size, C, H, W],
    one row with group_size = 0: sigma * noise[g] is added to every prompt of group g before the
    blend."""
    a = DdpmStepArgs()
    sums_bytes = _latent_common(a, eps, x, out, guidance, mask, group_size, group_blend, blend, "ddpm_step")
    (a.sqrt_beta_t, a.sqrt_alpha_t, a.sqrt_alpha_prev, a.sqrt_one_minus_alpha_prev,
     a.sigma) = [float(c) for c in coeffs]
    a.noise = _group_rows("ddpm_step", "noise", noise, x, group_size)
    _launch(lib().p2p_ddpm_step, "p2p_ddpm_step", a, x.device, "ddpm_blend" if sums_bytes else "ddpm_step",
            (eps, x, out, mask, noise), sums_bytes)
    return out


def _row_pass(what, a, out_name, width, eps, x, target, coef, guidance, out, observed):
    """p2p_<what> for R rows (a: its empty argument struct): eps [2R, ...] (f32 / bf16 / f16, uncond
    block first), x / target / out f32 [R, ...] of eps's row shape, coef f32 [R, width] on the
    device.  Launches on the current stream."""
    _require_cuda(eps, x, target, coef, out)
    R = x.shape[0]
    n = x.numel() // max(R, 1)
    _dense(f"{what} eps", eps, eps.dtype, 2 * R * n)
    for name, t in (("x", x), ("target", target), (out_name, out)):
        _dense(f"{what} {name}", t, torch.float32, R * n)
    _dense(f"{what} coef", coef, torch.float32, width * R)
    a.eps, a.eps_dtype, a.guidance = eps.data_ptr(), _dtype_code(eps), float(guidance)
    a.x, a.target, a.coef = x.data_ptr(), target.data_ptr(), coef.data_ptr()
    setattr(a, out_name, out.data_ptr())
    a.R, a.n = R, n
    _launch(getattr(lib(), f"p2p_{what}"), f"p2p_{what}", a, x.device, what if observed else None,
            (eps, x, target, out, coef))
    return out


def direct_offset(eps, x, target, coef, guidance: float, offset):
    """p2p_direct_offset for R rows (see _row_pass), coef f32 [R, 4]: each row's prev_coeffs.
    offset[r] = target[r] - prev_step(guided eps[r], x[r])."""
    return _row_pass("direct_offset", DirectOffsetArgs(), "offset", 4, eps, x, target, coef, guidance, offset, False)


def ddpm_noise(eps, x, target, coef, guidance: float, noise):
    """p2p_ddpm_noise for R rows (see _row_pass), coef f32 [R, 5]: each row's ddpm_coeffs.
    noise[r] = (target[r] - mu(guided eps[r], x[r])) / sigma[r], zeros where sigma[r] is 0.  The one of
    the two that reports to LAUNCH_OBSERVER ("ddpm_noise")."""
    return _row_pass("ddpm_noise", DdpmNoiseArgs(), "noise", 5, eps, x, target, coef, guidance, noise, True)


def attn_fwd_lse(q, k, v, o, heads, scale, lse):
    """O and the row log-sum-exp (log2 domain, scale folded) for the backward pass."""
    t = make_tensors(q, k, v, o, heads, scale, "bf16")
    _require_cuda(lse)
    assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == t.n_batch * heads * t.n_query
    _check(lib().p2p_attn_fwd_lse(ctypes.byref(t), lse.data_ptr(), _stream(q.device)), "p2p_attn_fwd_lse")


def attn_bwd(q, k, v, o, dout, lse, heads, scale, dq, dk, dv, delta, workspace=None):
    """dq (q's dtype and layout); dk / dv packed [N, K, H*d], written, in k's dtype or f32.
    workspace: p2p_attn_bwd_workspace bytes (allocated here when None)."""
    for x in (q, k, v, o, dout, dq, dk, dv):
        assert x.is_contiguous()
    assert dout.shape == o.shape == q.shape and dq.shape == q.shape
    assert dk.shape == k.shape and dv.shape == v.shape and dk.dtype == dv.dtype
    assert dk.dtype in (k.dtype, torch.float32)
    t = make_tensors(q, k, v, o, heads, scale, "bf16")
    _require_cuda(dout, lse, delta, dq, dk, dv)
    need = int(lib().p2p_attn_bwd_workspace(ctypes.byref(t)))
    if need > 0 and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_ptr = workspace.data_ptr() if need > 0 else None
    kv_f32 = int(dk.dtype == torch.float32)
    rc = lib().p2p_attn_bwd(ctypes.byref(t), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                            dk.data_ptr(), dv.data_ptr(), kv_f32, ws_ptr, need, _stream(q.device))
    _check(rc, "p2p_attn_bwd")


def _dense(what: str, t: torch.Tensor, dtype, numel: int):
    if t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
        raise HipError(f"{what}: needs a contiguous {dtype} tensor of {numel} elements, "
                       f"got {t.dtype} {tuple(t.shape)}")


def null_loss(eps_u, eps_c, x, target, coef, guidance: float, active, loss, grad_eps_u):
    """p2p_null_loss for B images: eps_u / eps_c / grad_eps_u [B, ...] in one dtype (f32 or bf16),
    x / target f32 of the same shape, coef f32 [4] on the device, active uint8 [B]; writes loss
    f32 [B] and grad_eps_u.  Launches on the current stream, nothing is read back."""
    _require_cuda(eps_u, eps_c, x, target, coef, active, loss, grad_eps_u)
    B = eps_u.shape[0]
    n = eps_u.numel() // max(B, 1)
    for name, t, dt in (("eps_u", eps_u, eps_u.dtype), ("eps_c", eps_c, eps_u.dtype), ("x", x, torch.float32),
                        ("target", target, torch.float32), ("grad_eps_u", grad_eps_u, eps_u.dtype)):
        _dense(f"null_loss {name}", t, dt, B * n)
    _dense("null_loss coef", coef, torch.float32, 4)
    _dense("null_loss active", active, torch.uint8, B)
    _dense("null_loss loss", loss, torch.float32, B)
    a = NullLossArgs()
    a.eps_u, a.eps_c, a.eps_dtype, a.guidance = eps_u.data_ptr(), eps_c.data_ptr(), _dtype_code(eps_u), float(guidance)
    a.x, a.target, a.coef, a.active = x.data_ptr(), target.data_ptr(), coef.data_ptr(), active.data_ptr()
    a.loss, a.grad_eps_u, a.B, a.n = loss.data_ptr(), grad_eps_u.data_ptr(), B, n
    _check(lib().p2p_null_loss(ctypes.byref(a), _stream(x.device)), "p2p_null_loss")
    return loss, grad_eps_u


def null_adam(param, grad, exp_avg, exp_avg_sq, lr, step, active, loss, threshold, steps_run,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """p2p_null_adam: torch.optim.Adam's step on param [B, ...] f32 for every image whose active
    byte is set, then the early stop (active[b] &= !(loss[b] < threshold[b])); lr is an f32 device
    scalar, step / steps_run int32 [B], active uint8 [B], loss / threshold f32 [B].  All in place."""
    _require_cuda(param, grad, exp_avg, exp_avg_sq, lr, step, active, loss, threshold, steps_run)
    B = param.shape[0]
    m = param.numel() // max(B, 1)
    for name, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _dense(f"null_adam {name}", t, torch.float32, B * m)
    _dense("null_adam lr", lr, torch.float32, 1)
    for name, t, dt in (("step", step, torch.int32), ("steps_run", steps_run, torch.int32),
                        ("active", active, torch.uint8), ("loss", loss, torch.float32),
                        ("threshold", threshold, torch.float32)):
        _dense(f"null_adam {name}", t, dt, B)
    a = NullAdamArgs()
    a.param, a.grad, a.exp_avg, a.exp_avg_sq = param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    a.lr, a.step, a.active, a.loss = lr.data_ptr(), step.data_ptr(), active.data_ptr(), loss.data_ptr()
    a.threshold, a.steps_run, a.B, a.m = threshold.data_ptr(), steps_run.data_ptr(), B, m
    a.beta1, a.beta2, a.eps = float(beta1), float(beta2), float(eps)
    _check(lib().p2p_null_adam(ctypes.byref(a), _stream(param.device)), "p2p_null_adam")


# -- U-Net glue (p2p_unet.hip).  Each returns its output, or None when the library reports the
# arguments unsupported (dtype, alignment) or the tensors are not dense: the caller then runs
# its torch lines.  Any other rejection raises.
P2P_E_HEAD_DIM, P2P_E_DTYPE, P2P_E_KEYS, P2P_E_ALIGN = -2, -3, -4, -6
ACT_NONE, ACT_SILU = 0, 1
LAYOUT_NCHW, LAYOUT_TOKENS = 0, 1


def _glue_rc(rc: int, what: str) -> bool:
    if rc in (P2P_E_DTYPE, P2P_E_ALIGN):
        return False
    _check(rc, what)
    return True


def _glue_dtype(t: torch.Tensor) -> int:
    return {torch.bfloat16: P2P_DTYPE_BF16, torch.float16: P2P_DTYPE_F16}.get(t.dtype, P2P_DTYPE_F32)


def _vec(t: Optional[torch.Tensor], like: torch.Tensor, numel: int):
    """A dense per-channel vector in ``like``'s dtype (or None)."""
    if t is None:
        return None
    if t.dtype != like.dtype or not t.is_contiguous() or t.numel() != numel:
        raise HipError("per-channel operand must be dense, in the tensor's dtype")
    return t


def group_norm(x, gamma, beta, groups: int, eps: float, silu: bool = False, tokens: bool = False,
               chan_add=None, chan_bias=None, return_stats: bool = False):
    """act(GroupNorm(x + chan_add + chan_bias) * gamma + beta) (p2p_group_norm).  x: [N, C, H, W];
    chan_add: [N, C] or [C]; chan_bias: [C]; returns [N, C, H, W], or [N, H*W, C] with ``tokens``.
    With ``return_stats`` it returns (y, stats): the f32 workspace whose first N * groups * 2
    elements are the {mean, rstd} pairs, which group_norm_bwd reads."""
    _require_cuda(x, gamma, beta, chan_add, chan_bias)
    if x.dim() != 4 or not x.is_contiguous():
        return None
    N, C, H, W = x.shape
    a = GroupNormArgs()
    a.x = x.data_ptr()
    if chan_add is not None:
        per_n = chan_add.dim() == 2
        _vec(chan_add, x, N * C if per_n else C)
        a.chan_add, a.chan_add_stride = chan_add.data_ptr(), C if per_n else 0
    if chan_bias is not None:
        a.chan_bias = _vec(chan_bias, x, C).data_ptr()
    a.gamma, a.beta = _vec(gamma, x, C).data_ptr(), _vec(beta, x, C).data_ptr()
    y = x.new_empty((N, H * W, C) if tokens else (N, C, H, W))
    if groups < 1 or C % groups:
        raise HipError(f"group_norm: {C} channels in {groups} groups")
    # {mean, rstd} per slab, and the per-chunk partials of the split statistics for large slabs
    n_stats = int(lib().p2p_group_norm_stats_floats(N, C, H * W, int(groups)))
    stats = torch.empty(max(n_stats, N * groups * 2), dtype=torch.float32, device=x.device)
    a.y, a.stats = y.data_ptr(), stats.data_ptr()
    a.n, a.channels, a.hw, a.groups = N, C, H * W, int(groups)
    a.eps = float(eps)
    a.act = ACT_SILU if silu else ACT_NONE
    a.y_layout = LAYOUT_TOKENS if tokens else LAYOUT_NCHW
    a.dtype = _glue_dtype(x)
    if not _glue_rc(lib().p2p_group_norm(ctypes.byref(a), _stream(x.device)), "p2p_group_norm"):
        return None
    return (y, stats) if return_stats else y


def group_norm_bwd(dy, x, stats, gamma, beta, groups: int, silu: bool = False, tokens: bool = False,
                   chan_add=None, chan_bias=None):
    """The gradient of group_norm with respect to x (p2p_group_norm_bwd) from its inputs, the
    ``stats`` it returned and ``dy`` (dense, in the layout of the forward's output).  A shape the
    library does not serve raises: the caller decides that before the forward."""
    _require_cuda(dy, x, stats, gamma, beta, chan_add, chan_bias)
    N, C, H, W = x.shape
    if not x.is_contiguous() or not dy.is_contiguous() or dy.dtype != x.dtype or \
            tuple(dy.shape) != ((N, H * W, C) if tokens else (N, C, H, W)):
        raise HipError(f"group_norm_bwd: dy {tuple(dy.shape)} {dy.dtype} does not match x {tuple(x.shape)} {x.dtype}")
    if stats.dtype != torch.float32 or not stats.is_contiguous() or stats.numel() < N * int(groups) * 2:
        raise HipError("group_norm_bwd: stats must be the forward's f32 workspace")
    a = GroupNormBwdArgs()
    a.x, a.dy, a.stats = x.data_ptr(), dy.data_ptr(), stats.data_ptr()
    if chan_add is not None:
        per_n = chan_add.dim() == 2
        _vec(chan_add, x, N * C if per_n else C)
        a.chan_add, a.chan_add_stride = chan_add.data_ptr(), C if per_n else 0
    if chan_bias is not None:
        a.chan_bias = _vec(chan_bias, x, C).data_ptr()
    a.gamma, a.beta = _vec(gamma, x, C).data_ptr(), _vec(beta, x, C).data_ptr()
    n_ws = int(lib().p2p_group_norm_bwd_workspace_floats(N, C, H * W, int(groups)))
    if n_ws < 1:
        raise HipError(f"group_norm_bwd: {C} channels in {groups} groups")
    ws = torch.empty(n_ws, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    a.dx, a.workspace = dx.data_ptr(), ws.data_ptr()
    a.n, a.channels, a.hw, a.groups = N, C, H * W, int(groups)
    a.act = ACT_SILU if silu else ACT_NONE
    a.dy_layout = LAYOUT_TOKENS if tokens else LAYOUT_NCHW
    a.dtype = _glue_dtype(x)
    _check(lib().p2p_group_norm_bwd(ctypes.byref(a), _stream(x.device)), "p2p_group_norm_bwd")
    return dx


def bias_residual(a_nchw, b, bias=None, bias2=None, tokens: bool = False):
    """a + b + bias + bias2 as [N, C, H, W] (p2p_bias_residual).  a_nchw: [N, C, H, W]; b: the same
    shape, or [N, H*W, C] with ``tokens``; biases: [C] or None."""
    _require_cuda(a_nchw, b, bias, bias2)
    if a_nchw.dim() != 4 or not a_nchw.is_contiguous() or not b.is_contiguous() or b.dtype != a_nchw.dtype:
        return None
    N, C, H, W = a_nchw.shape
    if tuple(b.shape) != ((N, H * W, C) if tokens else (N, C, H, W)):
        raise HipError(f"bias_residual: b {tuple(b.shape)} does not match a {tuple(a_nchw.shape)}")
    r = BiasResidualArgs()
    r.a, r.b = a_nchw.data_ptr(), b.data_ptr()
    if bias is not None:
        r.bias = _vec(bias, a_nchw, C).data_ptr()
    if bias2 is not None:
        r.bias2 = _vec(bias2, a_nchw, C).data_ptr()
    out = torch.empty_like(a_nchw)
    r.out = out.data_ptr()
    r.n, r.channels, r.hw = N, C, H * W
    r.b_layout = LAYOUT_TOKENS if tokens else LAYOUT_NCHW
    r.dtype = _glue_dtype(a_nchw)
    ok = _glue_rc(lib().p2p_bias_residual(ctypes.byref(r), _stream(a_nchw.device)), "p2p_bias_residual")
    return out if ok else None


# -- the resnets' 3x3 convolutions (p2p_conv.hip)
# p2p_conv3x3_set_loop's values (include/p2p_hip.h)
CONV_LOOP_AUTO, CONV_LOOP_TILE, CONV_LOOP_PIPE128, CONV_LOOP_PIPE256 = 0, 1, 2, 3
# A/B switch, read once: P2P_CONV_PIPE=0 keeps every 3x3 convolution on the register-staged loop
CONV_PIPE = os.environ.get("P2P_CONV_PIPE", "1") != "0"


def conv3x3_set_loop(loop: int):
    """Process-wide: the tile loop p2p_conv3x3 / p2p_conv3x3_ex launch where the plan is bk = 64, bn = 160
    (CONV_LOOP_*; the bits are the same under each).  For tests and A/B runs; not under graph capture."""
    _check(lib().p2p_conv3x3_set_loop(int(loop)), "p2p_conv3x3_set_loop")


def conv3x3_split(n: int, h: int, w: int, c_in: int, c_out: int) -> int:
    """Workgroups along K per output tile that p2p_conv3x3 takes for these sizes (p2p_select.h): 1 =
    one launch, above 1 = the split form, 0 or negative = the sizes are not served."""
    return int(lib().p2p_conv3x3_split(n, h, w, c_in, c_out))


class ConvWeights:
    """The packed [9, C_out, C_in] images of nn.Conv2d 3x3 weights that p2p_conv3x3 stages (one
    p2p_conv3x3_pack launch each), per convolution module, with what each was built from: the
    weight's address, ``_version``, dtype and device.  ``get`` compares those on the host and repacks
    when one has changed (an optimiser step, load_state_dict, ``.to()``) -- but never under graph
    capture, where a miss returns None and the caller runs its own convolution: a captured graph must
    not bake in a repack of weights that can change between replays.  The entries die with their
    modules.  A packed image is a second copy of the weight."""

    def __init__(self):
        self._packed = weakref.WeakKeyDictionary()

    @staticmethod
    def key_of(w: torch.Tensor):
        return (w.data_ptr(), w._version, w.dtype, w.device)

    def get(self, conv) -> Optional[torch.Tensor]:
        w = conv.weight
        hit = self._packed.get(conv)
        if hit is not None and hit[0] == self.key_of(w):
            return hit[1]
        if torch.cuda.is_current_stream_capturing():
            return None
        packed = conv3x3_pack(w)
        if packed is not None:
            self._packed[conv] = (self.key_of(w), packed)
        return packed


CONV_WEIGHTS = ConvWeights()


def conv3x3_pack(weight: torch.Tensor) -> Optional[torch.Tensor]:
    """[9, C_out, C_in] from a dense [C_out, C_in, 3, 3] weight (p2p_conv3x3_pack), or None where the
    kernel does not serve it (f32, CPU, a channel count that is no multiple of 32)."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or not weight.is_cuda or not weight.is_contiguous():
        return None
    c_out, c_in = weight.shape[:2]
    with torch.no_grad():
        packed = torch.empty((9, c_out, c_in), dtype=weight.dtype, device=weight.device)
    a = Conv3x3PackArgs()
    a.weight, a.packed = weight.data_ptr(), packed.data_ptr()
    a.c_in, a.c_out = c_in, c_out
    a.dtype = _glue_dtype(weight)
    ok = _glue_rc(lib().p2p_conv3x3_pack(ctypes.byref(a), _stream(weight.device)), "p2p_conv3x3_pack")
    return packed if ok else None


def conv3x3(x_tokens: torch.Tensor, packed: torch.Tensor, h: int, w: int):
    """F.conv2d(x, weight, None, 1, 1) as [N, C_out, H, W] (p2p_conv3x3) from the token-major
    x_tokens [N, H*W, C_in] -- group_norm's ``tokens`` output -- and ``packed`` = conv3x3_pack(weight).
    None where the library does not serve the operands; the caller runs its own convolution."""
    _require_cuda(x_tokens, packed)
    if x_tokens.dim() != 3 or packed.dim() != 3 or not x_tokens.is_contiguous() or not packed.is_contiguous() or \
            packed.dtype != x_tokens.dtype:
        return None
    N, HW, c_in = x_tokens.shape
    c_out = packed.shape[1]
    if HW != h * w or packed.shape[0] != 9 or packed.shape[2] != c_in:
        raise HipError(f"conv3x3: x {tuple(x_tokens.shape)} / weight {tuple(packed.shape)} / {h} x {w} do not match")
    n_ws = int(lib().p2p_conv3x3_workspace_floats(N, h, w, c_in, c_out))
    if n_ws < 0 or conv3x3_split(N, h, w, c_in, c_out) < 1:
        return None
    a = Conv3x3Args()
    y = x_tokens.new_empty((N, c_out, h, w))
    a.x, a.weight, a.y = x_tokens.data_ptr(), packed.data_ptr(), y.data_ptr()
    if n_ws:
        ws = torch.empty(n_ws, dtype=torch.float32, device=x_tokens.device)
        a.workspace = ws.data_ptr()
    a.n, a.height, a.width, a.c_in, a.c_out = N, h, w, c_in, c_out
    a.dtype = _glue_dtype(x_tokens)
    return y if _glue_rc(lib().p2p_conv3x3(ctypes.byref(a), _stream(x_tokens.device)), "p2p_conv3x3") else None


# the sampling forms of p2p_conv3x3_ex (include/p2p_hip.h)
CONV_SAME, CONV_UP2, CONV_DOWN2 = 0, 1, 2


def conv3x3_out_map(form: int, h: int, w: int):
    """The output map of a form's input map h x w."""
    return {CONV_SAME: (h, w), CONV_UP2: (2 * h, 2 * w), CONV_DOWN2: (h // 2, w // 2)}[form]


def conv3x3_ex_split(form: int, n: int, h: int, w: int, c_in: int, c_out: int) -> int:
    """conv3x3_split for a sampling form, from the INPUT map h x w: 0 or negative = not served."""
    return int(lib().p2p_conv3x3_ex_split(form, n, h, w, c_in, c_out))


def conv3x3_ex(x_tokens: torch.Tensor, packed: torch.Tensor, bias, h: int, w: int, form: int = CONV_SAME):
    """The 3x3 convolution of the token-major x_tokens [N, h*w, C_in] in a sampling form
    (p2p_conv3x3_ex), with ``bias`` ([C_out] or None) added before the one rounding, as [N, C_out, H', W']:
    CONV_SAME F.conv2d(x, weight, bias, 1, 1); CONV_UP2 the same of F.interpolate(x, scale_factor=2,
    mode="nearest"), which is never written; CONV_DOWN2 F.conv2d(x, weight, bias, 2, 1) for even h, w.
    None where the library does not serve the operands; the caller runs its own lines."""
    _require_cuda(x_tokens, packed, bias)
    if x_tokens.dim() != 3 or packed.dim() != 3 or not x_tokens.is_contiguous() or not packed.is_contiguous() or \
            packed.dtype != x_tokens.dtype:
        return None
    N, HW, c_in = x_tokens.shape
    c_out = packed.shape[1]
    if HW != h * w or packed.shape[0] != 9 or packed.shape[2] != c_in or form not in (CONV_SAME, CONV_UP2, CONV_DOWN2):
        raise HipError(f"conv3x3_ex: x {tuple(x_tokens.shape)} / weight {tuple(packed.shape)} / {h} x {w} / form {form} "
                       f"do not match")
    n_ws = int(lib().p2p_conv3x3_ex_workspace_floats(form, N, h, w, c_in, c_out))
    if n_ws < 0 or conv3x3_ex_split(form, N, h, w, c_in, c_out) < 1:
        return None
    a = Conv3x3ExArgs()
    y = x_tokens.new_empty((N, c_out, *conv3x3_out_map(form, h, w)))
    a.x, a.weight, a.y = x_tokens.data_ptr(), packed.data_ptr(), y.data_ptr()
    if bias is not None:
        a.bias = _vec(bias, x_tokens, c_out).data_ptr()
    if n_ws:
        ws = torch.empty(n_ws, dtype=torch.float32, device=x_tokens.device)
        a.workspace = ws.data_ptr()
    a.n, a.in_height, a.in_width, a.c_in, a.c_out = N, h, w, c_in, c_out
    a.dtype, a.form = _glue_dtype(x_tokens), form
    return y if _glue_rc(lib().p2p_conv3x3_ex(ctypes.byref(a), _stream(x_tokens.device)), "p2p_conv3x3_ex") else None


def conv_input_tokens(x):
    """The token-major copy [N, H*W, C] of a dense NCHW activation that has no norm in front of its
    convolution (Upsample2D, Downsample2D): one p2p_nchw_to_tokens launch on the forward path, under
    the forward bindings' contract -- None where the kernel does not serve x (``nchw_to_tokens`` is
    the backward's binding of the same kernel, and raises)."""
    _require_cuda(x)
    if x.dim() != 4 or not x.is_contiguous():
        return None
    N, C, H, W = x.shape
    t = NchwToTokensArgs()
    dst = x.new_empty((N, H * W, C))
    t.src, t.dst = x.data_ptr(), dst.data_ptr()
    t.n, t.channels, t.hw = N, C, H * W
    t.dtype = _glue_dtype(x)
    return dst if _glue_rc(lib().p2p_nchw_to_tokens(ctypes.byref(t), _stream(x.device)), "p2p_nchw_to_tokens") else None


def conv3x3_up2(x_tokens, packed, bias, h: int, w: int):
    """conv3x3_ex in the CONV_UP2 form: Upsample2D's interpolate + convolution from the low-resolution map."""
    return conv3x3_ex(x_tokens, packed, bias, h, w, CONV_UP2)


def conv3x3_down2(x_tokens, packed, bias, h: int, w: int):
    """conv3x3_ex in the CONV_DOWN2 form: Downsample2D's stride-2 convolution."""
    return conv3x3_ex(x_tokens, packed, bias, h, w, CONV_DOWN2)


# -- the feed-forward GEMMs (p2p_linear.hip).  As the glue: None where the library does not serve the
# operands (CPU, f32, sizes or strides off the kernel's grid, a shape the selection declines)
LINEAR_BIAS, LINEAR_GEGLU, LINEAR_RESIDUAL = 0, 1, 2


def linear_split(form: int, m: int, k: int, n: int) -> int:
    """Workgroups along K per output tile that p2p_linear takes for x [m, k] and n output columns
    (p2p_select.h): 1 = one launch, above 1 = the split form, 0 or negative = not served."""
    return int(lib().p2p_linear_split(form, m, k, n))


def _rows(t: torch.Tensor) -> Optional[torch.Tensor]:
    """t [..., C] as a [rows, C] view with a unit last stride (dense and row-strided inputs), else None."""
    t2 = t.reshape(-1, t.shape[-1])
    return t2 if t2.stride(-1) == 1 and t2.data_ptr() == t.data_ptr() else None


def linear(x, weight, bias=None, form: int = LINEAR_BIAS, res=None, want_p: bool = False):
    """epilogue(x . weight^T) for x [..., K] and nn.Linear's weight (p2p_linear), f32 accumulation and one
    rounding.  LINEAR_BIAS: F.linear(x, weight, bias) [..., N].  LINEAR_GEGLU: weight [2 D, K];
    h * gelu(gate) [..., D] of F.linear's two halves, and with ``want_p`` the pair (out, p): p [..., 2 D]
    the rounded F.linear itself.  LINEAR_RESIDUAL: F.linear(x, weight, bias) + res, res [..., N].
    None where the library does not serve the operands; the caller runs its own lines."""
    ts = (x, weight) + (() if bias is None else (bias,)) + (() if res is None else (res,))
    if not all(t.is_cuda and t.dtype == x.dtype for t in ts) or x.dtype not in (torch.bfloat16, torch.float16):
        return None
    if form not in (LINEAR_BIAS, LINEAR_GEGLU, LINEAR_RESIDUAL) or (res is None) != (form != LINEAR_RESIDUAL) or \
            (want_p and form != LINEAR_GEGLU):
        raise HipError(f"linear: form {form} with res {res is not None}, want_p {want_p}")
    if weight.dim() != 2 or not weight.is_contiguous() or x.dim() < 1 or x.shape[-1] != weight.shape[1] or \
            (form == LINEAR_GEGLU and weight.shape[0] % 2):
        return None
    K = weight.shape[1]
    N = weight.shape[0] // 2 if form == LINEAR_GEGLU else weight.shape[0]
    x2 = _rows(x)
    r2 = None if res is None else _rows(res)
    if x2 is None or x2.shape[0] < 1 or (res is not None and (r2 is None or tuple(res.shape) != tuple(x.shape[:-1]) + (N,))):
        return None
    M = x2.shape[0]
    if linear_split(form, M, K, N) < 1:
        return None
    a = LinearArgs()
    a.x, a.weight = x2.data_ptr(), weight.data_ptr()
    a.x_row_stride = x2.stride(0) if M > 1 else K
    if bias is not None:
        a.bias = _vec(bias, x, weight.shape[0]).data_ptr()
    if r2 is not None:
        a.res, a.res_row_stride = r2.data_ptr(), (r2.stride(0) if M > 1 else N)
    y = x.new_empty(x.shape[:-1] + (N,))
    a.y = y.data_ptr()
    p = x.new_empty(x.shape[:-1] + (2 * N,)) if want_p else None
    if p is not None:
        a.p_out = p.data_ptr()
    n_ws = int(lib().p2p_linear_workspace_floats(form, M, K, N))
    if n_ws > 0:
        ws = torch.empty(n_ws, dtype=torch.float32, device=x.device)
        a.workspace = ws.data_ptr()
    a.m, a.k, a.n, a.form, a.dtype = M, K, N, form, _glue_dtype(x)
    if not _glue_rc(lib().p2p_linear(ctypes.byref(a), _stream(x.device)), "p2p_linear"):
        return None
    return (y, p) if want_p else y


def geglu(x):
    """x[..., :D] * gelu(x[..., D:]) for x [..., 2D] with a unit last stride (p2p_geglu)."""
    _require_cuda(x)
    D = x.shape[-1] // 2
    x2 = x.reshape(-1, x.shape[-1])     # a view for the dense and row-strided inputs served here
    if x.shape[-1] != 2 * D or x2.stride(-1) != 1 or x2.data_ptr() != x.data_ptr():
        return None
    g = GegluArgs()
    out = x.new_empty(x.shape[:-1] + (D,))
    g.inp, g.out = x2.data_ptr(), out.data_ptr()
    g.in_row_stride, g.out_row_stride = x2.stride(0) if x2.shape[0] > 1 else 2 * D, D
    g.rows, g.d = x2.shape[0], D
    g.dtype = _glue_dtype(x)
    return out if _glue_rc(lib().p2p_geglu(ctypes.byref(g), _stream(x.device)), "p2p_geglu") else None


def geglu_bwd(dout, x):
    """The gradient of geglu with respect to its input x [..., 2D] (p2p_geglu_bwd), dense in x's
    shape, from ``dout`` [..., D] (dense).  Unsupported raises."""
    _require_cuda(dout, x)
    D = x.shape[-1] // 2
    x2 = x.reshape(-1, x.shape[-1])
    if x.shape[-1] != 2 * D or x2.stride(-1) != 1 or x2.data_ptr() != x.data_ptr():
        raise HipError("geglu_bwd: the input must be the forward's (rows of 2 D elements, unit last stride)")
    if not dout.is_contiguous() or dout.dtype != x.dtype or tuple(dout.shape) != tuple(x.shape[:-1]) + (D,):
        raise HipError(f"geglu_bwd: dout {tuple(dout.shape)} {dout.dtype} does not match x {tuple(x.shape)} {x.dtype}")
    g = GegluBwdArgs()
    din = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    g.inp, g.dout, g.din = x2.data_ptr(), dout.data_ptr(), din.data_ptr()
    g.in_row_stride = x2.stride(0) if x2.shape[0] > 1 else 2 * D
    g.rows, g.d = x2.shape[0], D
    g.dtype = _glue_dtype(x)
    _check(lib().p2p_geglu_bwd(ctypes.byref(g), _stream(x.device)), "p2p_geglu_bwd")
    return din


def nchw_to_tokens(src):
    """[N, C, H, W] -> [N, H*W, C] (p2p_nchw_to_tokens): permute(0, 2, 3, 1) made dense, the
    gradient of bias_residual's token-major operand.  Unsupported raises."""
    _require_cuda(src)
    if src.dim() != 4 or not src.is_contiguous():
        raise HipError("nchw_to_tokens needs a dense [N, C, H, W] tensor")
    N, C, H, W = src.shape
    t = NchwToTokensArgs()
    dst = src.new_empty((N, H * W, C))
    t.src, t.dst = src.data_ptr(), dst.data_ptr()
    t.n, t.channels, t.hw = N, C, H * W
    t.dtype = _glue_dtype(src)
    _check(lib().p2p_nchw_to_tokens(ctypes.byref(t), _stream(src.device)), "p2p_nchw_to_tokens")
    return dst


# -- the U-Net's time path (p2p_unet.hip).  As the glue above: None where the kernels do not serve
# the operands (f32, CPU, a width that is no multiple of 8 or above TIME_MAX_D, more than MAX_BATCH rows).
TIME_MAX_D = 2048
TIME_PROJ_TILE = 16


def _time_operands(ts, d_in: int, n: int) -> bool:
    first = ts[0]
    return (all(t.is_cuda and t.dtype == first.dtype and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ts)
            and first.dtype in (torch.bfloat16, torch.float16) and d_in % 8 == 0 and d_in <= TIME_MAX_D
            and 1 <= n <= MAX_BATCH)


def time_embed(timesteps, w1, b1, w2, b2):
    """linear_2(silu(linear_1([cos(t f_i), sin(t f_i)]))) in the weights' dtype, [N, D], for N int64
    timesteps on the GPU (p2p_time_embed): timestep_embedding and TimestepEmbedding with f32 between
    the layers and one rounding at the end.  A stride-0 ``timesteps`` (one step expanded to N rows) is
    read as it is."""
    D, d_in = w1.shape
    N = timesteps.shape[0]
    if timesteps.dim() != 1 or timesteps.dtype != torch.int64 or not timesteps.is_cuda or \
            timesteps.stride(0) not in (0, 1) or not _time_operands((w1, b1, w2, b2), d_in, N) or \
            D % 8 or D > TIME_MAX_D:
        return None
    if tuple(w2.shape) != (D, D) or b1.numel() != D or b2.numel() != D:
        raise HipError(f"time_embed: linear_2 {tuple(w2.shape)} does not follow linear_1 {tuple(w1.shape)}")
    a = TimeEmbedArgs()
    a.timesteps, a.timestep_stride = timesteps.data_ptr(), timesteps.stride(0) if N > 1 else 1
    a.w1, a.b1, a.w2, a.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    ws = torch.empty((N, D), dtype=torch.float32, device=w1.device)
    emb = torch.empty((N, D), dtype=w1.dtype, device=w1.device)
    a.workspace, a.emb = ws.data_ptr(), emb.data_ptr()
    a.n, a.in_channels, a.d = N, d_in, D
    a.dtype = _glue_dtype(w1)
    return emb if _glue_rc(lib().p2p_time_embed(ctypes.byref(a), _stream(w1.device)), "p2p_time_embed") else None


class TimeProjTable:
    """The device-side segment table of p2p_time_proj for a list of (weight [C_r, D], bias [C_r])
    pairs, and what it was built from.  Building it copies 4 int64 per segment from pinned memory
    without waiting for the copy; the pinned allocation itself may synchronise the device, which is
    why a table is built in an eager call only (once per model and per move of its weights), never
    under graph capture.  ``valid_for`` compares addresses on the host only."""

    def __init__(self, pairs, gaps: Sequence[int] = ()):
        """``gaps``: elements (per row of emb) left unwritten in front of each segment's output (the
        tests poison them); the product packs the segments."""
        w0 = pairs[0][0]
        self.d, self.dtype, self.device = w0.shape[1], w0.dtype, w0.device
        flat = [t for pair in pairs for t in pair]
        self.supported = all(w.dim() == 2 and w.shape[1] == self.d and b.shape == (w.shape[0],) for w, b in pairs) \
            and _time_operands(flat, self.d, 1)
        self.key = self.key_of(pairs)
        self.widths = [w.shape[0] for w, _ in pairs]
        gaps = list(gaps) or [0] * len(pairs)
        self.starts, at = [], 0           # of out_r, in elements per row of emb
        for c, gap in zip(self.widths, gaps):
            self.starts.append(at + gap)
            at += gap + c
        self.row_elems = at
        self.tiles = sum((c + TIME_PROJ_TILE - 1) // TIME_PROJ_TILE for c in self.widths)
        self.table = self._rows = None
        if self.supported:
            rows = [[w, b, s, c] for w, b, s, c in zip(self.key[0::2], self.key[1::2], self.starts, self.widths)]
            self._rows = torch.tensor(rows, dtype=torch.int64).pin_memory()   # alive until the copy has run
            self.table = self._rows.to(self.device, non_blocking=True)        # [segments, 4]

    @staticmethod
    def key_of(pairs):
        return tuple(t.data_ptr() for pair in pairs for t in pair)

    def valid_for(self, pairs) -> bool:
        return self.key == self.key_of(pairs)


def time_proj(emb, table: TimeProjTable, out=None):
    """[W_r . silu(emb) + b_r for r] as dense [N, C_r] views of one arena (p2p_time_proj): every
    time_emb_proj(F.silu(emb)) of the U-Net in one launch.  ``out``: None, or a 1-D arena of at least
    N * table.row_elems elements."""
    N = emb.shape[0]
    if not table.supported or emb.dim() != 2 or emb.shape[1] != table.d or emb.dtype != table.dtype or \
            emb.device != table.device or not emb.is_contiguous() or not 1 <= N <= MAX_BATCH:
        return None
    if out is None:
        out = torch.empty(N * table.row_elems, dtype=emb.dtype, device=emb.device)
    elif out.dim() != 1 or out.numel() < N * table.row_elems or out.dtype != emb.dtype or not out.is_contiguous():
        raise HipError("time_proj: out must be a dense 1-D arena of N * row_elems elements")
    a = TimeProjArgs()
    a.emb, a.table, a.out = emb.data_ptr(), table.table.data_ptr(), out.data_ptr()
    a.n, a.d, a.segments, a.tiles = N, table.d, len(table.widths), table.tiles
    a.dtype = _glue_dtype(emb)
    if not _glue_rc(lib().p2p_time_proj(ctypes.byref(a), _stream(emb.device)), "p2p_time_proj"):
        return None
    return [out[s * N:(s + c) * N].view(N, c) for s, c in zip(table.starts, table.widths)]


# -- the image ends (p2p_image.hip).  As the glue above: None where the library reports the shape
# or alignment unsupported (height * width % 4 != 0), and the caller runs its torch lines.
def image_u8(x: torch.Tensor):
    """uint8 [N, H, W, 3] from a decoder output x [N, 3, H, W] (f32 / bf16 / f16), byte for byte
    (((x.float() / 2 + 0.5).clamp(0, 1)) * 255).to(torch.uint8) in NHWC (p2p_image_u8)."""
    _require_cuda(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise HipError(f"image_u8 needs [N, 3, H, W], got {tuple(x.shape)}")
    if not x.is_contiguous():
        return None
    N, _, H, W = x.shape
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=x.device)
    a = ImageU8Args()
    a.x, a.out = x.data_ptr(), out.data_ptr()
    a.n, a.height, a.width, a.dtype = N, H, W, _dtype_code(x)
    return out if _glue_rc(lib().p2p_image_u8(ctypes.byref(a), _stream(x.device)), "p2p_image_u8") else None


def image_to_model(img: torch.Tensor, dtype: torch.dtype):
    """[N, 3, H, W] in ``dtype`` from uint8 pixels [H, W, 3] or [N, H, W, 3]: img / 127.5 - 1 in f32,
    rounded once (p2p_image_to_model)."""
    _require_cuda(img)
    if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise HipError(f"image_to_model needs uint8 [H, W, 3] or [N, H, W, 3], got {img.dtype} {tuple(img.shape)}")
    if img.dim() == 3:
        img = img[None]
    if not img.is_contiguous():
        return None
    N, H, W, _ = img.shape
    out = torch.empty((N, 3, H, W), dtype=dtype, device=img.device)
    a = ImageToModelArgs()
    a.img, a.out = img.data_ptr(), out.data_ptr()
    a.n, a.height, a.width, a.dtype = N, H, W, _dtype_code(out)
    ok = _glue_rc(lib().p2p_image_to_model(ctypes.byref(a), _stream(img.device)), "p2p_image_to_model")
    return out if ok else None


# -- the attention-map figures (p2p_viz.hip).  None where the kernels do not serve the tensors (not
# on the GPU, not f32 and dense, P * K % 4 != 0, more than MAX_AGG_LAYERS layers, a panel size
# outside the supported range): the callers in controllers.py then run their torch / PIL lines.
def maps_aggregate(stores: Sequence[torch.Tensor], n_prompts: int, select: int, steps: int):
    """The ``select`` prompt's average over ``stores`` (running sums [n_prompts * heads_l, P, K]) and
    their heads of sum / steps, [P, K] f32 (p2p_maps_aggregate): main.py:293-307 for one prompt
    without a scaled copy of any store."""
    stores = list(stores)
    if not stores or not all(s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.dim() == 3
                             for s in stores):
        return None
    if len(stores) > MAX_AGG_LAYERS:
        return None
    P, K = stores[0].shape[1], stores[0].shape[2]
    if any(s.shape[1:] != (P, K) or s.shape[0] % n_prompts or s.device != stores[0].device for s in stores):
        raise HipError(f"maps_aggregate: stores must be [{n_prompts} * heads, {P}, {K}] on one device")
    a = MapsAggregateArgs()
    for i, s in enumerate(stores):
        a.stores[i], a.heads[i] = s.data_ptr(), s.shape[0] // n_prompts
    a.n_layers, a.n_prompts, a.select = len(stores), int(n_prompts), int(select)
    a.P, a.K, a.steps = P, K, int(steps)
    out = torch.empty((P, K), dtype=torch.float32, device=stores[0].device)
    a.out = out.data_ptr()
    ok = _glue_rc(lib().p2p_maps_aggregate(ctypes.byref(a), _stream(out.device)), "p2p_maps_aggregate")
    return out if ok else None


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_coeffs(n_in: int, n_out: int):
    """The tables of PIL's 8-bit bicubic resize of n_in pixels to n_out (Resample.c precompute_coeffs
    and normalize_coeffs_8bpc, in its operation order, in double precision): (coeffs int32
    [n_out, ksize], bounds int32 [n_out, 2]).  Output pixel i is
    clamp((2^21 + sum_t in[bounds[i, 0] + t] * coeffs[i, t]) >> 22, 0, 255), t < bounds[i, 1];
    ksize is 5 whenever n_in <= n_out."""
    import math
    import numpy as np
    scale = float(n_in) / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    coeffs = np.zeros((n_out, ksize), dtype=np.int32)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coeffs[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = xmin, xmax
    return coeffs, bounds


_resize_tables = {}


def _device_resize_tables(res: int, S: int, device):
    """resize_coeffs(res, S) on ``device``, uploaded once per (res, S, device)."""
    key = (res, S, str(device))
    hit = _resize_tables.get(key)
    if hit is None:
        coeffs, bounds = resize_coeffs(res, S)
        assert coeffs.shape == (S, RESIZE_TAPS) and int((bounds[:, 0] + bounds[:, 1]).max()) <= res
        hit = _resize_tables[key] = (torch.from_numpy(coeffs).to(device), torch.from_numpy(bounds).to(device))
    return hit


def map_panels_supported(res: int, S: int) -> bool:
    return 1 <= res <= PANEL_MAX_RES and res <= S <= PANEL_MAX_SIDE and S % 4 == 0


def map_panels(src: torch.Tensor, n: int, res: int, S: int, mode: int, panel_stride: int, pixel_stride: int,
               out: Optional[torch.Tensor] = None, out_row_stride: Optional[int] = None,
               out_panel_stride: Optional[int] = None):
    """``n`` maps of res x res values of the f32 tensor ``src`` -- element (panel i, pixel p) at flat
    index i * panel_stride + p * pixel_stride -- as grey RGB uint8 panels of S x S pixels
    (p2p_map_panels): mode PANEL_MAX is (255 * x / x.max()).astype(uint8), PANEL_MINMAX subtracts the
    minimum first; the upscale is Image.resize((S, S)), byte for byte.  ``out``: None (a new uint8
    [n, S, S, 3]) or a dense uint8 canvas on src's device that panel i is written into from byte
    i * out_panel_stride on, its rows out_row_stride bytes apart; every other byte of it is left
    alone.  Returns ``out``."""
    if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous()) or not map_panels_supported(res, S):
        return None
    if n < 1 or panel_stride < 0 or pixel_stride < 1 or \
            (n - 1) * panel_stride + (res * res - 1) * pixel_stride >= src.numel():
        raise HipError(f"map_panels: {n} panels of {res}^2 pixels (strides {panel_stride}, {pixel_stride}) "
                       f"do not lie in {src.numel()} elements")
    if mode not in (PANEL_MAX, PANEL_MINMAX):
        raise HipError(f"map_panels: unknown mode {mode}")
    if out is None:
        out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=src.device)
        out_row_stride, out_panel_stride = 3 * S, 3 * S * S
    else:
        _require_cuda(out)
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != src.device:
            raise HipError("map_panels: out must be a dense uint8 tensor on the maps' device")
        if out_row_stride < 3 * S or out_panel_stride < 0 or \
                (n - 1) * out_panel_stride + (S - 1) * out_row_stride + 3 * S > out.numel():
            raise HipError(f"map_panels: {n} panels (strides {out_row_stride}, {out_panel_stride} bytes) do not "
                           f"lie in a canvas of {out.numel()} bytes")
    coeffs, bounds = _device_resize_tables(res, S, src.device)
    a = MapPanelsArgs()
    a.inp, a.panel_stride, a.pixel_stride = src.data_ptr(), int(panel_stride), int(pixel_stride)
    a.coeffs, a.bounds, a.out = coeffs.data_ptr(), bounds.data_ptr(), out.data_ptr()
    a.out_row_stride, a.out_panel_stride = int(out_row_stride), int(out_panel_stride)
    a.res, a.n, a.S, a.mode = int(res), int(n), int(S), int(mode)
    return out if _glue_rc(lib().p2p_map_panels(ctypes.byref(a), _stream(src.device)), "p2p_map_panels") else None


# -- the text encoders (p2p_text.hip).  As the glue above: None where the library reports the dtype,
# shape or alignment unsupported -- or the tensors are not on the GPU -- and the caller runs its
# torch lines; any other rejection raises.
LN_MAX_CHANNELS = 2048


def _text_attn(q, k, v, heads, scale, key_counts, what):
    if not (q.is_cuda and k.is_cuda and v.is_cuda) or q.dtype not in (torch.bfloat16, torch.float16):
        return None
    o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    for n0 in range(0, q.shape[0], MAX_BATCH):     # the library takes MAX_BATCH entries per launch
        sl = slice(n0, n0 + MAX_BATCH)
        t = make_tensors(q[sl], k[sl], v[sl], o[sl], heads, scale, "bf16")
        if what == "p2p_causal_attn_fwd":
            rc = lib().p2p_causal_attn_fwd(ctypes.byref(t), _stream(q.device))
        else:
            counts = key_counts[sl].data_ptr() if key_counts is not None else None
            rc = lib().p2p_text_attn_fwd(ctypes.byref(t), counts, _stream(q.device))
        if rc in (P2P_E_HEAD_DIM, P2P_E_KEYS, P2P_E_DTYPE, P2P_E_ALIGN):
            return None                            # decided from the shapes: the first chunk's answer is every chunk's
        _check(rc, what)
    return o


def causal_attn(q, k, v, heads: int, scale: float):
    """softmax(causal(q k^T * scale)) v for q / k / v [N, T, heads * 64] with a unit last stride
    (strided views of one QKV GEMM output are served as they are), T <= MAX_KEYS_CROSS
    (p2p_causal_attn_fwd).  Returns a dense [N, T, heads * 64] tensor."""
    return _text_attn(q, k, v, heads, scale, None, "p2p_causal_attn_fwd")


def text_attn(q, k, v, heads: int, scale: float, key_counts=None):
    """softmax(q k^T * scale) v, every token attending to every token, for the operands of
    causal_attn (p2p_text_attn_fwd).  ``key_counts``: None, or a contiguous int32 [N] tensor on the
    operands' device: entry n attends to its first key_counts[n] tokens only (the kernel clamps a
    count into [1, T]); all T rows are computed.  Returns a dense [N, T, heads * 64] tensor."""
    if key_counts is not None:
        _require_cuda(key_counts)
        if (key_counts.dtype != torch.int32 or key_counts.shape != (q.shape[0],) or not key_counts.is_contiguous()
                or key_counts.device != q.device):
            raise HipError(f"text_attn: key_counts must be a contiguous int32 [{q.shape[0]}] tensor on {q.device}")
    return _text_attn(q, k, v, heads, scale, key_counts, "p2p_text_attn_fwd")


def layer_norm(x, gamma, beta, eps: float, add=None, add_bias=None, sum_out=None):
    """LayerNorm(x + add + add_bias) * gamma + beta over the last dimension (p2p_layer_norm).  x, add:
    dense [..., C]; add_bias, gamma, beta: [C]; sum_out: None, or a dense tensor like x (x itself is
    allowed) that receives the rounded sum.  Returns y, shaped like x."""
    C = x.shape[-1]
    ts = [t for t in (x, add, add_bias, gamma, beta, sum_out) if t is not None]
    if not all(t.is_cuda and t.dtype == x.dtype and t.is_contiguous() for t in ts) or C > LN_MAX_CHANNELS:
        return None
    if (add is not None and add.shape != x.shape) or (sum_out is not None and sum_out.shape != x.shape):
        raise HipError(f"layer_norm: add / sum_out do not match x {tuple(x.shape)}")
    a = LayerNormArgs()
    a.x = x.data_ptr()
    a.add = add.data_ptr() if add is not None else None
    a.add_bias = _vec(add_bias, x, C).data_ptr() if add_bias is not None else None
    a.gamma, a.beta = _vec(gamma, x, C).data_ptr(), _vec(beta, x, C).data_ptr()
    a.sum_out = sum_out.data_ptr() if sum_out is not None else None
    y = torch.empty_like(x)
    a.y = y.data_ptr()
    a.rows, a.channels = x.numel() // C, C
    a.eps = float(eps)
    a.dtype = _glue_dtype(x)
    return y if _glue_rc(lib().p2p_layer_norm(ctypes.byref(a), _stream(x.device)), "p2p_layer_norm") else None


def bias_quick_gelu(x, bias, out=None):
    """h * sigmoid(1.702 h), h = x + bias, for x [..., D] with a unit last stride (p2p_bias_quick_gelu);
    ``out``: None (a new dense tensor) or x itself (in place)."""
    return _bias_act(x, bias, out, "p2p_bias_quick_gelu")


def bias_gelu(x, bias, out=None):
    """0.5 h (1 + erf(h / sqrt 2)), h = x + bias: the exact GELU, for the operands of bias_quick_gelu
    (p2p_bias_gelu)."""
    return _bias_act(x, bias, out, "p2p_bias_gelu")


def _bias_act(x, bias, out, what):
    D = x.shape[-1]
    if not (x.is_cuda and bias.is_cuda) or bias.dtype != x.dtype:
        return None
    x2 = x.reshape(-1, D)     # a view for the dense and row-strided inputs served here
    if x2.stride(-1) != 1 or x2.data_ptr() != x.data_ptr():
        return None
    if out is not None and out is not x:
        raise HipError(f"{what}: out is None or the input itself")
    res = x if out is x else x.new_empty(x.shape)
    g = BiasActArgs()
    g.inp, g.bias, g.out = x2.data_ptr(), _vec(bias, x, D).data_ptr(), res.data_ptr()
    g.in_row_stride = x2.stride(0) if x2.shape[0] > 1 else D
    g.out_row_stride = g.in_row_stride if out is x else D
    g.rows, g.d = x2.shape[0], D
    g.dtype = _glue_dtype(x)
    return res if _glue_rc(getattr(lib(), what)(ctypes.byref(g), _stream(x.device)), what) else None
