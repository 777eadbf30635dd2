"""float16 tensors at the C ABI (ABI 16): P2P_DTYPE_F16 is declared, accepted by the forward entry
points as a 2-byte type on the 16-bit MFMA pipe only, and rejected by the autograd pair -- all
decided before anything is launched (no GPU needed for these calls)."""
import ctypes
import os
import re

import torch

from conftest import ROOT

from p2p_amd import _hip

from test_capi import _tensors

HEADER = os.path.join(ROOT, "include", "p2p_hip.h")


def test_header_declares_f16_and_abi():
    text = open(HEADER).read()
    assert re.search(r"\bP2P_DTYPE_F16\s*=\s*2\b", text)
    abi = int(re.search(r"#define\s+P2P_ABI_VERSION\s+(\d+)", text).group(1))
    assert abi == _hip.ABI_VERSION == 16
    assert _hip.lib().p2p_abi_version() == 16
    assert _hip.P2P_DTYPE_F16 == 2


def test_dtype_code():
    assert _hip._dtype_code(torch.empty(1, dtype=torch.float16)) == 2
    assert _hip._dtype_code(torch.empty(1, dtype=torch.bfloat16)) == 1
    assert _hip._dtype_code(torch.empty(1, dtype=torch.float32)) == 0


def test_self_attn_takes_f16_as_a_two_byte_type():
    L = _hip.lib()

    def rc(**kw):
        t = _tensors(**kw)
        return L.p2p_self_attn_fwd(ctypes.byref(t), None, None, None, 0, None, None)

    # accepted as a dtype, then 324 elements x 2 bytes breaks the 16-byte row alignment (an f32
    # row of 324 elements would be aligned: the element size in use is 2)
    assert rc(io_dtype=2, q_row_stride=324) == -6
    assert rc(io_dtype=2, compute=1) == -3      # the exact-f32 check mode takes f32 tensors only
    assert rc(io_dtype=3) == -3


def test_autograd_pair_rejects_f16():
    L = _hip.lib()
    t = _tensors(io_dtype=2, n_query=1024, n_key=1024, head_dim=80)
    assert L.p2p_attn_fwd_lse(ctypes.byref(t), 64, None) == -3
    assert L.p2p_attn_bwd(ctypes.byref(t), 64, 64, 64, 64, 64, 64, 0, None, 0, None) == -3
    assert L.p2p_attn_bwd_workspace(ctypes.byref(t)) == -3


def test_latent_step_dtype_range():
    L = _hip.lib()
    a = _hip.LatentArgs()
    a.eps, a.x, a.out = 64, 128, 256
    a.n_prompts, a.channels, a.height, a.width = 2, 4, 64, 64
    a.eps_dtype = 7
    bad = L.p2p_latent_step(ctypes.byref(a), None)
    assert bad == -3
    a.eps_dtype = 3
    assert L.p2p_latent_step(ctypes.byref(a), None) == bad


def test_layout_rules_count_f16_as_two_bytes():
    """The operand layout contract (include/p2p_hip.h) with float16 tensors: the span limit counts
    2-byte elements, and production's fused-projection strides pass."""
    from test_capi import LAYOUT_CALLS, _layout_tensors, _layout_violations

    def accepted(**kw):
        return _hip.self_attn_kernel(_tensors(io_dtype=2, **kw)) is not None

    # P = K = 4096, C = 320: (4095 ld + 320) x 2 <= INT32_MAX  <=>  ld <= 262207 (twice the f32 limit)
    for op in "qkvo":
        assert accepted(**{f"{op}_row_stride": 262200, f"{op}_batch_stride": 262200 * 4096})
        assert not accepted(**{f"{op}_row_stride": 262208, f"{op}_batch_stride": 262208 * 4096})
    assert accepted(q_row_stride=960, k_row_stride=960, v_row_stride=960, q_batch_stride=960 * 4096,
                    k_batch_stride=960 * 4096, v_batch_stride=960 * 4096)
    assert _hip.self_attn_kernel(_tensors(io_dtype=2, q_row_stride=960, k_row_stride=960, v_row_stride=960,
                                          q_batch_stride=960 * 4096, k_batch_stride=960 * 4096,
                                          v_batch_stride=960 * 4096)) == "self40_kernel<40,8,2,256,H16>"
    # every rule, every operand, through the forward entry points that take float16
    L = _hip.lib()
    for fn in ("p2p_self_attn_fwd", "p2p_cross_attn_fwd", "p2p_attn_probs", "p2p_attn_pv"):
        needs, call = LAYOUT_CALLS[fn]
        for op in needs:
            for rule, kw in _layout_violations(op).items():
                assert call(L, _layout_tensors(io_dtype=2, **kw)) == -1, (fn, op, rule)
    # the autograd forward still answers the dtype first
    assert LAYOUT_CALLS["p2p_attn_fwd_lse"][1](L, _layout_tensors(io_dtype=2, q_row_stride=312)) == -3
