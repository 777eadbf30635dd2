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
