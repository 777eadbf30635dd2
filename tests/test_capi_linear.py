"""p2p_linear rejects bad arguments before launching anything, the new entry points are declared and
exported together, the ABI version stands, and p2p_linear.hip is part of the hashed source list."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from p2p_amd import _hip, _srchash

E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32
BIAS, GEGLU, RES = _hip.LINEAR_BIAS, _hip.LINEAR_GEGLU, _hip.LINEAR_RESIDUAL
NEW = ("p2p_linear", "p2p_linear_split", "p2p_linear_workspace_floats")


def _lin(**kw):
    a = _hip.LinearArgs()
    a.x, a.weight, a.bias, a.y, a.workspace = 4096, 1 << 20, 1 << 19, 1 << 21, 1 << 22
    a.m, a.k, a.n, a.form, a.dtype = 128, 64, 64, BIAS, BF16
    a.x_row_stride = a.res_row_stride = 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), E_ARG), (dict(weight=None), E_ARG), (dict(y=None), E_ARG),
    (dict(form=RES, res=None), E_ARG), (dict(form=3), E_ARG), (dict(form=-1), E_ARG),
    (dict(m=0), E_ARG), (dict(k=0), E_ARG), (dict(n=-8), E_ARG),
    (dict(m=1 << 20, k=4096, x_row_stride=4096), E_ARG),              # the elements of x
    (dict(m=1 << 20, n=4096), E_ARG),                                 # the elements of y
    (dict(form=GEGLU, m=1 << 20, n=1024), E_ARG),                     # y fits, p_out does not
    (dict(k=65536, n=32768, x_row_stride=65536), E_ARG),              # the elements of the weight
    (dict(m=1 << 20, x_row_stride=4096), E_ARG),                      # x fits dense, its strided rows do not
    (dict(form=RES, res=1 << 23, m=1 << 20, res_row_stride=4096), E_ARG),
    (dict(x_row_stride=-64), E_ARG),
    (dict(k=2560, n=160, x_row_stride=2560, workspace=None), E_ARG),  # these sizes split K: a workspace is needed
    (dict(dtype=F32), E_DTYPE), (dict(dtype=9), E_DTYPE),
    (dict(k=48, x_row_stride=48), E_ALIGN), (dict(n=20), E_ALIGN), (dict(form=GEGLU, n=36), E_ALIGN),
    (dict(x_row_stride=68), E_ALIGN), (dict(x_row_stride=56), E_ALIGN),        # % 8, and shorter than a row
    (dict(form=RES, res=1 << 23, res_row_stride=60), E_ALIGN), (dict(form=RES, res=1 << 23, res_row_stride=56), E_ALIGN),
    (dict(x=4104), E_ALIGN), (dict(weight=(1 << 20) + 2), E_ALIGN), (dict(y=(1 << 21) + 8), E_ALIGN),
    (dict(bias=(1 << 19) + 1), E_ALIGN), (dict(form=RES, res=(1 << 23) + 4), E_ALIGN),
    (dict(form=GEGLU, p_out=(1 << 24) + 8), E_ALIGN),
    (dict(k=2560, n=160, x_row_stride=2560, workspace=(1 << 22) + 4), E_ALIGN),
])
def test_linear_rejects(kw, code):
    assert _hip.lib().p2p_linear(ctypes.byref(_lin(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_linear(ctypes.byref(_lin(dtype=F16, **kw)), None) == code


def test_null_args_and_size_queries():
    L = _hip.lib()
    assert L.p2p_linear(None, None) == E_ARG
    assert L.p2p_linear_split(BIAS, 0, 64, 64) == E_ARG and L.p2p_linear_workspace_floats(BIAS, 0, 64, 64) == E_ARG
    assert L.p2p_linear_split(5, 128, 64, 64) == E_ARG and L.p2p_linear_workspace_floats(5, 128, 64, 64) == E_ARG
    assert L.p2p_linear_split(BIAS, 128, 48, 64) == E_ALIGN and L.p2p_linear_workspace_floats(RES, 128, 64, 60) == E_ALIGN
    assert L.p2p_linear_split(BIAS, 128, 64, 64) == 1 and L.p2p_linear_workspace_floats(BIAS, 128, 64, 64) == 0
    split = L.p2p_linear_split(RES, 136, 2560, 160)
    assert split > 1 and L.p2p_linear_workspace_floats(RES, 136, 2560, 160) == split * 160 * 256   # rows in whole tiles


def test_new_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "p2p_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS
        assert hasattr(_hip.lib(), name)
    assert re.search(r"^#define P2P_ABI_VERSION 16$", header, re.M)
    assert _hip.lib().p2p_abi_version() == 16


def test_source_is_hashed():
    assert "p2p_linear.hip" in _srchash.SOURCES and "p2p_mma_tile.h" in _srchash.HEADERS


def test_cpu_and_f32_operands_are_declined():
    import torch
    x, w = torch.zeros(128, 64, dtype=torch.bfloat16), torch.zeros(64, 64, dtype=torch.bfloat16)
    assert _hip.linear(x, w) is None
    assert _hip.linear(x, w, None, RES, res=torch.zeros(128, 64, dtype=torch.bfloat16)) is None
    assert _hip.linear(x.float(), w.float()) is None
