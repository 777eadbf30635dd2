"""p2p_conv3x3 and p2p_conv3x3_pack reject bad arguments before launching anything, the new entry
points are declared and exported together, and p2p_conv.hip is part of the hashed source list."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from p2p_amd import _hip, _srchash

E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32
NEW = ("p2p_conv3x3", "p2p_conv3x3_split", "p2p_conv3x3_workspace_floats", "p2p_conv3x3_pack")


def _conv(**kw):
    a = _hip.Conv3x3Args()
    a.x, a.weight, a.y, a.workspace = 4096, 1 << 20, 1 << 21, 1 << 22
    a.n, a.height, a.width, a.c_in, a.c_out, a.dtype = 2, 8, 8, 64, 64, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), E_ARG), (dict(weight=None), E_ARG), (dict(y=None), E_ARG),
    (dict(n=0), E_ARG), (dict(height=0), E_ARG), (dict(width=-1), E_ARG), (dict(c_in=0), E_ARG), (dict(c_out=0), E_ARG),
    (dict(n=65536, height=256, width=256), E_ARG),             # n h w = 2^32
    (dict(n=32768, height=64, width=64, c_in=64), E_ARG),      # n h w fits, the elements of x do not
    (dict(c_in=1280, c_out=1280, workspace=None), E_ARG),      # these sizes split K: a workspace is needed
    (dict(dtype=F32), E_DTYPE), (dict(dtype=9), E_DTYPE),
    (dict(c_in=48), E_ALIGN), (dict(c_out=80), E_ALIGN),       # channel counts in 32s
    (dict(height=3, width=3), E_ALIGN),                        # h w % 8
    (dict(x=4104), E_ALIGN), (dict(weight=(1 << 20) + 2), E_ALIGN), (dict(y=(1 << 21) + 8), E_ALIGN),
    (dict(c_in=1280, c_out=1280, workspace=(1 << 22) + 4), E_ALIGN),
    (dict(height=128, width=64), E_ALIGN),                     # a map the selection does not serve
])
def test_conv3x3_rejects(kw, code):
    assert _hip.lib().p2p_conv3x3(ctypes.byref(_conv(**kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_conv3x3(ctypes.byref(_conv(dtype=F16, **kw)), None) == code


def _pack(**kw):
    a = _hip.Conv3x3PackArgs()
    a.weight, a.packed, a.c_in, a.c_out, a.dtype = 4096, 1 << 20, 64, 64, BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(weight=None), E_ARG), (dict(packed=None), E_ARG), (dict(c_in=0), E_ARG), (dict(c_out=-32), E_ARG),
    (dict(c_in=32768, c_out=32768), E_ARG),
    (dict(dtype=F32), E_DTYPE),
    (dict(c_in=40), E_ALIGN), (dict(c_out=72), E_ALIGN), (dict(packed=(1 << 20) + 8), E_ALIGN), (dict(weight=4097), E_ALIGN),
])
def test_conv3x3_pack_rejects(kw, code):
    assert _hip.lib().p2p_conv3x3_pack(ctypes.byref(_pack(**kw)), None) == code


def test_null_args_and_size_queries():
    L = _hip.lib()
    assert L.p2p_conv3x3(None, None) == E_ARG and L.p2p_conv3x3_pack(None, None) == E_ARG
    assert L.p2p_conv3x3_split(0, 8, 8, 64, 64) == E_ARG and L.p2p_conv3x3_workspace_floats(0, 8, 8, 64, 64) == E_ARG
    assert L.p2p_conv3x3_split(2, 8, 8, 48, 64) == E_ALIGN and L.p2p_conv3x3_workspace_floats(2, 8, 8, 64, 80) == E_ALIGN
    assert L.p2p_conv3x3_split(2, 128, 64, 64, 64) == 0 and L.p2p_conv3x3_workspace_floats(2, 128, 64, 64, 64) == 0
    assert L.p2p_conv3x3_workspace_floats(2, 8, 8, 64, 64) == 0        # no split: no workspace
    split = L.p2p_conv3x3_split(2, 8, 8, 1280, 1280)
    assert split > 1 and L.p2p_conv3x3_workspace_floats(2, 8, 8, 1280, 1280) == split * 2 * 64 * 1280


def test_new_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "p2p_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS
        assert hasattr(_hip.lib(), name)


def test_source_is_hashed():
    assert "p2p_conv.hip" in _srchash.SOURCES
