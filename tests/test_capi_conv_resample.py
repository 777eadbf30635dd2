"""p2p_conv3x3_ex rejects bad arguments before launching anything, with p2p_conv3x3's codes, in every
sampling form; the new entry points are declared and exported together, and the old entry's structs
keep their layout."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from p2p_amd import _hip

E_ARG, E_DTYPE, E_ALIGN = -1, -3, -6
BF16, F16, F32 = _hip.P2P_DTYPE_BF16, _hip.P2P_DTYPE_F16, _hip.P2P_DTYPE_F32
SAME, UP2, DOWN2 = _hip.CONV_SAME, _hip.CONV_UP2, _hip.CONV_DOWN2
NEW = ("p2p_conv3x3_ex", "p2p_conv3x3_ex_split", "p2p_conv3x3_ex_workspace_floats")


def _conv(**kw):
    a = _hip.Conv3x3ExArgs()
    a.x, a.weight, a.bias, a.y, a.workspace = 4096, 1 << 20, 1 << 19, 1 << 21, 1 << 22
    a.n, a.in_height, a.in_width, a.c_in, a.c_out, a.dtype, a.form = 2, 8, 8, 64, 64, BF16, SAME
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("form", [SAME, UP2, DOWN2], ids=["same", "up2", "down2"])
@pytest.mark.parametrize("kw,code", [
    (dict(x=None), E_ARG), (dict(weight=None), E_ARG), (dict(y=None), E_ARG),
    (dict(n=0), E_ARG), (dict(in_height=0), E_ARG), (dict(in_width=-1), E_ARG), (dict(c_in=0), E_ARG), (dict(c_out=0), E_ARG),
    (dict(n=65536, in_height=256, in_width=256), E_ARG),           # n h w = 2^32
    (dict(n=32768, in_height=64, in_width=64, c_in=64), E_ARG),    # the elements of x (or of y) do not fit
    (dict(c_in=1280, c_out=1280, workspace=None), E_ARG),          # these sizes split K: a workspace is needed
    (dict(dtype=F32), E_DTYPE), (dict(dtype=9), E_DTYPE),
    (dict(c_in=48), E_ALIGN), (dict(c_out=80), E_ALIGN),           # channel counts in 32s
    (dict(in_height=3, in_width=3), E_ALIGN),                      # h_out w_out % 8 (9, 36); odd sizes for Down2
    (dict(x=4104), E_ALIGN), (dict(weight=(1 << 20) + 2), E_ALIGN), (dict(y=(1 << 21) + 8), E_ALIGN),
    (dict(bias=(1 << 19) + 1), E_ALIGN),
    (dict(c_in=1280, c_out=1280, workspace=(1 << 22) + 4), E_ALIGN),
    (dict(in_height=512, in_width=256), E_ALIGN),                  # an output map the selection does not serve
])
def test_conv3x3_ex_rejects(form, kw, code):
    assert _hip.lib().p2p_conv3x3_ex(ctypes.byref(_conv(form=form, **kw)), None) == code
    if "dtype" not in kw:
        assert _hip.lib().p2p_conv3x3_ex(ctypes.byref(_conv(form=form, dtype=F16, **kw)), None) == code


@pytest.mark.parametrize("form", [3, -1, 99])
def test_unknown_form(form):
    L = _hip.lib()
    assert L.p2p_conv3x3_ex(ctypes.byref(_conv(form=form)), None) == E_ARG
    assert L.p2p_conv3x3_ex_split(form, 2, 8, 8, 64, 64) == E_ARG
    assert L.p2p_conv3x3_ex_workspace_floats(form, 2, 8, 8, 64, 64) == E_ARG


def test_down2_needs_even_input_sizes():
    L = _hip.lib()
    assert L.p2p_conv3x3_ex(ctypes.byref(_conv(form=DOWN2, in_height=15, in_width=16)), None) == E_ALIGN
    assert L.p2p_conv3x3_ex_split(DOWN2, 2, 16, 15, 64, 64) == E_ALIGN


def test_null_args_and_size_queries():
    L = _hip.lib()
    assert L.p2p_conv3x3_ex(None, None) == E_ARG
    for form in (SAME, UP2, DOWN2):
        assert L.p2p_conv3x3_ex_split(form, 0, 8, 8, 64, 64) == E_ARG
        assert L.p2p_conv3x3_ex_workspace_floats(form, 0, 8, 8, 64, 64) == E_ARG
        assert L.p2p_conv3x3_ex_split(form, 2, 8, 8, 48, 64) == E_ALIGN
        assert L.p2p_conv3x3_ex_workspace_floats(form, 2, 8, 8, 64, 80) == E_ALIGN
        assert L.p2p_conv3x3_ex_split(form, 2, 512, 256, 64, 64) == 0
        assert L.p2p_conv3x3_ex_workspace_floats(form, 2, 512, 256, 64, 64) == 0
    assert L.p2p_conv3x3_ex_workspace_floats(UP2, 2, 4, 4, 64, 64) == 0        # no split: no workspace
    for form, h, out_hw in ((SAME, 8, 64), (UP2, 4, 64), (DOWN2, 16, 64)):
        split = L.p2p_conv3x3_ex_split(form, 2, h, h, 1280, 1280)
        assert split == L.p2p_conv3x3_split(2, 8, 8, 1280, 1280) > 1
        assert L.p2p_conv3x3_ex_workspace_floats(form, 2, h, h, 1280, 1280) == split * 2 * out_hw * 1280


def test_new_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "p2p_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _hip.EXPORTED_SYMBOLS
        assert hasattr(_hip.lib(), name)
    for form, value in (("P2P_CONV_SAME", SAME), ("P2P_CONV_UP2", UP2), ("P2P_CONV_DOWN2", DOWN2)):
        assert re.search(r"\b%s = %d\b" % (form, value), header), form
    assert "#define P2P_ABI_VERSION 16" in header       # additive


def test_struct_layouts():
    """The old entry's struct is untouched; the new one's fields are where the header puts them."""
    assert ctypes.sizeof(_hip.Conv3x3Args) == 4 * 8 + 6 * 4
    assert [f[0] for f in _hip.Conv3x3Args._fields_] == ["x", "weight", "y", "workspace", "n", "height", "width", "c_in",
                                                        "c_out", "dtype"]
    assert [f[0] for f in _hip.Conv3x3ExArgs._fields_] == ["x", "weight", "bias", "y", "workspace", "n", "in_height",
                                                          "in_width", "c_in", "c_out", "dtype", "form"]
    assert ctypes.sizeof(_hip.Conv3x3ExArgs) == 5 * 8 + 7 * 4 + 4   # (padded to the pointers' alignment)
