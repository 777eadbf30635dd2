"""p2p_conv3x3_set_loop: declared in the header, exported, bound and hashed with its loop's header;
every known value is taken and an unknown one is refused with P2P_E_ARG, which changes nothing."""
import os
import re

import pytest

from conftest import ROOT

from p2p_amd import _hip, _srchash

E_ARG = -1


def test_declared_exported_and_hashed():
    with open(os.path.join(ROOT, "include", "p2p_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint p2p_conv3x3_set_loop\(int32_t loop\);", header)
    assert "#define P2P_ABI_VERSION 16" in header       # additive
    assert "p2p_conv3x3_set_loop" in _hip.EXPORTED_SYMBOLS
    assert hasattr(_hip.lib(), "p2p_conv3x3_set_loop") and callable(_hip.conv3x3_set_loop)
    assert "p2p_mma_pipe.h" in _srchash.HEADERS and "p2p_mma_tile.h" in _srchash.HEADERS
    assert "p2p_conv.hip" in _srchash.SOURCES
    assert (_hip.CONV_LOOP_AUTO, _hip.CONV_LOOP_TILE, _hip.CONV_LOOP_PIPE128, _hip.CONV_LOOP_PIPE256) == (0, 1, 2, 3)


def test_known_values_are_taken():
    L = _hip.lib()
    try:
        for value in (1, 2, 3, 0):
            assert L.p2p_conv3x3_set_loop(value) == 0
    finally:
        L.p2p_conv3x3_set_loop(0)


@pytest.mark.parametrize("value", [-1, 4, 99, 1 << 20])
def test_unknown_value_is_refused(value):
    L = _hip.lib()
    assert L.p2p_conv3x3_set_loop(value) == E_ARG
    with pytest.raises(_hip.HipError):
        _hip.conv3x3_set_loop(value)
    assert L.p2p_conv3x3_set_loop(0) == 0
