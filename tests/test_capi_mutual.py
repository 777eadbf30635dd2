"""p2p_mutual_attn_fwd / p2p_mutual_attn_kernel / p2p_token_classes at the C ABI: declared, exported,
bound, additive to ABI 16, and every rejection made before anything is launched or dereferenced (the
pointers below are never valid; no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from p2p_amd import _hip, _srchash

from test_capi import _tensors, declared_functions

HEADER = os.path.join(ROOT, "include", "p2p_hip.h")
NEW = ("p2p_mutual_attn_fwd", "p2p_mutual_attn_kernel", "p2p_token_classes")


def mutual(t, kv_src=None, token_class=None):
    src = (ctypes.c_int32 * len(kv_src))(*kv_src) if kv_src is not None else None
    return _hip.lib().p2p_mutual_attn_fwd(ctypes.byref(t), src, token_class, None)


def self_fwd(t):
    return _hip.lib().p2p_self_attn_fwd(ctypes.byref(t), None, None, None, 0, None, None)


def test_symbols_declared_exported_and_bound():
    L = _hip.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert L.p2p_mutual_attn_kernel.restype is ctypes.c_char_p
    assert callable(_hip.mutual_attn) and callable(_hip.token_classes) and callable(_hip.mutual_attn_kernel)


def test_abi_is_still_16():
    abi = int(re.search(r"#define\s+P2P_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert abi == _hip.ABI_VERSION == _hip.lib().p2p_abi_version() == 16


def test_source_is_registered():
    assert "p2p_mutual.hip" in _srchash.SOURCES
    assert os.path.exists(os.path.join(ROOT, "prompt-to-prompt_amd", "csrc", "p2p_mutual.hip"))


@pytest.mark.parametrize("kw,kv_src,code", [
    (dict(q=None), None, -1), (dict(k=None), None, -1), (dict(v=None), None, -1), (dict(o=None), None, -1),
    (dict(n_key=77), None, -1),                                     # n_query != n_key
    (dict(n_key=4095), None, -1),
    (dict(), [0, 0, 2, 2, 4, 4, 6, 8], -5),                         # kv_src[n] >= n_batch
    (dict(), [0, 0, 2, 2, 4, 4, 6, 1 << 20], -5),
    (dict(n_batch=65), None, -5),                                   # above P2P_MAX_BATCH
    (dict(head_dim=44), None, -2),
    (dict(io_dtype=7), None, -3),
    (dict(io_dtype=1, compute=1), None, -3),
    (dict(io_dtype=2, compute=1), None, -3),
])
def test_rejections(kw, kv_src, code):
    assert mutual(_tensors(**kw), kv_src) == code
    assert mutual(_tensors(**kw), kv_src, token_class=64) == code
    assert _hip.lib().p2p_mutual_attn_fwd(None, None, None, None) == -1


def test_null_tensors_and_negative_sources():
    assert _hip.mutual_attn_kernel(_tensors(n_key=77)) is None
    # every entry skipped: accepted, and nothing is launched (the pointers are not valid)
    assert mutual(_tensors(), [-1] * 8) == 0
    assert mutual(_tensors(), [-1] * 8, token_class=64) == 0
    assert mutual(_tensors(io_dtype=1), [-7] * 8) == 0


ALIGN = [dict(q_row_stride=321), dict(k_row_stride=322), dict(v_batch_stride=320 * 4096 + 2), dict(q=8), dict(k=24),
         dict(v=4), dict(o=40), dict(io_dtype=2, q_row_stride=324), dict(io_dtype=1, o_row_stride=324)]


@pytest.mark.parametrize("kw", ALIGN)
def test_alignment_contract_is_self_attn_fwds(kw):
    t = _tensors(**kw)
    assert mutual(t) == self_fwd(t) == -6


ROWS, CH = 77, 320


def violations(op):
    """tests/test_capi.py's _layout_violations for a square ROWS x ROWS call."""
    wide = 1 << 24                          # 76 rows x 2^24 elements x 2 bytes is already past INT32_MAX
    bad = {
        "rows_overlap": {f"{op}_row_stride": CH - 8},
        "negative_row_stride": {f"{op}_row_stride": -CH},
        "negative_batch_stride": {f"{op}_batch_stride": -CH * ROWS},
        "span_past_int32": {f"{op}_row_stride": wide, f"{op}_batch_stride": wide * ROWS},
    }
    if op == "o":
        bad["batch_entries_overlap"] = {"o_batch_stride": (ROWS - 1) * CH + CH - 8}
        bad["zero_batch_stride_on_o"] = {"o_batch_stride": 0}
    return bad


LAYOUT = [pytest.param(kw, id=f"{op}-{rule}") for op in "qkvo" for rule, kw in violations(op).items()]


@pytest.mark.parametrize("kw", LAYOUT)
@pytest.mark.parametrize("io_dtype", [0, 1, 2])
def test_stride_contract_is_self_attn_fwds(kw, io_dtype):
    """The operand layout contract: the code p2p_self_attn_fwd returns for the same tensors."""
    base = {f"{x}_batch_stride": CH * ROWS for x in "qkvo"}
    base.update(kw)
    t = _tensors(io_dtype=io_dtype, n_query=ROWS, n_key=ROWS, **base)
    assert mutual(t, [0] * 8) == self_fwd(t) == -1


def test_layout_contract_accepts_what_self_attn_fwd_accepts():
    def accepted(**kw):
        t = _tensors(**kw)
        return _hip.mutual_attn_kernel(t, True) is not None, _hip.self_attn_kernel(t) is not None

    assert accepted() == (True, True)
    assert accepted(q_batch_stride=0, k_batch_stride=0, v_batch_stride=0) == (True, True)     # broadcast entries
    assert accepted(o_batch_stride=0) == (False, False)
    # fused-projection views: row stride 3C, bases C apart
    fused = dict(q_row_stride=960, k_row_stride=960, v_row_stride=960, q_batch_stride=960 * 4096,
                 k_batch_stride=960 * 4096, v_batch_stride=960 * 4096, io_dtype=1)
    assert accepted(**fused) == (True, True)
    assert accepted(o_row_stride=131104, o_batch_stride=131104 * 4096) == (False, False)      # span past int32


def test_token_classes_rejections():
    L = _hip.lib()

    def args(**kw):
        a = _hip.TokenClassesArgs()
        a.sums[0] = 64
        a.n_groups, a.group_size, a.lh, a.res, a.threshold, a.cfg, a.n_res = 1, 2, 10, 16, 0.1, 1, 1
        a.side[0], a.out[0] = 32, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rc(a):
        return L.p2p_token_classes(ctypes.byref(a), None)

    assert L.p2p_token_classes(None, None) == -1
    for kw in (dict(n_groups=0), dict(n_groups=33), dict(group_size=0), dict(lh=0), dict(res=0), dict(res=33),
               dict(n_res=0), dict(n_res=4), dict(threshold=float("nan"))):
        assert rc(args(**kw)) == -1, kw
    assert rc(args(group_size=33)) == -5                       # 66 rows with cfg
    a = args()
    a.sums[0] = None
    assert rc(a) == -1
    a = args()
    a.sums[0] = 66
    assert rc(a) == -6
    a = args()
    a.out[0] = None
    assert rc(a) == -1
    a = args()
    a.side[0] = 0
    assert rc(a) == -1
