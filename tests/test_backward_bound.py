"""The bounds tests/test_gpu_backward.py holds the attention backward to, checked on the CPU:

(a) every case of backward_ref.CASES takes the query split it is named for (p2p_attn_bwd_workspace
    is host-only), so the GPU shapes reach the paths they are there for;
(b) a float32 restatement of the kernels' roundings (backward_ref.emulate) stays inside the bf16
    bounds against the float64 reference: the bounds admit a correct kernel;
(c) the same restatement with one seeded fault -- lse off by 2^-5, the last key of the dQ pass
    dropped, the last query of the dK/dV pass dropped -- breaks a bound on every case with K > 1,
    and the lse fault is one that the older criterion (3e-2 of the maximum, cosine 0.999) lets
    through on every case;
(d) p2p_attn_bwd rejects bad arguments before any launch (dummy pointers, no GPU).
"""
import ctypes

import pytest
import torch

from p2p_amd import _hip

import backward_ref as br
from test_capi import _tensors

CASES = list(range(len(br.CASES)))
MANY_KEYS = [i for i in CASES if br.CASES[i][2] > 1]
ids = lambda i: br.CASE_IDS[i]  # noqa: E731


def _case_tensors(index):
    N, P, K, H, d, _ = br.CASES[index]
    C = H * d
    return _tensors(n_batch=N, n_query=P, n_key=K, n_heads=H, head_dim=d, io_dtype=1, scale=d ** -0.5,
                    q_row_stride=C, k_row_stride=C, v_row_stride=C, o_row_stride=C, q_batch_stride=P * C,
                    o_batch_stride=P * C, k_batch_stride=K * C, v_batch_stride=K * C)


# ---------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("index", CASES, ids=ids)
def test_case_takes_its_split(index):
    t = _case_tensors(index)
    assert _hip.lib().p2p_attn_bwd_workspace(ctypes.byref(t)) == br.workspace_bytes(index)


def test_case_table_is_the_issue_s():
    assert len(br.CASES) == len(br.SPLITS) == 11
    assert br.CASES[10] == (1, 64, 3328, 8, 160, 2) and br.workspace_bytes(10) == 68157440
    # case 11 runs the reduction's grid-stride loop: more float4s than 4096 blocks x 256 threads
    N, _, K, H, d, _ = br.CASES[10]
    assert N * K * H * d // 4 > 4096 * 256
    assert br.CASES[9][0] == 64      # P2P_MAX_BATCH


# ---------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("index", CASES, ids=ids)
def test_clean_emulation_is_inside_the_bounds(index):
    inp, ref = br.cpu_case(index, torch.bfloat16)
    figures = br.measure(br.emulate(*inp), ref)
    print(br.CASE_IDS[index], {k: round(v / br.U, 2) if k != "lse" else v for k, v in figures.items()})
    assert not br.violations(figures, torch.bfloat16)


def test_reference_gradients_are_autograd_s():
    """reference() against torch autograd of the same float64 attention."""
    (q, k, v, dout, H, scale), ref = br.cpu_case(0, torch.bfloat16)
    qd, kd, vd = (x.double().requires_grad_() for x in (q, k, v))
    s = br._heads(qd, H) @ br._heads(kd, H).transpose(-1, -2) * scale
    o = br._tokens(s.softmax(-1) @ br._heads(vd, H))
    o.backward(dout.double())
    for name, want in (("O", o.detach()), ("dQ", qd.grad), ("dK", kd.grad), ("dV", vd.grad)):
        assert (ref[name] - want).abs().max().item() <= 1e-12 * want.abs().max().item(), name
    lse = torch.logsumexp(s.detach(), -1) * br.LOG2E
    assert (ref["lse"] - lse.reshape(ref["lse"].shape)).abs().max().item() <= 1e-12
    # the bounds dominate what they bound
    for name in br.QUANTITIES:
        assert (ref[name].abs() <= ref["B_" + name] * (1 + 1e-12) + 1e-300).all(), name


# ---------------------------------------------------------------------------- (c)
GRADS = ("elem:dQ", "frob:dQ", "elem:dK", "frob:dK", "elem:dV", "frob:dV")


@pytest.mark.parametrize("index", MANY_KEYS, ids=ids)
@pytest.mark.parametrize("mutant", ["lse", "lastkey", "lastquery"])
def test_mutant_breaks_a_bound(index, mutant):
    inp, ref = br.cpu_case(index, torch.bfloat16)
    got = br.emulate(*inp, mutant=mutant)
    bad = br.violations(br.measure(got, ref), torch.bfloat16)
    old = br.old_criterion_passes(got, ref)
    print(br.CASE_IDS[index], mutant, "older criterion passes:", old, "broken:", sorted(bad))
    # a gradient bound, not only the lse's own
    assert any(key in GRADS for key in bad), bad
    if mutant == "lse":
        assert "lse" in bad
        # a uniform 2.2 % scale error: inside 3e-2 of the maximum, cosine loss ~1e-5
        assert old, "the older criterion was expected to let the lse fault through"
        # and it is the Frobenius bound that sees it
        assert {"frob:dQ", "frob:dK", "frob:dV"} <= set(bad)


def test_lse_bound_against_the_mutant_size():
    """2^-5 against a 2^-7 bound: the lse fault is four bounds away, not marginal."""
    assert br.LSE_ABS * 4 == 2.0 ** -5


# ---------------------------------------------------------------------------- f32 constants
def test_f32_bounds_follow_the_rule():
    """2x the emulation's maximum over the cases, never above the project's 3e-2."""
    elem = frob = 0.0
    for index in CASES:
        inp, ref = br.cpu_case(index, torch.float32)
        figures = br.measure(br.emulate(*inp), ref)
        assert figures["lse"] <= br.LSE_ABS
        for key, val in figures.items():
            if key.startswith("elem:"):
                elem = max(elem, val)
            elif key.startswith("frob:"):
                frob = max(frob, val)
    print("f32 emulation maxima (u): elem %.2f frob %.2f" % (elem / br.U, frob / br.U))
    assert br.ELEM_F32 == pytest.approx(min(2 * elem, 3e-2), rel=0.05)
    assert br.FROB_F32 == pytest.approx(min(2 * frob, 3e-2), rel=0.05)
    assert br.ELEM_F32 <= 3e-2 and br.FROB_F32 <= 3e-2


# ---------------------------------------------------------------------------- (d)
def _bwd(t, dout=64, lse=128, delta=192, dq=256, dk=320, dv=384, kv_f32=0, ws=None, ws_bytes=0):
    return _hip.lib().p2p_attn_bwd(ctypes.byref(t), dout, lse, delta, dq, dk, dv, kv_f32, ws, ws_bytes, None)


@pytest.mark.parametrize("name", ["dout", "lse", "delta", "dq", "dk", "dv"])
def test_bwd_rejects_a_null_pointer(name):
    assert _bwd(_tensors(io_dtype=1), **{name: None}) == -1


def test_bwd_rejects_a_missing_or_short_workspace():
    t = _case_tensors(1)
    need = br.workspace_bytes(1)
    assert need > 0
    assert _bwd(t, ws=None, ws_bytes=need) == -1
    assert _bwd(t, ws=512, ws_bytes=need - 1) == -1
    assert _bwd(t, ws=512 + 8, ws_bytes=need) == -6


@pytest.mark.parametrize("name", ["dout", "dq", "dk", "dv"])
def test_bwd_rejects_a_pointer_off_16_bytes(name):
    assert _bwd(_tensors(io_dtype=1), **{name: 72}) == -6
    t = _case_tensors(1)
    assert _bwd(t, ws=512, ws_bytes=br.workspace_bytes(1), **{name: 72}) == -6


def test_bwd_rejects_the_f32_check_mode():
    assert _bwd(_tensors(io_dtype=0, compute=1)) == -3


@pytest.mark.parametrize("d", [16, 48])
def test_bwd_rejects_a_head_dim_without_backward(d):
    # 16 has a compiled forward and no backward; 48 has neither
    for io in (0, 1):
        assert _bwd(_tensors(io_dtype=io, head_dim=d)) == -2
