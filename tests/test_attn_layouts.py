"""tests/attn_layouts.py itself, and what tests/test_gpu_layouts.py rests on, checked without a GPU:

- the views have the strides each layout promises and keep the 16-byte rule for bf16, f16 and f32;
- every (case, layout) pair of the GPU file passes the library's argument validation and selects the
  kernel the case names (the p2p_*_attn_kernel queries launch nothing and follow no pointer);
- the padding check reports a planted one-element write at the end of a row, between batch entries
  and before the view; the unwritten-element check reports a planted hole;
- the data tells the strides apart: for every (shape, layout) pair of the GPU file the f32 reference
  computed with V read at K's row stride, and with K's batch stride used for Q, is further from the
  correct one than the bound the GPU test applies -- wherever the layout makes the two strides
  differ (dense and the fused projections share some by construction; skewed shares none);
- the kernel names the GPU cases declare are the production rows of csrc/p2p_select.h.
"""
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

from p2p_amd import _hip

import attn_layouts as al
import test_gpu_layouts as gl
from test_gpu_kernels import ref_out, ref_probs

CSRC = os.path.join(ROOT, "prompt-to-prompt_amd", "csrc")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
GEOM = dict(N=3, P=10, K=7, H=2, d=8)      # C = 16


def _build(layout, dtype=torch.bfloat16, P=None, **kw):
    g = dict(GEOM, **({"P": P} if P else {}))
    return al.build(g["N"], g["P"], g["K"], g["H"], g["d"], dtype, 1, layout, **kw), g


# ---------------------------------------------------------------------------- the views
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_layout_strides(dtype):
    C = 16
    ops, g = _build("dense", dtype)
    assert all(t.is_contiguous() for t in (ops.q, ops.k, ops.v, ops.o))
    ops, g = _build("fused_self", dtype, P=7)
    for i, t in enumerate((ops.q, ops.k, ops.v)):
        assert t.stride() == (7 * 3 * C, 3 * C, 1) and t.storage_offset() == i * C
        assert t.data_ptr() == ops.bufs["qkv"].data_ptr() + i * C * t.element_size()
    assert ops.o.is_contiguous()
    ops, g = _build("fused_cross", dtype)
    assert ops.q.is_contiguous() and ops.o.is_contiguous()
    for i, t in enumerate((ops.k, ops.v)):
        assert t.stride() == (7 * 2 * C, 2 * C, 1) and t.storage_offset() == i * C
    ops, g = _build("skewed", dtype)
    ts = dict(q=ops.q, k=ops.k, v=ops.v, o=ops.o)
    assert [ts[n].stride(1) for n in "qkvo"] == [C + 8, C + 16, C + 24, C + 32]
    strides = [ts[n].stride(i) for n in "qkvo" for i in (0, 1)]
    assert len(set(strides)) == 8
    for n in "qkvo":
        rows = ts[n].shape[1]
        extra = ts[n].stride(0) - rows * ts[n].stride(1)
        assert extra > 0 and extra % 8 == 0 and ts[n].storage_offset() > 0 and ts[n].storage_offset() % 8 == 0
    assert len({ts[n].stride(0) - ts[n].shape[1] * ts[n].stride(1) for n in "qkvo"}) == 4
    ops, g = _build("broadcast_kv", dtype)
    assert ops.k.stride() == (0, C, 1) and ops.v.stride() == (0, C, 1)
    assert torch.equal(ops.k[0], ops.k[2]) and torch.equal(ops.k, ops.dense["k"]) and torch.equal(ops.v, ops.dense["v"])


@pytest.mark.parametrize("layout", al.LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_views_hold_the_values_and_keep_the_16_byte_rule(layout, dtype):
    ops, g = _build(layout, dtype, P=7 if layout == "fused_self" else None)
    want = al.values(g["N"], g["P"], g["K"], g["H"], g["d"], dtype, 1)
    if layout == "broadcast_kv":
        want = (want[0], want[1][:1].expand_as(want[1]), want[2][:1].expand_as(want[2]))
    for got, w, name in zip((ops.q, ops.k, ops.v), want, "qkv"):
        assert al.same_bits(got, w) and al.same_bits(ops.dense[name], w.contiguous())
    es = ops.q.element_size()
    for t in (ops.q, ops.k, ops.v, ops.o):
        assert t.data_ptr() % 16 == 0 and t.stride(-1) == 1
        assert (t.stride(0) * es) % 16 == 0 and (t.stride(1) * es) % 16 == 0
    # everything that belongs to no input view is the filler, the whole o buffer the sentinel
    inside = {}
    for n in "qkv":
        v = ops.views[n]
        inside[id(v.buf)] = inside.get(id(v.buf), torch.zeros(v.buf.numel(), dtype=torch.bool)) | al._inside(v)
    for n in "qkv":
        v = ops.views[n]
        assert torch.isnan(v.buf[~inside[id(v.buf)]].float()).all() and not torch.isnan(v.buf[inside[id(v.buf)]].float()).any()
    assert (al._bits(ops.views["o"].buf) == al.SENTINEL[es]).all()
    assert torch.isfinite(ops.views["o"].buf.float()).all()
    # a fresh o buffer: nothing outside spoilt, nothing inside written
    assert not al.padding_report(ops.views["o"])
    assert len(al.unwritten_report(ops.views["o"], limit=10 ** 6)) == g["N"] * g["P"] * g["H"] * g["d"]


# ---------------------------------------------------------------------------- the two reports
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_padding_check_reports_a_planted_write(dtype):
    ops, g = _build("skewed", dtype)
    view, C = ops.views["o"], 16
    ops.o.fill_(1.0)
    al.check_output(ops)                                     # a clean launch passes
    spots = {"the padding after the row": view.offset + view.bs + 4 * view.ld + C,      # entry 1, row 4, first pad element
             "between batch entries": view.offset + view.bs - 1,                       # last slack element after entry 0
             "before the view": view.offset - 1,
             "the tail": view.offset + 2 * view.bs + 10 * view.ld}                      # first element after the last row
    for where, i in spots.items():
        keep = view.buf[i].clone()
        view.buf[i] = 1.0
        report = al.padding_report(view)
        assert len(report) == 1 and where in report[0] and f"element {i} " in report[0], (where, report)
        with pytest.raises(AssertionError, match="written outside the view"):
            al.check_output(ops)
        view.buf[i] = keep
        assert not al.padding_report(view)


@pytest.mark.parametrize("layout", ["dense", "skewed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_unwritten_check_reports_a_planted_hole(layout, dtype):
    ops, g = _build(layout, dtype)
    view = ops.views["o"]
    fresh = ops.o[1, 3, 5].clone()                           # the sentinel
    ops.o.fill_(float("nan"))                                # NaN is "written": NaN-ness is another check
    assert not al.unwritten_report(view)
    ops.o[1, 3, 5] = fresh
    report = al.unwritten_report(view)
    assert len(report) == 1 and "entry 1 row 3 column 5" in report[0], report
    with pytest.raises(AssertionError, match="never written"):
        al.check_output(ops)


def test_guarded_buffer():
    buf, used = al.guarded(100, 16, "cpu", fill=7.0)
    assert used.numel() == 100 and (used == 7.0).all() and al.guards_intact(buf, 100, 16)
    used.zero_()
    assert al.guards_intact(buf, 100, 16)
    buf[15] = 0.0
    assert not al.guards_intact(buf, 100, 16)
    buf[15] = al.GUARD
    buf[116] = 0.0
    assert not al.guards_intact(buf, 100, 16)


# ---------------------------------------------------------------------------- the GPU file's cases
def _pairs():
    for c in gl.ALL_CASES:
        for layout in ["dense"] + c.layouts() + (["broadcast_kv"] if c.kind == "cross" else []):
            yield pytest.param(c, layout, id=f"{c.id}-{layout}")


@pytest.mark.parametrize("c,layout", list(_pairs()))
def test_case_passes_validation_and_selects_its_kernel(monkeypatch, c, layout):
    """The library's own answer for the views of every (case, layout) pair, from host tensors: the
    queries validate as the forward calls do (the operand layout contract included), select, launch
    nothing and follow no pointer."""
    monkeypatch.setattr(_hip, "_require_cuda", lambda *ts: None)
    ops = c.build(layout)
    t = _hip.make_tensors(ops.q, ops.k, ops.v, ops.o, c.H, c.scale, c.compute)
    for name in "qkvo":
        view = ops.views[name]
        assert getattr(t, name + "_row_stride") == view.ld and getattr(t, name + "_batch_stride") == view.bs
        assert getattr(t, name) == view.buf.data_ptr() + view.offset * view.buf.element_size()
    if c.kind == "self":
        assert _hip.self_attn_kernel(t) == c.kernel
    elif c.kind == "maps":
        assert _hip.self_attn_kernel(t, keeps_maps=True) == c.kernel
    elif c.kind == "cross":
        assert gl.cross_kernel_name(c, ops, gl.cross_groups(c, "cpu")[0]) == c.kernel
    else:   # the materialise protocol has no query; its fused-mode answer shows the views pass validation
        assert _hip.self_attn_kernel(t) is not None


def test_pv_cases_name_the_rows_select_self_takes(tmp_path):
    """The P V mode has no name query in the C ABI: ask csrc/p2p_select.h itself (host-only C++)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    io = {torch.float32: "P2P_DTYPE_F32", torch.bfloat16: "P2P_DTYPE_BF16", torch.float16: "P2P_DTYPE_F16"}
    compute = {"bf16": "P2P_COMPUTE_BF16", "f32": "P2P_COMPUTE_F32"}
    calls = "".join(f'  std::puts(p2p::name((p2p::SelfKernel)p2p::select_self({io[c.dtype]}, {compute[c.compute]}, {c.d}, '
                    f'{c.P}, {c.K}, p2p::MODE_PV_, false, false, 0)));\n' for c in gl.PV_CASES)
    src, exe = tmp_path / "pv.cpp", tmp_path / "pv"
    src.write_text('#include <cstdio>\n#include "p2p_select.h"\nint main() {\n' + calls + "  return 0;\n}\n")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[:len(gl.PV_CASES)] == [c.kernel for c in gl.PV_CASES]


def test_expected_kernels_are_the_production_rows_of_the_table():
    text = open(os.path.join(CSRC, "p2p_select.h")).read()
    rows = re.findall(r'^\s*X\((\w+),[^"\n]*"([^"]+)"\)', text, flags=re.M)
    assert len(rows) >= 36
    production = [name for ident, name in rows if not ident.endswith("_STAMPS") and ident != "SELF_WIDE"]
    assert sorted(production) == sorted(gl.EXPECTED_KERNELS)
    gl.test_cases_cover_the_selection_table()


# ---------------------------------------------------------------------------- the data shows a mix-up
def _shapes():
    seen = {}
    for c in gl.ALL_CASES:
        key = (c.N, c.P, c.K, c.H, c.d, c.dtype, c.compute, c.seed, c.qscale, c.cross)
        seen.setdefault(key, c)
    return [pytest.param(c, id=c.id) for c in seen.values()]


@pytest.mark.parametrize("c", _shapes())
def test_stride_mixups_show_in_the_data(c):
    """Negative control for the data, per shape and layout: O from the same buffers with V read at
    K's row stride, and with K's batch stride used for Q (finite filler in place of NaN), against
    the bound of the GPU test.  Where a layout makes the two strides equal the mix-up is the
    identity; skewed makes none equal."""
    seen = {"ld": 0, "bs": 0}
    for layout in ["dense"] + c.layouts() + (["broadcast_kv"] if c.kind == "cross" else []):
        ops = c.build(layout, filler=0.5)
        vq, vk, vv = (ops.views[n] for n in "qkv")

        def out(q, v):
            return ref_out(ref_probs(q, ops.k, c.H, c.scale), v, c.H)

        want = out(ops.q, ops.v)
        bound = gl.o_bound(ops.v, want, c.compute, c.dtype)
        assert layout != "skewed" or (vv.ld != vk.ld and vq.bs != vk.bs)
        if vv.ld != vk.ld:
            err = (out(ops.q, vv.tensor(ld=vk.ld)) - want).abs().max().item()
            assert err > bound, (layout, "V at K's row stride", err, bound)
            seen["ld"] += 1
        if vq.bs != vk.bs:
            err = (out(vq.tensor(bs=vk.bs), ops.v) - want).abs().max().item()
            assert err > bound, (layout, "Q at K's batch stride", err, bound)
            seen["bs"] += 1
    assert seen["ld"] >= 1 and seen["bs"] >= 1
