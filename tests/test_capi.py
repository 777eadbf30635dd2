"""The C-ABI library: builds, loads, exports every symbol include/p2p_hip.h declares, and
rejects bad arguments before launching anything (no GPU needed for these calls)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from p2p_amd import _hip

HEADER = os.path.join(ROOT, "include", "p2p_hip.h")


def declared_functions():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(p2p_\w+)\s*\(", text, flags=re.M)))


def test_library_exists_and_loads():
    assert os.path.exists(_hip.library_path()), "run __graft_entry__.build()"
    L = _hip.lib()
    assert L.p2p_abi_version() == _hip.ABI_VERSION


def test_every_declared_symbol_is_exported():
    L = _hip.lib()
    names = declared_functions()
    assert len(names) >= 8
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(_hip.EXPORTED_SYMBOLS)


def test_error_strings():
    L = _hip.lib()
    for code in (0, -1, -2, -3, -4, -5, -6):
        assert L.p2p_error_string(code)


def _tensors(**kw):
    t = _hip.AttnTensors()
    t.q = t.k = t.v = t.o = 16
    t.q_row_stride = t.k_row_stride = t.v_row_stride = t.o_row_stride = 320
    t.q_batch_stride = t.k_batch_stride = t.v_batch_stride = t.o_batch_stride = 320 * 4096
    t.n_batch, t.n_query, t.n_key, t.n_heads, t.head_dim = 8, 4096, 4096, 8, 40
    t.io_dtype, t.compute, t.scale = 0, 0, 40 ** -0.5
    for k, v in kw.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize("kw,code", [
    (dict(q=None), -1),
    (dict(n_batch=65), -5),
    (dict(head_dim=44), -2),
    (dict(io_dtype=7), -3),
    (dict(io_dtype=1, compute=1), -3),
    (dict(q_row_stride=321), -6),
    (dict(q=8), -6),
])
def test_self_attn_rejects(kw, code):
    L = _hip.lib()
    t = _tensors(**kw)
    assert L.p2p_self_attn_fwd(ctypes.byref(t), None, None, None, 0, None, None) == code


def test_self_attn_rejects_bad_source_index():
    L = _hip.lib()
    t = _tensors()
    src = (ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 99)
    assert L.p2p_self_attn_fwd(ctypes.byref(t), src, None, None, 0, None, None) == -5


def test_self_attn_store_needs_lse_workspace():
    # a kept map needs the row log-sum-exp scratch (rejected before any launch)
    L = _hip.lib()
    t = _tensors(n_query=1024, n_key=1024, head_dim=80)
    slots = (ctypes.c_int32 * 8)(-1, -1, -1, -1, 0, 8, 16, 24)
    assert L.p2p_self_attn_fwd(ctypes.byref(t), None, 64, slots, 1, None, None) == -1
    assert L.p2p_self_attn_fwd(ctypes.byref(t), None, 64, slots, 1, 72, None) == -6


def test_cross_attn_rejects():
    L = _hip.lib()
    t = _tensors(n_key=77)
    G = (_hip.Group * 2)()
    G[0].first, G[0].count = 0, 4
    G[1].first, G[1].count = 4, 3          # does not cover the batch
    assert L.p2p_cross_attn_fwd(ctypes.byref(t), G, 2, None, None, 0, None) == -5
    t2 = _tensors(n_key=200)
    assert L.p2p_cross_attn_fwd(ctypes.byref(t2), G, 2, None, None, 0, None) == -4
    G[1].count = 4
    G[1].program = 64                      # an edit program needs its alpha row
    assert L.p2p_cross_attn_fwd(ctypes.byref(t), G, 2, None, None, 0, None) == -1


def test_localblend_rejects():
    L = _hip.lib()
    a = _hip.BlendArgs()
    assert L.p2p_localblend(ctypes.byref(a), None) == -1
    assert L.p2p_store_scale(None, None, 1.0, 10, None) == -1


def _blend_args(**kw):
    """p2p_localblend arguments inside every limit (dummy pointers: nothing may be launched)."""
    a = _hip.BlendArgs()
    for l in range(5):
        a.maps[l] = 1 << 20
    a.n_maps, a.heads_per_map, a.n_prompts, a.n_words, a.map_res = 5, 8, 4, 77, 16
    a.alpha_layers, a.th_pool, a.th_sub = 1 << 21, 0.3, 0.3
    a.x_t, a.channels, a.lat_h, a.lat_w = 1 << 22, 4, 64, 64
    a.word_sums, a.mask_out = 1 << 23, 1 << 24
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw", [dict(n_prompts=17), dict(map_res=17), dict(n_words=129), dict(n_maps=9),
                                dict(x_t=None, mask_out=None), dict(n_prompts=0), dict(n_maps=0),
                                dict(alpha_layers=None), dict(word_sums=None), dict(lat_h=0), dict(lat_w=0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_localblend_rejects_past_its_limits(kw):
    """The limits include/p2p_hip.h states for p2p_localblend: one past each is P2P_E_ARG."""
    assert _hip.lib().p2p_localblend(ctypes.byref(_blend_args(**kw)), None) == -1


def _step_args(cls, kw):
    """p2p_latent_step / p2p_plms_step arguments of the one-launch LocalBlend form, inside every
    limit (dummy pointers)."""
    a = cls()
    a.eps, a.x, a.out = 1024, 2048, 4096
    a.eps_dtype, a.cfg, a.guidance = 0, 1, 7.5
    a.n_prompts, a.channels, a.height, a.width = 4, 4, 64, 64
    a.blend_sums[0], a.blend_lh, a.blend_res = 1 << 20, 40, 16
    a.blend_th_pool, a.blend_th_sub = 0.3, 0.3
    if cls is _hip.PlmsArgs:
        a.n_hist, a.w[0], a.sample_coeff, a.eps_num, a.eps_den = 0, 1.0, 1.01, 0.02, 0.5
    else:
        a.sqrt_beta_t, a.sqrt_alpha_t, a.sqrt_alpha_prev, a.sqrt_one_minus_alpha_prev = 0.6, 0.8, 0.85, 0.52
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("entry", ["p2p_latent_step", "p2p_plms_step"])
@pytest.mark.parametrize("kw", [dict(height=12), dict(width=12), dict(height=17, width=17), dict(blend_res=17),
                                dict(x=2052), dict(out=4100), dict(eps=1028), dict(mask=512), dict(group_blend=512),
                                dict(out=2048), dict(blend_lh=0), dict(blend_res=0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_one_launch_latent_step_rejects(entry, kw):
    """The one-launch LocalBlend form's conditions (blend_res <= height, width; height * width % 4
    == 0; blend_res^2 <= 256; x, out, eps 16-byte aligned; no mask as well): P2P_E_ARG, before any
    launch (no GPU is needed to be refused)."""
    cls = _hip.PlmsArgs if entry == "p2p_plms_step" else _hip.LatentArgs
    assert getattr(_hip.lib(), entry)(ctypes.byref(_step_args(cls, kw)), None) == -1


def test_clock_probe_rejects():
    L = _hip.lib()
    assert L.p2p_clock_probe(None, 8, 1000, None) == -1
    assert L.p2p_clock_probe(64, 0, 1000, None) == -1
    assert L.p2p_clock_probe(64, 8, 0, None) == -1
    assert L.p2p_clock_probe(64, 2048, 1000, None) == -1


def test_cross_attn_rejects_program_with_too_few_edits():
    """a group of 4 prompts needs a program with >= 3 edit records; one built for fewer
    would make the kernel read past the program blob and the alpha row."""
    L = _hip.lib()
    t = _tensors(n_key=77)
    G = (_hip.Group * 2)()
    G[0].first, G[0].count = 0, 4
    G[1].first, G[1].count = 4, 4
    G[1].program, G[1].alpha, G[1].n_edits = 64, 128, 2
    assert L.p2p_cross_attn_fwd(ctypes.byref(t), G, 2, None, None, 0, None) == -5


def test_library_built_from_this_tree():
    """The Makefile stamps the source hash; a stale prebuilt library fails this check."""
    from p2p_amd import _srchash
    assert _hip.lib().p2p_source_hash().decode() == _srchash.source_hash()
    assert _hip.check_source_hash() == _srchash.source_hash()


def test_production_library_ignores_variant_env(monkeypatch):
    """kernel variants are an experiments-build feature read once at load; the
    production build never reads P2P_SELF_VARIANT (its getenv is compiled out)."""
    import subprocess
    out = subprocess.run(["strings", _hip.library_path()], capture_output=True, text=True).stdout
    assert "P2P_SELF_VARIANT" not in out


# ---------------------------------------------------------------------------- operand layout contract
# include/p2p_hip.h: for every operand a call needs, row stride >= n_heads * head_dim, batch stride
# >= 0 (0 is a broadcast entry, legal on q / k / v), o's batch entries apart, and the operand's span
# within a 32-bit byte offset -- else P2P_E_ARG, before anything is launched.
C, ROWS_Q, ROWS_K = 320, 4096, 77           # _tensors' channels; the rows the calls below see
G_ALL = (_hip.Group * 1)()
G_ALL[0].first, G_ALL[0].count = 0, 8

LAYOUT_CALLS = {   # entry point -> (operands it needs, the call with dummy pointers)
    "p2p_self_attn_fwd": ("qkvo", lambda L, t: L.p2p_self_attn_fwd(ctypes.byref(t), None, None, None, 0, None, None)),
    "p2p_cross_attn_fwd": ("qkvo", lambda L, t: L.p2p_cross_attn_fwd(ctypes.byref(t), G_ALL, 1, None, None, 0, None)),
    "p2p_attn_probs": ("qk", lambda L, t: L.p2p_attn_probs(ctypes.byref(t), None, 64, None)),
    "p2p_attn_pv": ("vo", lambda L, t: L.p2p_attn_pv(ctypes.byref(t), 64, None)),
    "p2p_attn_fwd_lse": ("qkvo", lambda L, t: L.p2p_attn_fwd_lse(ctypes.byref(t), 64, None)),
}


def _layout_tensors(**kw):
    """_tensors with n_key = 77 (what the cross call takes) and k / v batch strides to match."""
    base = dict(n_key=ROWS_K, k_batch_stride=C * ROWS_K, v_batch_stride=C * ROWS_K)
    base.update(kw)
    return _tensors(**base)


def _layout_violations(op, es=4):
    rows = ROWS_Q if op in "qo" else ROWS_K
    wide = 1 << 24                          # 76 rows x 2^24 elements x 2 bytes is already past INT32_MAX
    bad = {
        "rows_overlap": {f"{op}_row_stride": C - 8},
        "negative_row_stride": {f"{op}_row_stride": -C},
        "negative_batch_stride": {f"{op}_batch_stride": -C * rows},
        # batch entries apart, so that nothing but the span is wrong
        "span_past_int32": {f"{op}_row_stride": wide, f"{op}_batch_stride": wide * rows},
    }
    if op == "o":
        bad["batch_entries_overlap"] = {"o_batch_stride": (rows - 1) * C + C - 8}
        bad["zero_batch_stride_on_o"] = {"o_batch_stride": 0}
    return bad


LAYOUT_REJECTS = [pytest.param(fn, kw, id=f"{fn}-{op}-{rule}") for fn, (needs, _) in LAYOUT_CALLS.items()
                  for op in needs for rule, kw in _layout_violations(op).items()]


@pytest.mark.parametrize("fn,kw", LAYOUT_REJECTS)
def test_attn_rejects_a_layout_violation(fn, kw):
    L = _hip.lib()
    call = LAYOUT_CALLS[fn][1]
    assert call(L, _layout_tensors(io_dtype=1, **kw)) == -1
    # the same violation on 4-byte elements (the autograd forward and the check mode take them)
    assert call(L, _layout_tensors(**kw)) == -1


def test_layout_rules_through_the_selection_query():
    """The queries validate as the forward calls do and launch nothing, so they can also show what the
    rules ACCEPT: the exact span limit, broadcast q / k / v entries, one batch entry of o."""
    def accepted(**kw):
        return _hip.self_attn_kernel(_tensors(**kw)) is not None

    assert accepted()
    # f32, P = K = 4096, C = 320: (4095 ld + 320) x 4 <= INT32_MAX  <=>  ld <= 131103
    for op in "qkvo":
        assert accepted(**{f"{op}_row_stride": 131100, f"{op}_batch_stride": 131100 * 4096})
        assert not accepted(**{f"{op}_row_stride": 131104, f"{op}_batch_stride": 131104 * 4096})
    assert accepted(q_batch_stride=0, k_batch_stride=0, v_batch_stride=0)
    assert not accepted(o_batch_stride=0)
    assert accepted(o_batch_stride=0, n_batch=1)
    assert accepted(o_batch_stride=4095 * 320 + 320) and not accepted(o_batch_stride=4095 * 320 + 320 - 4)
    # padded rows: the bound follows the row stride in use
    assert accepted(o_row_stride=328, o_batch_stride=4095 * 328 + 320)
    assert not accepted(o_row_stride=328, o_batch_stride=4095 * 328 + 320 - 8)


def test_production_strides_pass_the_layout_rules():
    """What ptp_utils._project hands the kernels: q, k, v column slices of one [N, P, 3C] projection
    (self), k, v slices of the cached [N, 77, 2C] one (cross), bf16, and the largest span the product
    has (P = 4096 rows of 1536 elements, 12 MB)."""
    P = 4096
    t = _tensors(io_dtype=1, q_row_stride=3 * C, k_row_stride=3 * C, v_row_stride=3 * C, q_batch_stride=3 * C * P,
                 k_batch_stride=3 * C * P, v_batch_stride=3 * C * P, q=16, k=16 + 2 * C, v=16 + 4 * C)
    assert _hip.self_attn_kernel(t) == "self40_kernel<40,8,2,256>"
    assert _hip.self_attn_kernel(t, keeps_maps=True) == "self_attn_fused_kernel<…,D,64,8,EXACT>"
    t = _tensors(io_dtype=1, n_key=77, k_row_stride=2 * C, v_row_stride=2 * C, k_batch_stride=2 * C * 77,
                 v_batch_stride=2 * C * 77, k=16, v=16 + 2 * C)
    G = (_hip.Group * 2)()
    G[0].first, G[0].count = 0, 4
    G[1].first, G[1].count = 4, 4
    assert _hip.cross_attn_kernel(t, G) == "cross_group_kernel<D,4>"
    # the uncond prompts as one broadcast entry
    t.k_batch_stride = t.v_batch_stride = 0
    assert _hip.cross_attn_kernel(t, G) == "cross_group_kernel<D,4>"
    t = _tensors(io_dtype=1, n_heads=8, head_dim=64, q_row_stride=1536, k_row_stride=1536, v_row_stride=1536,
                 o_row_stride=512, q_batch_stride=1536 * P, k_batch_stride=1536 * P, v_batch_stride=1536 * P,
                 o_batch_stride=512 * P)
    assert _hip.self_attn_kernel(t) == "self_attn_fused_kernel<…,D,64,4>"
