"""The attention-map figures as far as a CPU can check them: the resize tables against PIL itself,
view_images / text_under_image against the reference's formulas, the two new entry points'
declarations and argument checks (no launch), and the figure functions on a hand-built CPU store.
Expected values are torch / NumPy / PIL expressions written here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from p2p_amd import _hip, controllers, null_text, ptp_utils
from p2p_amd.tokenizer import StandInTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_ALIGN = -1, -6


# ------------------------------------------------------------------ the resize, restated
def np_resize(u8, S):
    """PIL's 8-bit bicubic of a square uint8 image to S x S from _hip.resize_coeffs: integer taps,
    the accumulator from 2^21, shift, clamp; the horizontal pass first, rounded to uint8."""
    coeffs, bounds = _hip.resize_coeffs(u8.shape[0], S)

    def along_rows(img):
        out = np.empty((img.shape[0], S), np.uint8)
        for xx in range(S):
            x0, n = bounds[xx]
            acc = (1 << 21) + img[:, x0:x0 + n].astype(np.int64) @ coeffs[xx, :n].astype(np.int64)
            out[:, xx] = np.clip(acc >> 22, 0, 255)
        return out

    return along_rows(along_rows(u8).T).T


def pil_resize(u8, S):
    rgb = np.repeat(u8[:, :, None], 3, axis=2)
    out = np.array(Image.fromarray(rgb).resize((S, S)))
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    return out[..., 0]


@pytest.mark.parametrize("res", [3, 8, 12, 16, 33, 64])
@pytest.mark.parametrize("S", [64, 100, 256])
def test_resize_tables_reproduce_pil(res, S):
    rng = np.random.default_rng(res * 1000 + S)
    coeffs, bounds = _hip.resize_coeffs(res, S)
    assert coeffs.shape == (S, _hip.RESIZE_TAPS) and coeffs.dtype == np.int32
    assert bounds.shape == (S, 2) and bounds.min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= res
    inputs = [rng.integers(0, 256, (res, res), dtype=np.uint8),
              ((rng.random((res, res)) < 0.1) * 255).astype(np.uint8),
              np.full((res, res), 255, np.uint8)]
    for u8 in inputs:
        assert np.array_equal(np_resize(u8, S), pil_resize(u8, S))


# ------------------------------------------------------------------ view_images, text_under_image
def grid_formula(images, num_rows, offset_ratio=0.02):
    h, w, _ = images[0].shape
    off = int(h * offset_ratio)
    cols = len(images) // num_rows
    want = np.full((h * num_rows + off * (num_rows - 1), w * cols + off * (cols - 1), 3), 255, np.uint8)
    for i in range(num_rows):
        for j in range(cols):
            want[i * (h + off):i * (h + off) + h, j * (w + off):j * (w + off) + w] = images[i * cols + j]
    return want


def _images(n, h=50, w=40, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


def test_view_images_list_array_and_single():
    imgs = _images(4)
    got = ptp_utils.view_images(imgs)
    assert isinstance(got, Image.Image)
    assert np.array_equal(np.array(got), grid_formula(imgs, 1))
    assert np.array_equal(np.array(ptp_utils.view_images(np.stack(imgs), num_rows=2)), grid_formula(imgs, 2))
    assert np.array_equal(np.array(ptp_utils.view_images(imgs[0])), imgs[0])


def test_view_images_pads_as_the_reference():
    imgs = _images(5)
    white = np.full_like(imgs[0], 255)
    got = np.array(ptp_utils.view_images(imgs, num_rows=2))       # 5 % 2 = 1 white cell: 6 cells, 2 x 3
    assert np.array_equal(got, grid_formula(imgs + [white], 2))
    assert got.shape == (2 * 50 + 1, 3 * 40 + 2 * 1, 3)


def test_view_images_never_calls_show(monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("Image.show() was called")
    monkeypatch.setattr(Image.Image, "show", boom)
    ptp_utils.view_images(_images(2))


def test_text_under_image():
    img = _images(1, h=64, w=96)[0]
    out = ptp_utils.text_under_image(img, "burger")
    assert out.dtype == np.uint8 and out.shape == (64 + int(.2 * 64), 96, 3)
    assert np.array_equal(out[:64], img)
    assert (out[64:] != 255).any()
    blank = ptp_utils.text_under_image(img, "")
    assert (blank[64:] == 255).all()


def test_top_level_module_has_the_names():
    import ptp_utils as top
    assert top.view_images is ptp_utils.view_images and top.text_under_image is ptp_utils.text_under_image
    for name in ("aggregate_attention_device", "cross_attention_panels", "show_cross_attention",
                 "self_attention_components", "show_self_attention_comp"):
        assert getattr(null_text, name) is getattr(controllers, name)


# ------------------------------------------------------------------ symbols and arguments
def test_symbols_are_declared_exported_and_bound():
    L = _hip.lib()
    assert L.p2p_abi_version() == 16 == _hip.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    assert re.search(r"^int\s+p2p_maps_aggregate\s*\(const p2p_maps_aggregate_args\*", text, flags=re.M)
    assert re.search(r"^int\s+p2p_map_panels\s*\(const p2p_map_panels_args\*", text, flags=re.M)
    assert re.search(r"#define\s+P2P_ABI_VERSION\s+16\b", text)
    for fn in ("p2p_maps_aggregate", "p2p_map_panels"):
        assert fn in _hip.EXPORTED_SYMBOLS and hasattr(L, fn)
    assert int(re.search(r"#define\s+P2P_MAX_AGG_LAYERS\s+(\d+)", text).group(1)) == _hip.MAX_AGG_LAYERS == 16
    assert int(re.search(r"#define\s+P2P_RESIZE_TAPS\s+(\d+)", text).group(1)) == _hip.RESIZE_TAPS
    from p2p_amd import _srchash
    assert "p2p_viz.hip" in _srchash.SOURCES


def _agg(**kw):
    a = _hip.MapsAggregateArgs()
    for i in range(2):
        a.stores[i], a.heads[i] = 4096 * (i + 1), 8
    a.n_layers, a.n_prompts, a.select, a.P, a.K, a.steps, a.out = 2, 3, 1, 256, 77, 5, 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_maps_aggregate_rejects_before_any_launch():
    f = _hip.lib().p2p_maps_aggregate
    assert f(None, None) == E_ARG
    assert f(ctypes.byref(_agg(out=None)), None) == E_ARG
    assert f(ctypes.byref(_agg(select=3)), None) == E_ARG          # select == n_prompts
    assert f(ctypes.byref(_agg(select=-1)), None) == E_ARG
    assert f(ctypes.byref(_agg(steps=0)), None) == E_ARG
    assert f(ctypes.byref(_agg(n_layers=17)), None) == E_ARG
    assert f(ctypes.byref(_agg(n_layers=0)), None) == E_ARG
    a = _agg()
    a.heads[1] = 0
    assert f(ctypes.byref(a), None) == E_ARG
    a = _agg()
    a.stores[1] = None
    assert f(ctypes.byref(a), None) == E_ARG
    assert f(ctypes.byref(_agg(P=9, K=77)), None) == E_ALIGN       # P * K % 4 != 0
    a = _agg()
    a.stores[0] = 4096 + 8
    assert f(ctypes.byref(a), None) == E_ALIGN
    assert f(ctypes.byref(_agg(out=(1 << 20) + 4)), None) == E_ALIGN


def _pan(**kw):
    a = _hip.MapPanelsArgs()
    a.inp, a.coeffs, a.bounds, a.out = 4096, 8192, 16384, 1 << 20
    a.panel_stride, a.pixel_stride = 1, 77
    a.res, a.n, a.S, a.mode = 16, 77, 256, _hip.PANEL_MAX
    a.out_row_stride, a.out_panel_stride = 3 * 256, 3 * 256 * 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_map_panels_rejects_before_any_launch():
    f = _hip.lib().p2p_map_panels
    assert f(None, None) == E_ARG
    for name in ("inp", "coeffs", "bounds", "out"):
        assert f(ctypes.byref(_pan(**{name: None})), None) == E_ARG
    assert f(ctypes.byref(_pan(res=65)), None) == E_ARG
    assert f(ctypes.byref(_pan(res=0)), None) == E_ARG
    assert f(ctypes.byref(_pan(S=258, out_row_stride=3 * 260)), None) == E_ARG     # S % 4 != 0
    assert f(ctypes.byref(_pan(S=516, out_row_stride=3 * 516)), None) == E_ARG     # S > 512
    assert f(ctypes.byref(_pan(S=12, out_row_stride=36)), None) == E_ARG           # S < res
    assert f(ctypes.byref(_pan(mode=2)), None) == E_ARG
    assert f(ctypes.byref(_pan(mode=-1)), None) == E_ARG
    assert f(ctypes.byref(_pan(n=0)), None) == E_ARG
    assert f(ctypes.byref(_pan(out_row_stride=3 * 256 - 4)), None) == E_ARG        # rows would overlap
    assert f(ctypes.byref(_pan(out=(1 << 20) + 2)), None) == E_ALIGN
    assert f(ctypes.byref(_pan(out_row_stride=3 * 256 + 2)), None) == E_ALIGN


def test_bindings_return_none_off_the_gpu():
    stores = [torch.rand(6, 16, 8)]
    assert _hip.maps_aggregate(stores, 3, 0, 2) is None
    assert _hip.map_panels(torch.rand(3, 16), 3, 4, 64, _hip.PANEL_MINMAX, 16, 1) is None
    assert not _hip.map_panels_supported(65, 256) and not _hip.map_panels_supported(16, 258)
    assert not _hip.map_panels_supported(16, 8) and _hip.map_panels_supported(64, 512)


# ------------------------------------------------------------------ the figure functions, CPU store
PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a lion eating a lasagna"]
RES, HEADS, SIZE = 4, 2, 64


@pytest.fixture(scope="module")
def cpu_store():
    g = torch.Generator().manual_seed(7)
    s = controllers.AttentionStore()
    s.attention_store = s.get_empty_store()
    n = len(PROMPTS) * HEADS
    for place in ("down", "up"):
        s.attention_store[f"{place}_cross"].append(torch.rand(n, RES * RES, 77, generator=g) * 2)
        s.attention_store[f"{place}_cross"].append(torch.rand(n, 4 * RES * RES, 77, generator=g))   # another res
        s.attention_store[f"{place}_self"].append(torch.rand(n, RES * RES, RES * RES, generator=g) * 2)
    s.cur_step = 2
    return s


def panel_expr(x, size, minmax):
    if minmax:
        x = x - x.min()
    grey = (255 * x / x.max()).numpy().astype(np.uint8)
    return np.array(Image.fromarray(np.repeat(grey[:, :, None], 3, axis=2)).resize((size, size)))


def test_aggregate_device_on_a_cpu_store(cpu_store):
    for is_cross in (True, False):
        want = controllers.aggregate_attention(cpu_store, RES, ["up", "down"], is_cross, 1, PROMPTS)
        got = controllers.aggregate_attention_device(cpu_store, RES, ["up", "down"], is_cross, 1, PROMPTS)
        assert got.shape == want.shape and torch.equal(got, want)
    with pytest.raises(IndexError):
        controllers.aggregate_attention_device(cpu_store, RES, ["up"], True, 2, PROMPTS)
    with pytest.raises(ValueError, match="no stored cross maps at 3x3"):
        controllers.aggregate_attention_device(cpu_store, 3, ["up"], True, 0, PROMPTS)


def test_cross_panels_on_a_cpu_store(cpu_store):
    tok = StandInTokenizer()
    agg = controllers.aggregate_attention(cpu_store, RES, ["up", "down"], True, 1, PROMPTS)
    n = len(tok.encode(PROMPTS[1]))
    got = controllers.cross_attention_panels(cpu_store, RES, ["up", "down"], 1, PROMPTS, tok, size=SIZE)
    assert got.dtype == np.uint8 and got.shape == (n, SIZE, SIZE, 3)
    for i in range(n):
        assert np.array_equal(got[i], panel_expr(agg[:, :, i], SIZE, False))
    img = controllers.show_cross_attention(cpu_store, RES, ["up", "down"], 1, PROMPTS, tok)
    assert img.size == (256 * n + 6 * (n - 1), 307)
    top = np.array(img)[:256, :256]
    assert np.array_equal(top, panel_expr(agg[:, :, 0], 256, False))


def test_self_components_on_a_cpu_store(cpu_store):
    agg = controllers.aggregate_attention(cpu_store, RES, ["up", "down"], False, 0, PROMPTS)
    m = agg.numpy().reshape(RES ** 2, RES ** 2)
    _, _, vh = np.linalg.svd(m - np.mean(m, axis=1, keepdims=True))
    comps = controllers.self_attention_components(cpu_store, RES, ["up", "down"], 5, 0, PROMPTS)
    assert comps.dtype == np.float32 and np.array_equal(comps, vh[:5])
    img = controllers.show_self_attention_comp(cpu_store, RES, ["up", "down"], 5, 0, PROMPTS, size=SIZE)
    want = np.concatenate([panel_expr(torch.from_numpy(vh[i].reshape(RES, RES)), SIZE, True) for i in range(5)], axis=1)
    assert np.array_equal(np.array(img), want)


def test_no_self_maps_is_a_value_error(cpu_store):
    s = controllers.AttentionStore()
    s.store_self_maps = False
    s.attention_store = {k: (v if "cross" in k else []) for k, v in cpu_store.attention_store.items()}
    s.cur_step = 2
    with pytest.raises(ValueError, match="store_self_maps = False"):
        controllers.show_self_attention_comp(s, RES, ["up", "down"], 5, 0, PROMPTS)
    with pytest.raises(ValueError, match="no stored self maps at 8x8"):
        controllers.show_self_attention_comp(cpu_store, 8, ["up", "down"], 5, 0, PROMPTS)
