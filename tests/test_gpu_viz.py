"""The attention-map figures on the GPU (csrc/p2p_viz.hip): maps_aggregate_kernel bit for bit where
its arithmetic is exact and within the summation-order bound elsewhere, map_panels_kernel byte for
byte against the NumPy + PIL expression, and the public functions on a narrow U-Net's store.
Expected values are torch / NumPy / PIL expressions written here."""
import numpy as np
import pytest
import torch
from PIL import Image

from p2p_amd import _hip, controllers, null_text
from p2p_amd import pipeline as pl

pytestmark = pytest.mark.gpu

TINY = float(np.finfo(np.float32).tiny)      # the absolute floor: the smallest normal f32


def within_order_bound(a, b, n_terms):
    """|a - b| <= 2 n 2^-24 b: the worst case of two f32 summation orders over n non-negative terms
    (each order is within (n - 1) 2^-24 of the exact sum, the two roundings of the final division
    and of the terms take the rest)."""
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a - b).abs() <= 2 * n_terms * 2.0 ** -24 * b.abs() + TINY).all())


def torch_aggregate(stores, n_prompts, select, steps):
    """aggregate_attention's lines on the host, where torch divides by a scalar with an IEEE division
    (on the GPU it multiplies by the reciprocal, which is another rounding of every term)."""
    picked = [(s.cpu() / steps).reshape(n_prompts, -1, *s.shape[1:])[select] for s in stores]
    out = torch.cat(picked, dim=0)
    return out.sum(0) / out.shape[0]


def make_stores(cuda, heads, n_prompts, P, K, seed=0):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return [torch.rand(n_prompts * h, P, K, device=cuda, generator=g) * 3 for h in heads]


# ------------------------------------------------------------------ aggregate, exact cases
@pytest.mark.parametrize("steps", [1, 3])
def test_aggregate_one_term_is_exact(cuda, steps):
    (s,) = make_stores(cuda, [1], 3, 64, 77)
    s[2, 0, :4] = torch.tensor([0.0, -0.0, 1e-40, 3.0], device=cuda)
    got = _hip.maps_aggregate([s], 3, 2, steps)
    slab = s[2].cpu().numpy()
    want = slab / np.float32(steps) if steps > 1 else slab         # NumPy's f32 division: IEEE
    assert got.shape == (64, 77) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_aggregate_reads_only_the_selected_prompt(cuda):
    stores = make_stores(cuda, [2, 8], 3, 64, 64)
    want = torch_aggregate(stores, 3, 1, 4)
    for s in stores:
        h = s.shape[0] // 3
        s[:h] = float("nan")
        s[2 * h:] = float("nan")
    got = _hip.maps_aggregate(stores, 3, 1, 4)
    assert torch.isfinite(got).all()
    assert within_order_bound(got, want, 10)


# ------------------------------------------------------------------ aggregate, against torch
@pytest.mark.parametrize("heads,P,K,n_prompts,select,steps", [
    ([8] * 5, 256, 77, 3, 2, 50),
    ([2] * 2, 1024, 1024, 2, 1, 7),
    ([1, 2, 8, 8, 2, 1], 64, 64, 2, 0, 3),
])
def test_aggregate_matches_the_torch_expression(cuda, heads, P, K, n_prompts, select, steps):
    stores = make_stores(cuda, heads, n_prompts, P, K, seed=P + K)
    got = _hip.maps_aggregate(stores, n_prompts, select, steps)
    want = torch_aggregate(stores, n_prompts, select, steps)
    assert got.shape == want.shape
    assert within_order_bound(got, want, sum(heads))


def _store_of(stores_by_key, steps):
    s = controllers.AttentionStore()
    s.attention_store = s.get_empty_store()
    for key, lst in stores_by_key.items():
        s.attention_store[key] = list(lst)
    s.cur_step = steps
    return s


def test_odd_sizes_answer_through_torch(cuda):
    stores = make_stores(cuda, [2, 2], 2, 9, 77)           # P * K = 693: not a multiple of 4
    assert _hip.maps_aggregate(stores, 2, 1, 3) is None
    store = _store_of({"down_cross": stores[:1], "up_cross": stores[1:]}, 3)
    prompts = ["a", "b"]
    got = controllers.aggregate_attention_device(store, 3, ["up", "down"], True, 1, prompts)
    want = controllers.aggregate_attention(store, 3, ["up", "down"], True, 1, prompts)
    assert got.is_cuda and got.shape == (3, 3, 77)
    assert within_order_bound(got, want, 4)
    assert _hip.maps_aggregate(make_stores(cuda, [1] * 17, 1, 4, 4), 1, 0, 1) is None     # 17 layers


# ------------------------------------------------------------------ panels
def panel_expr(x, S, minmax):
    """x: a CPU f32 tensor [res, res].  A panel whose divisor is 0, or that holds a NaN: zeros."""
    if minmax:
        x = x - x.min()
    m = x.max()
    if torch.isnan(x).any() or m == 0:
        return np.zeros((S, S, 3), np.uint8)
    grey = (255 * x / m).numpy().astype(np.uint8)
    return np.array(Image.fromarray(np.repeat(grey[:, :, None], 3, axis=2)).resize((S, S)))


def special_rows(res, rows):
    """rows [n >= 6, res^2]: the first six replaced by the edge cases."""
    rows[0] = 0.3                                     # constant: 255 * .3 / .3 truncates to 254 in f32
    rows[1] = 0
    rows[1, (res * res) // 3] = 1.0                   # one hot pixel
    rows[2] = 0                                       # all zero
    rows[3, res * res - 1] = float("nan")             # holds a NaN
    rows[4] = rows[4] * 1e-30                         # tiny values
    rows[5, 0] = rows[5].max() * 4                    # one dominant corner
    return rows


@pytest.mark.parametrize("mode", [_hip.PANEL_MAX, _hip.PANEL_MINMAX])
@pytest.mark.parametrize("res,S", [(8, 256), (16, 256), (32, 256), (64, 256), (12, 100)])
def test_panels_rows_layout_is_byte_exact(cuda, mode, res, S):
    g = torch.Generator().manual_seed(res + S + mode)
    rows = torch.rand(7, res * res, generator=g) if mode == _hip.PANEL_MAX else torch.randn(7, res * res, generator=g)
    rows = special_rows(res, rows)
    got = _hip.map_panels(rows.to(cuda), 7, res, S, mode, res * res, 1)
    assert got.shape == (7, S, S, 3) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    for i in range(7):
        assert np.array_equal(got[i], panel_expr(rows[i].reshape(res, res), S, mode == _hip.PANEL_MINMAX)), i
    if mode == _hip.PANEL_MAX:
        assert (got[0] == 254).all()
    assert not got[2].any() and not got[3].any()


@pytest.mark.parametrize("mode", [_hip.PANEL_MAX, _hip.PANEL_MINMAX])
def test_panels_columns_of_a_cross_map(cuda, mode):
    g = torch.Generator().manual_seed(3)
    maps = torch.rand(256, 77, generator=g) ** 4           # [res^2, K]: panel i is column i
    got = _hip.map_panels(maps.to(cuda), 77, 16, 256, mode, 1, 77).cpu().numpy()
    assert got.shape == (77, 256, 256, 3)
    for i in range(77):
        assert np.array_equal(got[i], panel_expr(maps[:, i].reshape(16, 16), 256, mode == _hip.PANEL_MINMAX)), i


def test_panels_one_panel_and_an_offset_view(cuda):
    g = torch.Generator().manual_seed(4)
    maps = torch.rand(5, 16 * 16, generator=g)
    dev = maps.to(cuda)
    got = _hip.map_panels(dev[3:].contiguous(), 1, 16, 64, _hip.PANEL_MAX, 256, 1).cpu().numpy()
    assert np.array_equal(got[0], panel_expr(maps[3].reshape(16, 16), 64, False))
    # a view that starts 4 bytes past a 16-byte boundary: the scalar load path
    flat = torch.cat([torch.zeros(1), maps[2]]).to(cuda)[1:]
    got = _hip.map_panels(flat, 1, 16, 64, _hip.PANEL_MINMAX, 256, 1).cpu().numpy()
    assert np.array_equal(got[0], panel_expr(maps[2].reshape(16, 16), 64, True))


def test_panels_into_a_wider_canvas(cuda):
    res, S, n = 16, 64, 3
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(n, res * res, generator=g)
    H, W = S + 8, n * S + 16
    canvas = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=cuda)
    y0, x0 = 4, 8
    view = canvas.view(-1)[(y0 * W + x0) * 3:]
    out = _hip.map_panels(rows.to(cuda), n, res, S, _hip.PANEL_MINMAX, res * res, 1, out=view,
                          out_row_stride=3 * W, out_panel_stride=3 * S)
    assert out is view
    want = np.full((H, W, 3), 0xA5, np.uint8)
    for i in range(n):
        want[y0:y0 + S, x0 + i * S:x0 + (i + 1) * S] = panel_expr(rows[i].reshape(res, res), S, True)
    assert np.array_equal(canvas.cpu().numpy(), want)
    need = (n - 1) * 3 * S + (S - 1) * 3 * W + 3 * S       # bytes from the view's start to the last pixel's end
    with pytest.raises(_hip.HipError):                     # a canvas one byte short: refused, nothing launched
        _hip.map_panels(rows.to(cuda), n, res, S, _hip.PANEL_MINMAX, res * res, 1, out=view[:need - 1],
                        out_row_stride=3 * W, out_panel_stride=3 * S)
    assert np.array_equal(canvas.cpu().numpy(), want)


def test_panels_unsupported_sizes_return_none(cuda):
    x = torch.rand(2, 65 * 65, device=cuda)
    assert _hip.map_panels(x, 2, 65, 256, _hip.PANEL_MAX, 65 * 65, 1) is None
    assert _hip.map_panels(x, 2, 16, 258, _hip.PANEL_MAX, 256, 1) is None


# ------------------------------------------------------------------ end to end
SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128))
PROMPTS = pl.north_star_prompts()[:3]


@pytest.fixture(scope="module")
def run(cuda):
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, scheduler="ddim", unet_config=SMALL_UNET)
    ctrl = controllers.AttentionStore()
    pl.run_edit_group(model, PROMPTS, ctrl, pl.seed_latent(0), num_steps=2)
    assert ctrl.cur_step == 2
    return ctrl


def _n_terms(ctrl, res, from_where, is_cross):
    kind = "cross" if is_cross else "self"
    return sum(t.shape[0] // len(PROMPTS) for w in from_where for t in ctrl.attention_store[f"{w}_{kind}"]
               if t.shape[1] == res * res)


@pytest.mark.parametrize("res,from_where,is_cross", [(8, ("up", "down", "mid"), True), (16, ("up", "down"), True),
                                                     (32, ("up", "down"), True), (16, ("up", "down"), False)])
def test_device_aggregate_matches_aggregate_attention(run, res, from_where, is_cross):
    n = _n_terms(run, res, from_where, is_cross)
    assert n > 0
    for select in (0, 2):
        got = null_text.aggregate_attention_device(run, res, list(from_where), is_cross, select, PROMPTS)
        want = controllers.aggregate_attention(run, res, list(from_where), is_cross, select, PROMPTS)
        assert got.is_cuda and got.shape == want.shape
        assert within_order_bound(got, want, n)


def test_cross_panels_and_the_strip(run, tok):
    agg = controllers.aggregate_attention_device(run, 16, ["up", "down"], True, 1, PROMPTS).cpu()
    n = len(tok.encode(PROMPTS[1]))
    got = controllers.cross_attention_panels(run, 16, ["up", "down"], 1, PROMPTS, tok)
    assert got.dtype == np.uint8 and got.shape == (n, 256, 256, 3)
    for i in range(n):
        assert np.array_equal(got[i], panel_expr(agg[:, :, i], 256, False)), i
    img = controllers.show_cross_attention(run, 16, ["up", "down"], 1, PROMPTS, tok)
    assert img.size == (256 * n + 6 * (n - 1), 307)
    assert np.array_equal(np.array(img)[:256, :256], got[0])


def test_self_components_strip(run):
    comps = controllers.self_attention_components(run, 16, ["up", "down"], 6, 0, PROMPTS)
    assert comps.shape == (6, 256) and comps.dtype == np.float32
    img = controllers.show_self_attention_comp(run, 16, ["up", "down"], 6, 0, PROMPTS)
    want = np.concatenate([panel_expr(torch.from_numpy(comps[i].reshape(16, 16)), 256, True) for i in range(6)], axis=1)
    assert np.array_equal(np.array(img), want)


def test_without_self_maps_the_figure_says_so(run):
    ctrl = controllers.AttentionStore()
    ctrl.store_self_maps = False
    ctrl.attention_store = {k: (v if "cross" in k else []) for k, v in run.attention_store.items()}
    ctrl.cur_step = run.cur_step
    with pytest.raises(ValueError, match="store_self_maps = False"):
        controllers.show_self_attention_comp(ctrl, 16, ["up", "down"], 6, 0, PROMPTS)
