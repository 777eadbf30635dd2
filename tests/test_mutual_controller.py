"""controllers.MutualSelfAttentionControl on CPU tensors (its torch lines), and the float64 reference
of tests/mutual_ref.py against a second formulation and a case worked by hand.

The "U-Net" here is the SD sequence of 16 attention blocks (self then cross) at reduced sizes: 33x33
stands for the 64x64 layers (above MAX_STORED_QUERIES, so not stored), 20x20 for the 32x32 ones, and
the 16x16 and 8x8 layers are themselves (the word sums fold the five 16x16 cross layers)."""
import math

import pytest
import torch

from mutual_ref import mutual_ref, mutual_ref_dense, token_classes_ref
from p2p_amd import controllers as C

LAYERS = ([("down", 33)] * 2 + [("down", 20)] * 2 + [("down", 16)] * 2 + [("mid", 8)] + [("up", 16)] * 3 +
          [("up", 20)] * 3 + [("up", 33)] * 3)
PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a squirrel jumping over a burger"]
H, D, STEPS = 1, 8, 6
N = 2 * len(PROMPTS)
KV_SRC = [0, 0, 2, 2]                       # uncond edit <- uncond source, cond edit <- cond source


def drive(ctrl, steps=STEPS, seed=0):
    """Run `steps` denoising steps of the layer sequence; returns the self calls as dicts."""
    g = torch.Generator().manual_seed(seed)
    ctrl.num_att_layers = 2 * len(LAYERS)
    calls = []
    for step in range(steps):
        for layer, (place, side) in enumerate(LAYERS):
            P = side * side
            q, k, v = (torch.randn(N, P, H * D, generator=g) for _ in range(3))
            out = ctrl.attention(q, k, v, H, D ** -0.5, False, place)
            calls.append(dict(step=step, layer=layer, q=q, k=k, v=v, out=out))
            qc = torch.randn(N, P, H * D, generator=g)
            kc, vc = (torch.randn(N, 77, H * D, generator=g) for _ in range(2))
            ctrl.attention(qc, kc, vc, H, D ** -0.5, True, place)
    assert ctrl.cur_step == steps and ctrl.cur_att_layer == 0
    return calls


def plain(c):
    return mutual_ref(c["q"], c["k"], c["v"], H, D ** -0.5)


@pytest.fixture()
def observed():
    seen = []
    # (the classes live in a tensor the controller refills every step: keep a copy)
    C.MUTUAL_OBSERVER = lambda info: seen.append(
        {**info, "token_class": None if info["token_class"] is None else info["token_class"].clone()})
    yield seen
    C.MUTUAL_OBSERVER = None


def test_window_halves_and_sources(tok, observed):
    ctrl = C.MutualSelfAttentionControl(PROMPTS, STEPS, tokenizer=tok, device="cpu")
    assert ctrl.store_self_maps is False and (ctrl.start_step, ctrl.start_layer) == (4, 10)
    calls = drive(ctrl)
    active = [(c["step"], c["layer"]) for c in calls if c["step"] >= 4 and c["layer"] >= 10]
    assert len(active) == 2 * 6 and len(observed) == len(active)
    assert all(info["kv_src"] == KV_SRC and info["token_class"] is None for info in observed)
    for c in calls:
        want_plain = plain(c)
        if (c["step"], c["layer"]) not in active:
            # steps 0..3 and layers 0..9: plain attention, every row
            assert (c["out"].double() - want_plain).abs().max().item() < 1e-5, (c["step"], c["layer"])
            continue
        want = mutual_ref(c["q"], c["k"], c["v"], H, D ** -0.5, KV_SRC)
        assert (c["out"].double() - want).abs().max().item() < 1e-5
        # both halves are remapped: each edit row differs from its own plain attention ...
        for n in (1, 3):
            assert (c["out"][n].double() - want_plain[n]).abs().max().item() > 1e-2
        # ... and the source rows are untouched
        for n in (0, 2):
            assert (c["out"][n].double() - want_plain[n]).abs().max().item() < 1e-5
    # the cross maps are kept as an AttentionStore keeps them, the self maps are not
    assert len(ctrl.attention_store["down_cross"]) == 4 and len(ctrl.attention_store["up_cross"]) == 6
    assert not ctrl.attention_store["down_self"] and not ctrl.attention_store["up_self"]


def test_window_arguments(tok, observed):
    ctrl = C.MutualSelfAttentionControl(PROMPTS, 3, start_step=1, start_layer=14, tokenizer=tok, device="cpu")
    drive(ctrl, steps=3)
    assert [info["step"] for info in observed] == [1, 1, 2, 2]
    observed.clear()
    never = C.MutualSelfAttentionControl(PROMPTS, 3, start_step=3, tokenizer=tok, device="cpu")
    for c in drive(never, steps=3):
        assert (c["out"].double() - plain(c)).abs().max().item() < 1e-5
    assert not observed


def test_mask_guided_classes_from_the_word_sums(tok, observed):
    ctrl = C.MutualSelfAttentionControl(PROMPTS, STEPS, ref_words=("squirrel", "squirrel"), tokenizer=tok, device="cpu")
    sums_seen = []
    keep = C.MUTUAL_OBSERVER
    C.MUTUAL_OBSERVER = lambda info: (keep(info), sums_seen.append(ctrl._blend_sums.clone()))
    calls = [c for c in drive(ctrl) if c["step"] >= 4 and c["layer"] >= 10]
    assert len(observed) == len(calls) == 12
    for c, info, sums in zip(calls, observed, sums_seen):
        side = int(round(c["q"].shape[1] ** 0.5))
        want_cls, = token_classes_ref([sums], 0.1, [side])
        assert info["token_class"].dtype == torch.uint8 and torch.equal(info["token_class"], want_cls)
        assert torch.equal(want_cls[:2], want_cls[2:])          # uncond rows: the cond rows' classes
        assert 0 < want_cls.sum() < want_cls.numel()
        want = mutual_ref(c["q"], c["k"], c["v"], H, D ** -0.5, KV_SRC, want_cls)
        assert (c["out"].double() - want).abs().max().item() < 1e-5
        unmasked = mutual_ref(c["q"], c["k"], c["v"], H, D ** -0.5, KV_SRC)
        assert (c["out"].double() - unmasked).abs().max().item() > 1e-3
    # the word sums are the ref words' columns of the five 16x16 running-sum cross maps
    maps = ctrl.attention_store["down_cross"][2:4] + ctrl.attention_store["up_cross"][:3]
    alpha = ctrl._ref_alpha
    assert alpha.shape == (2, 77) and (alpha.sum(1) >= 1).all() and ((alpha == 0) | (alpha == 1)).all()   # the word's tokens
    for slot, m in enumerate(maps):
        assert m.shape == (2 * H, 256, 77)
        words = torch.einsum("bhpw,bw->bhp", m.reshape(2, H, 256, 77), alpha)
        assert torch.allclose(ctrl._blend_sums[:, 0, slot * H:(slot + 1) * H], words, rtol=1e-5, atol=1e-6)


def test_forward_raises_in_an_active_layer(tok):
    ctrl = C.MutualSelfAttentionControl(PROMPTS, STEPS, start_step=0, start_layer=1, tokenizer=tok, device="cpu")
    ctrl.num_att_layers = 2 * len(LAYERS)
    attn = torch.rand(N * H, 64, 64)
    ctrl(attn, False, "down")                       # layer 0: outside the window, the plain protocol
    ctrl(torch.rand(N * H, 64, 77), True, "down")
    with pytest.raises(RuntimeError, match="forward"):
        ctrl(attn, False, "down")                   # layer 1


def test_mixing_with_an_edit_controller_raises(tok):
    mutual = C.MutualSelfAttentionControl(PROMPTS, STEPS, tokenizer=tok, device="cpu")
    edit = C.AttentionReplace(["a cat on a mat", "a dog on a mat"], STEPS, .8, .4, tokenizer=tok, device="cpu")
    with pytest.raises(ValueError, match="MutualSelfAttentionControl"):
        C.GroupBatch([mutual, edit])
    C.GroupBatch([mutual, C.MutualSelfAttentionControl(PROMPTS, STEPS, tokenizer=tok, device="cpu")])
    with pytest.raises(ValueError, match="ref_words"):
        C.MutualSelfAttentionControl(PROMPTS, STEPS, ref_words=("squirrel",), tokenizer=tok, device="cpu")


# ------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("masked", [False, True])
def test_reference_formulations_agree(masked):
    g = torch.Generator().manual_seed(3)
    Nn, P, heads, d = 5, 37, 2, 8
    q, k, v = (torch.randn(Nn, P, heads * d, generator=g) for _ in range(3))
    tc = (torch.rand(Nn, P, generator=g) < 0.4).to(torch.uint8) if masked else None
    if masked:
        tc[2] = 1                                 # a source of one class: its class-0 readers fall back
    kv_src = [0, 0, 2, 2, -1]
    keep = torch.randn(Nn, P, heads * d, generator=g)
    a = mutual_ref(q, k, v, heads, 0.3, kv_src, tc, out=keep)
    b = mutual_ref_dense(q, k, v, heads, 0.3, kv_src, tc, out=keep)
    assert (a - b).abs().max().item() < 1e-12
    assert torch.equal(a[4], keep[4].double())
    assert torch.isfinite(a).all()


def test_reference_by_hand_six_tokens():
    """N = 3, P = 6, one head of width 1.  Entry 1 reads entry 0 (both classes there: restricted);
    entry 2 reads entry 1, whose tokens are all class 0, so entry 2's class-1 queries find no key of
    their class and read every key."""
    q = torch.tensor([[.5, -1., 2., 0., 1., -.5], [1., 2., -1., .5, 0., -2.], [2., -1., .5, 1., -.5, 0.]])[..., None]
    k = torch.tensor([[1., 0., -1., 2., .5, -.5], [0., 1., 2., -1., .5, 1.], [1., 1., 1., 1., 1., 1.]])[..., None]
    v = torch.tensor([[1., 2., 3., 4., 5., 6.], [6., 5., 4., 3., 2., 1.], [0., 0., 0., 0., 0., 0.]])[..., None]
    tc = torch.tensor([[1, 1, 0, 0, 0, 1], [0, 1, 1, 0, 0, 0], [0, 1, 0, 1, 0, 0]], dtype=torch.uint8)
    tc[1] = 0                                                   # entry 1 as a SOURCE has one class ...
    tc_q1 = [0, 1, 1, 0, 0, 0]                                  # ... so give its queries' classes by hand below
    kv_src, scale = [0, 0, 1], 0.7

    def row(qv, keys, vals, allowed):
        w = [math.exp(qv * kk * scale) if ok else 0.0 for kk, ok in zip(keys, allowed)]
        return sum(wi * vi for wi, vi in zip(w, vals)) / sum(w)

    k0, v0, k1, v1 = k[0, :, 0].tolist(), v[0, :, 0].tolist(), k[1, :, 0].tolist(), v[1, :, 0].tolist()
    cls0 = tc[0].tolist()
    want = torch.zeros(3, 6, dtype=torch.float64)
    for p in range(6):
        want[0, p] = row(q[0, p, 0].item(), k0, v0, [True] * 6)                               # its own keys
        want[2, p] = row(q[2, p, 0].item(), k1, v1, [True] * 6)     # class 0: all of entry 1; class 1: absent, all
    tc_run = tc.clone()
    tc_run[1] = torch.tensor(tc_q1, dtype=torch.uint8)
    for p in range(6):
        want[1, p] = row(q[1, p, 0].item(), k0, v0, [c == tc_q1[p] for c in cls0])
    # entry 2 must read entry 1 as a one-class source: evaluate it with entry 1's classes zeroed
    got_1 = mutual_ref(q, k, v, 1, scale, [0, 0, -1], tc_run)[1, :, 0]
    got_02 = mutual_ref(q, k, v, 1, scale, [0, -1, 1], tc)[:, :, 0]
    assert (got_1 - want[1]).abs().max().item() < 1e-12
    assert (got_02[0] - want[0]).abs().max().item() < 1e-12
    assert (got_02[2] - want[2]).abs().max().item() < 1e-12
    assert tc[2].sum() == 2 and tc[1].sum() == 0                # entry 2 does hold class-1 queries
    # and the restriction matters: entry 1 unrestricted differs
    free = mutual_ref(q, k, v, 1, scale, [0, 0, -1])[1, :, 0]
    assert (free - want[1]).abs().max().item() > 1e-2
    assert (mutual_ref_dense(q, k, v, 1, scale, [0, -1, 1], tc)[:, :, 0] - got_02).abs().max().item() < 1e-12
