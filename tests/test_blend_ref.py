"""tests/blend_ref.py, the float64 LocalBlend reference of the GPU geometry tests, checked on the
CPU: its nearest-index formula against F.interpolate, the reference against the oracle's LocalBlend
on the golden store, and the two conditions on the inputs the GPU tests draw (few pixels near a
threshold; masks neither empty nor full)."""
import numpy as np
import pytest
import torch

import blend_ref as br
from conftest import golden, golden_json
from oracle import control as oc

LG = golden("localblend")
LM = golden_json("localblend")


def test_kernel_nearest_index_is_interpolates():
    """min(floorf(Y * (float)R / (float)lat), R - 1), the kernel's formula, is F.interpolate's
    source index for every map resolution and latent extent the entry points serve."""
    bad = [(R, lat) for R in range(1, 17) for lat in range(1, 130)
           if not np.array_equal(br.kernel_nearest_index(lat, R), br.interpolate_nearest_index(lat, R))]
    assert not bad, bad


def _words(w):
    return [tuple(x) if isinstance(x, list) else x for x in w]


@pytest.mark.parametrize("ci", range(len(LM)))
def test_reference_agrees_with_the_oracle_on_the_golden_store(ci, tok):
    """Product geometry (five 16x16 layers, 77 words, 64x64 latent): the word-sum reference and the
    mask reference together against oracle.control's LocalBlend (f32, from the maps), except at
    pixels the reference itself flags as near a threshold."""
    case = LM[ci]
    kw = dict(case["kwargs"])
    if "th" in kw:
        kw["th"] = tuple(kw["th"])
    if "substruct_words" in kw:
        kw["substruct_words"] = _words(kw["substruct_words"])
    lb = oc.OracleLocalBlend(case["flavour"], case["prompts"], _words(case["words"]), tok, **kw)
    store = {key: [torch.from_numpy(LG[f"case{ci}_{key}_{i}"].astype(np.float32)) for i in range(n)]
             for key, n in (("down_cross", 4), ("up_cross", 3))}
    x = torch.from_numpy(LG[f"case{ci}_x_t"])
    for _ in range(case["calls"]):
        lb(x, store)
    want = lb.last_mask[:, 0].bool()
    maps = store["down_cross"][2:4] + store["up_cross"][:3]
    B = len(case["prompts"])
    sub = lb.sub.reshape(B, 77) if lb.sub is not None else None
    sums, _ = br.word_sums_ref(maps, maps[0].shape[0] // B, lb.alpha.reshape(B, 77), sub)
    th = (lb.threshold, 0.0) if case["flavour"] == "main" else lb.th
    got, dist = br.blend_mask_ref(sums, 16, th[0], th[1], (64, 64), sub is not None)
    assert got.shape == want.shape
    diff = got != want
    assert bool((dist[diff] < br.NEAR).all()), dist[diff]
    assert 0.0 < want.float().mean().item() < 1.0


def test_seed_table_is_the_search_rules():
    """Where an input's first seed breaks a condition the generator moves to the next one
    (blend_ref.search_seed); the table the GPU tests read is that search's result."""
    found = {}
    for R in br.RES:
        for key in br.input_keys(R):
            k = br.search_seed(key)
            if k:
                found[key] = k
    assert found == br.SEED_STEPS


@pytest.mark.parametrize("R", br.RES)
def test_grid_inputs_keep_the_near_cap_and_the_mask_fraction(R):
    """Every case of the GPU grid: the pixels whose deciding value lies within 1e-5 of a threshold
    are under 2 % of a prompt's latent pixels, and the mask covers 2 % .. 98 % of the pixels."""
    worst, n, paths = 0.0, 0, set()
    for key, sums, lat, (tp, ts) in br.mask_cases(R):
        mask, dist = br.blend_mask_ref(sums, R, tp, ts, lat, key[3])
        near = (dist < br.NEAR).flatten(1).float().mean(1).max().item()
        assert near < br.NEAR_CAP, (key, lat, near)
        assert br.FRAC[0] <= mask.float().mean().item() <= br.FRAC[1], (key, lat, mask.float().mean().item())
        worst = max(worst, near)
        paths.add(br.fast_path(R, lat))
        n += 1
    assert paths == {False, True}
    assert n == len(br.LHS) * len(br.BATCHES) * 2 * 7 * len(br.THRESHOLDS)
    print(f"R = {R}: {n} cases, largest near share {worst:.4%}")


@pytest.mark.parametrize("R", sorted(br.DEGENERATE_LATENTS))
def test_degenerate_inputs_keep_the_near_cap(R):
    """The degenerate-plane cases are exempt from the mask fraction, not from the near cap; and the
    reference gives them the masks torch's 0/0 = NaN implies."""
    for name, sums, sub in br.degenerate_cases(R):
        for lat in br.DEGENERATE_LATENTS[R]:
            for tp, ts in br.THRESHOLDS:
                mask, dist = br.blend_mask_ref(sums, R, tp, ts, lat, sub)
                assert (dist < br.NEAR).flatten(1).float().mean(1).max().item() < br.NEAR_CAP, (name, lat)
                if name == "edit_alpha_zero":
                    assert torch.equal(mask[1], mask[0])
                elif name == "source_alpha_zero":
                    assert not mask[0].any() and mask[1:].any()
                elif name == "edit_constant":
                    assert mask[1].all()
                elif name == "source_constant":
                    assert mask.all()
                else:
                    assert mask.any() and not mask.all()


def test_negative_control_references_differ_firmly():
    """The deliberately wrong references of the GPU negative controls differ from the right one
    outside the near set, so a kernel that agrees with the right one must leave theirs."""
    for R, lat in br.NEGATIVE_CONTROLS:
        sums = br.case_sums((R, 40, 2, False))
        right, _ = br.blend_mask_ref(sums, R, 0.5, 0.45, lat, False)
        for kw in (dict(pool=False), dict(source_or=False)):
            wrong, dist = br.blend_mask_ref(sums, R, 0.5, 0.45, lat, False, **kw)
            assert bool(((right != wrong) & (dist >= br.NEAR)).any()), (R, kw)
        const = torch.full((2, 2, 40, R * R), 0.7)
        right, _ = br.blend_mask_ref(const, R, 1.0, 1.0, lat, False)
        wrong, _ = br.blend_mask_ref(const, R, 1.0, 1.0, lat, False, strict=False)
        assert not right.any() and wrong.all()
