"""LocalBlend restated in float64 torch for any map resolution, map count and latent size -- the
reference of tests/test_gpu_blend_geometry.py and tests/test_gpu_latent.py, checked on the CPU by
tests/test_blend_ref.py -- with the word-sum reference and the input generators those tests share.

Every input is drawn on the host from a seeded CPU generator (the GPU tests move it to the
device), so the CPU test sees exactly the inputs the GPU tests use.
"""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

NEAR = 1e-5          # a deciding value closer than this to its threshold may fall either way in f32
NEAR_CAP = 0.02      # ... and such pixels are under 2 % of a prompt's latent pixels in every case
FRAC = (0.02, 0.98)  # every case's reference mask covers a share of the pixels inside this range


# ------------------------------------------------------------------ the mask reference
def blend_mask_ref(sums, R, th_pool, th_sub, size, sub, pool=True, strict=True, source_or=True):
    """null_text.py:41-67 in float64 on word sums that are already taken (sums [B, 2, LH, R*R]:
    plane 0 the alpha words, plane 1 the substruct words): mean over the LH maps, 3x3 max-pool
    (alpha plane only), nearest resampling to ``size`` (F.interpolate itself), max-normalise,
    threshold, then mask[:1] + mask, and substruct: mask * ~(sub[:1] + sub).

    Returns the mask [B, H, W] (bool) and, per latent pixel, the distance of the deciding
    normalised values from their thresholds.  A plane of zeros normalises to 0/0 = NaN, which is
    not > th at any precision: it decides nothing and its distance counts as infinite.

    pool / strict / source_or switch off one step each (no max-pool; >= for >; no mask[:1] |):
    the deliberately wrong references of the negative controls."""
    def plane(i, pooled, th):
        m = sums[:, i].double().mean(1).reshape(-1, 1, R, R)
        if pooled:
            m = F.max_pool2d(m, (3, 3), (1, 1), padding=(1, 1))
        m = F.interpolate(m, size=tuple(size))
        m = (m / m.amax(dim=(2, 3), keepdim=True))[:, 0]
        return (m.gt(th) if strict else m.ge(th)), torch.nan_to_num((m - th).abs(), nan=float("inf"))

    mask, dist = plane(0, pool, th_pool)
    if source_or:
        mask = mask[:1] | mask
        dist = torch.minimum(dist, dist[:1])
    if sub:
        s, sd = plane(1, False, th_sub)
        mask = mask & ~(s[:1] | s)
        dist = torch.minimum(dist, torch.minimum(sd, sd[:1]))
    return mask, dist


def kernel_nearest_index(lat, R):
    """build_blend_mask's source index of every latent row / column: f32 arithmetic,
    min(floorf(Y * ((float)R / (float)lat)), R - 1)."""
    scale = np.float32(R) / np.float32(lat)
    idx = np.floor(np.arange(lat, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, R - 1)


def interpolate_nearest_index(lat, R):
    """The source index F.interpolate (nearest) reads for every output position."""
    src = torch.arange(R, dtype=torch.float32).reshape(1, 1, R, 1)
    return F.interpolate(src, size=(lat, 1))[0, 0, :, 0].long().numpy()


# ------------------------------------------------------------------ the word-sum reference
def word_sums_ref(maps, heads, alpha, sub):
    """blend_wordsum_kernel in float64: maps[l] [B * heads, R*R, W], alpha / sub [B, W] (sub None:
    plane 1 is zero).  Returns the sums [B, 2, L * heads, R*R] and, in the same shape, the sum of
    the absolute products sum_w |v_w a_w| that the rounding bound scales with."""
    B, W = alpha.shape
    weights = torch.stack([alpha.double(), sub.double() if sub is not None else torch.zeros(B, W, dtype=torch.float64)], 1)
    m = torch.stack([t.double().reshape(B, heads, -1, W) for t in maps], 1)        # [B, L, heads, R2, W]
    m = m.reshape(B, len(maps) * heads, -1, W)
    return torch.einsum("bjpw,bsw->bsjp", m, weights), torch.einsum("bjpw,bsw->bsjp", m.abs(), weights.abs())


# ------------------------------------------------------------------ input generators
def smooth_sums(B, LH, R, sub, seed):
    """Smooth-ish positive word sums [B, 2, LH, R*R] f32, so the pooled maps cross the thresholds
    in many places: one spatial field per (prompt, plane), rand(4x4)**3 taken bilinearly to RxR,
    shared by the prompt's LH maps, times per-map noise 0.8 + 0.4 rand (the mean over the maps
    keeps the field's structure).  Without substruct plane 1 is zero."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B * 2, 1, 4, 4, generator=g) ** 3
    field = F.interpolate(base, size=(R, R), mode="bilinear", align_corners=False)
    sums = field.reshape(B, 2, 1, R * R) * (0.8 + 0.4 * torch.rand(B, 2, LH, R * R, generator=g))
    sums = sums.contiguous()
    if not sub:
        sums[:, 1] = 0
    return sums


def word_inputs(B, heads, n_maps, R, W, sub, seed):
    """Non-negative random maps [n_maps][B * heads, R*R, W] and word weights in (0, 1.5) that are
    not just 0 or 1 (alpha [B, W]; sub [B, W] or None), f32."""
    g = torch.Generator().manual_seed(seed)
    maps = [torch.rand(B * heads, R * R, W, generator=g) for _ in range(n_maps)]
    alpha = 1.5 * torch.rand(B, W, generator=g)
    subw = 1.5 * torch.rand(B, W, generator=g) if sub else None
    return maps, alpha, subw


# ------------------------------------------------------------------ the geometry grid
RES = (16, 15, 10, 8, 5)             # 15, 5: scalar loads; 10: 100 pixels, 25 live lanes; 8: 64 pixels
LHS = (1, 40, 48, 49, 100)           # below, at, one over and two over a batch of 48 buffer loads
BATCHES = (1, 2, 16)
THRESHOLDS = ((0.3, 0.3), (0.5, 0.45))


def latents(R):
    return ((64, 64), (R, R), (24, 40), (96, 32), (12, 12), (8, 20), (R - 1, 64))


def fast_path(R, lat):
    """build_blend_mask's branch: the latent samples every map pixel."""
    return lat[0] >= R and lat[1] >= R


def input_keys(R):
    """The inputs of one resolution's cases: (R, LH, B, sub)."""
    return [(R, LH, B, sub) for LH in LHS for B in BATCHES for sub in (False, True)]


def base_seed(key):
    R, LH, B, sub = key
    return ((R * 1000 + LH) * 100 + B) * 2 + int(sub)


def input_ok(sums, R, sub):
    """The two conditions on a drawn input, over every latent and threshold pair it is used with:
    the near set of every prompt is under NEAR_CAP of its latent pixels, and the mask's share of
    the pixels lies in FRAC.  Returns (ok, largest near share, mask share range)."""
    worst, lo, hi = 0.0, 1.0, 0.0
    for lat, (tp, ts) in itertools.product(latents(R), THRESHOLDS):
        mask, dist = blend_mask_ref(sums, R, tp, ts, lat, sub)
        worst = max(worst, (dist < NEAR).flatten(1).float().mean(1).max().item())
        f = mask.float().mean().item()
        lo, hi = min(lo, f), max(hi, f)
    return worst < NEAR_CAP and FRAC[0] <= lo and hi <= FRAC[1], worst, (lo, hi)


def search_seed(key):
    """The fixed rule: the first seed base_seed(key) + k, k = 0, 1, ..., whose input passes
    input_ok.  Returns k."""
    R, LH, B, sub = key
    for k in range(64):
        if input_ok(smooth_sums(B, LH, R, sub, base_seed(key) + k), R, sub)[0]:
            return k
    raise AssertionError(f"no seed for {key}")


# k of search_seed for the inputs whose first seed breaks a condition (every other key: 0).
# tests/test_blend_ref.py recomputes the search and pins this table.
SEED_STEPS = {
    (16, 48, 2, True): 1, (8, 1, 2, True): 1, (8, 1, 16, True): 1, (8, 40, 16, False): 1, (8, 48, 1, False): 1,
    (5, 1, 16, False): 2, (5, 40, 1, False): 5, (5, 40, 2, False): 3, (5, 40, 16, False): 9, (5, 48, 1, False): 1,
    (5, 48, 2, False): 1, (5, 48, 16, False): 6, (5, 49, 2, False): 1, (5, 49, 16, False): 2, (5, 100, 2, False): 1,
}


@functools.lru_cache(maxsize=None)
def case_sums(key):
    R, LH, B, sub = key
    return smooth_sums(B, LH, R, sub, base_seed(key) + SEED_STEPS.get(key, 0))


def mask_cases(R):
    """Every (key, sums, latent, (th_pool, th_sub)) of one resolution."""
    for key in input_keys(R):
        for lat, th in itertools.product(latents(R), THRESHOLDS):
            yield key, case_sums(key), lat, th


# ------------------------------------------------------------------ degenerate planes
DEGENERATE_LATENTS = {16: ((64, 64), (12, 12)), 10: ((64, 64), (8, 20))}    # fast and generic path each
DEGENERATE_SEED = {16: 7016, 10: 7010}


def degenerate_cases(R):
    """(name, sums [3, 2, 40, R*R], substruct on) with one plane made degenerate: all zero (torch
    normalises it to 0/0 = NaN, which is not > th) or constant (it normalises to 1 everywhere)."""
    def make(sub, b, plane, value):
        sums = smooth_sums(3, 40, R, sub, DEGENERATE_SEED[R] + int(sub))
        sums[b, plane] = value
        return sums

    return [("edit_alpha_zero", make(False, 1, 0, 0.0), False), ("source_alpha_zero", make(False, 0, 0, 0.0), False),
            ("edit_constant", make(False, 1, 0, 0.7), False), ("source_constant", make(False, 0, 0, 0.7), False),
            ("edit_sub_zero", make(True, 1, 1, 0.0), True), ("source_sub_zero", make(True, 0, 1, 0.0), True)]


# the negative controls' geometries: the product's (fast path) and a down-sampling one (generic path)
NEGATIVE_CONTROLS = ((16, (64, 64)), (10, (8, 20)))
