"""p2p_mutual_attn_fwd and p2p_token_classes vs the float64 torch lines of tests/mutual_ref.py (GPU).

Bounds are the project's own: o_tol of tests/test_gpu_kernels.py (2^-7 max|V| on the 16-bit pipe,
1e-5 max|V| in the f32 check mode) and, for fp16 inputs, the bound tests/test_gpu_f16.py holds
p2p_self_attn_fwd to (o_tol plus one f16 output ulp of the largest value)."""
import pytest
import torch

import attn_layouts as al
from mutual_ref import mutual_ref, token_classes_ref
from p2p_amd import _hip
from test_gpu_kernels import make_qkv, o_tol

pytestmark = pytest.mark.gpu

GEOMS = [(4, 100, 2, 40), (4, 256, 2, 80), (4, 320, 2, 160), (4, 192, 2, 16), (3, 33, 2, 8), (4, 2048, 1, 40)]
MODES = [("f32", torch.float32), ("bf16", torch.float32)]          # check mode; the 16-bit pipe (split-bf16)
CASES = [pytest.param(g, c, dt, id="x".join(map(str, g)) + f"-{c}-{str(dt)[6:]}") for g in GEOMS for c, dt in MODES]
CASES += [pytest.param(g, "bf16", dt, id="x".join(map(str, g)) + f"-bf16-{str(dt)[6:]}")
          for g in GEOMS[:3] for dt in (torch.bfloat16, torch.float16)]
PATTERNS = ("none", "alternating", "first128", "first133", "source_one_class", "queries_one_class", "random")


def kv_source(N):
    return [0, 0, 2, 2] if N == 4 else [0] * N


def classes(pattern, N, P, kv_src, dev):
    """uint8 [N, P] (None for "none"): the rows of the sources hold the key classes."""
    if pattern == "none":
        return None
    g = torch.Generator(device="cpu").manual_seed(7)
    tc = torch.zeros(N, P, dtype=torch.uint8)
    sources = sorted({s for n, s in enumerate(kv_src) if s >= 0})
    edits = [n for n, s in enumerate(kv_src) if s != n]
    if pattern == "alternating":
        tc[:] = (torch.arange(P) % 2).to(torch.uint8)
    elif pattern in ("first128", "first133"):
        # source keys 0 .. n1 - 1 are class 1 and every query class 0: the first key tiles hold no
        # admitted key (first133: the admitted keys start inside a tile)
        n1 = (128 if pattern == "first128" else 133) if P > 133 else P // 2 + 3
        tc[sources, :n1] = 1
        tc[edits] = 0
    elif pattern == "source_one_class":
        tc[sources] = 1
        tc[edits] = (torch.rand(len(edits), P, generator=g) < 0.5).to(torch.uint8)
    elif pattern == "queries_one_class":
        tc[sources] = (torch.rand(len(sources), P, generator=g) < 0.5).to(torch.uint8)
        tc[edits] = 1
    else:
        tc[:] = (torch.rand(N, P, generator=g) < 0.3).to(torch.uint8)
    return tc.to(dev)


def bound(v, want, compute, dtype):
    if dtype == torch.float16:
        return o_tol(v, "bf16") + 2.0 ** -10 * want.abs().max().item()     # tests/test_gpu_f16.py
    return o_tol(v, compute)


def run(q, k, v, H, scale, kv_src, tc, compute, o=None):
    o = torch.empty_like(q) if o is None else o
    assert _hip.mutual_attn(q, k, v, o, H, scale, kv_src, token_class=tc, compute=compute) is o
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("geom,compute,dtype", CASES)
def test_mutual_attention(cuda, geom, compute, dtype):
    N, P, H, d = geom
    q, k, v = make_qkv(N, P, P, H, d, dtype)
    scale = d ** -0.5
    kv_src = kv_source(N)
    plain = mutual_ref(q, k, v, H, scale)                 # every entry on its own keys
    unmasked = mutual_ref(q, k, v, H, scale, kv_src)
    for pattern in PATTERNS:
        tc = classes(pattern, N, P, kv_src, cuda)
        want = unmasked if tc is None else mutual_ref(q, k, v, H, scale, kv_src, tc)
        o = run(q, k, v, H, scale, kv_src, tc, compute)
        assert torch.isfinite(o).all(), pattern
        tol = bound(v, want, compute, dtype)
        err = (o.double() - want).abs().max().item()
        print(f"{pattern}: max |O - ref| = {err:.3e} (bound {tol:.3e})")
        assert err < tol, (pattern, err, tol)
        # entries that read their own keys are plain attention, classes or not
        own = [n for n, s in enumerate(kv_src) if s == n]
        assert (o[own].double() - plain[own]).abs().max().item() < tol, pattern
        if pattern == "source_one_class":
            # a query of the class the source lacks reads every key: unrestricted attention
            lacking = (tc == 0)
            lacking[own] = False
            assert lacking.any()
            assert (o.double() - unmasked)[lacking].abs().max().item() < tol


def test_skipped_entries_keep_their_bits(cuda):
    N, P, H, d = 4, 100, 2, 40
    q, k, v = make_qkv(N, P, P, H, d, torch.bfloat16)
    kv_src = [-1, 0, -1, 2]
    tc = classes("random", N, P, kv_src, cuda)
    o = torch.full((N, P, H * d), al.SENTINEL[2], dtype=torch.int16, device=cuda).view(torch.bfloat16)
    run(q, k, v, H, d ** -0.5, kv_src, tc, "bf16", o=o)
    bits = o.view(torch.int16)
    assert (bits[[0, 2]] == al.SENTINEL[2]).all()
    assert (bits[[1, 3]] != al.SENTINEL[2]).any(-1).all()          # every row of the others was written
    want = mutual_ref(q, k, v, H, d ** -0.5, kv_src, tc)
    assert (o[[1, 3]].double() - want[[1, 3]]).abs().max().item() < o_tol(v, "bf16")
    # all entries skipped: nothing runs
    o2 = o.clone()
    run(q, k, v, H, d ** -0.5, [-1] * N, tc, "bf16", o=o2)
    assert al.same_bits(o2, o)


@pytest.mark.parametrize("compute,dtype", [("f32", torch.float32), ("bf16", torch.float32), ("bf16", torch.bfloat16),
                                           ("bf16", torch.float16)])
def test_peaky_logits_stay_finite(cuda, compute, dtype):
    """q scaled by 16, no admitted key in the first key tiles of the edit rows: nothing non-finite."""
    N, P, H, d = 4, 256, 2, 80
    q, k, v = make_qkv(N, P, P, H, d, dtype, qscale=16.0)
    kv_src = kv_source(N)
    for pattern in ("first128", "first133"):
        tc = classes(pattern, N, P, kv_src, cuda)
        o = run(q, k, v, H, d ** -0.5, kv_src, tc, compute)
        assert torch.isfinite(o).all()
        want = mutual_ref(q, k, v, H, d ** -0.5, kv_src, tc)
        err = (o.double() - want).abs().max().item()
        print(f"{pattern}: max |O - ref| = {err:.3e}")


@pytest.mark.parametrize("layout", ["fused_self", "skewed"])
def test_layouts_bit_identical_to_dense(cuda, layout):
    """The fused-projection and the NaN-padded operand layouts of tests/attn_layouts.py: the same
    bits as the dense launch, nothing written outside O's view."""
    N, P, H, d = 4, 100, 2, 40
    kv_src = kv_source(N)
    tc = classes("random", N, P, kv_src, cuda)
    outs = {}
    for lay in ("dense", layout):
        ops = al.build(N, P, P, H, d, torch.bfloat16, 3, lay, dev="cuda")
        run(ops.q, ops.k, ops.v, H, d ** -0.5, kv_src, tc, "bf16", o=ops.o)
        al.check_output(ops)
        outs[lay] = ops.o.contiguous()
    assert torch.isfinite(outs[layout]).all()
    assert al.same_bits(outs["dense"], outs[layout])


def test_broadcast_kv_batch_stride_zero(cuda):
    """k and v with batch stride 0: every entry reads entry 0's rows whatever kv_src names."""
    N, P, H, d = 4, 100, 2, 40
    ops = al.build(N, P, P, H, d, torch.bfloat16, 3, "broadcast_kv", dev="cuda")
    kv_src = kv_source(N)
    run(ops.q, ops.k, ops.v, H, d ** -0.5, kv_src, None, "bf16", o=ops.o)
    al.check_output(ops)
    want = mutual_ref(ops.dense["q"], ops.dense["k"], ops.dense["v"], H, d ** -0.5, [0] * N)
    assert (ops.o.double() - want).abs().max().item() < o_tol(ops.dense["v"], "bf16")


# ------------------------------------------------------------------------------ token classes
def word_sums(B, lh, res, dev, constant_row=None):
    """[B, 2, lh, res^2] f32 whose normalised means lie on the grid i / 16: map l of plane 0 holds
    level * (l + 1), so the mean is level * (lh + 1) / 2 and the min-max normalisation level / 16."""
    g = torch.Generator(device="cpu").manual_seed(11)
    level = torch.randint(0, 17, (B, res * res), generator=g).float()
    level[:, 0], level[:, 1] = 0, 16                         # both ends of the grid occur
    if constant_row is not None:
        level[constant_row] = 5
    sums = torch.empty(B, 2, lh, res * res)
    sums[:, 0] = level[:, None, :] * torch.arange(1, lh + 1).float()[None, :, None]
    sums[:, 1] = torch.randn(B, lh, res * res, generator=g) * 100         # plane 1 is not read
    return sums.to(dev)


@pytest.mark.parametrize("threshold", [0.1, 0.5 + 1 / 32])
@pytest.mark.parametrize("groups,cfg", [(1, True), (2, True), (1, False)])
def test_token_classes(cuda, threshold, groups, cfg):
    B, lh, res, sides = 3, 10, 16, (16, 32, 64)
    sums = [word_sums(B, lh, res, cuda, constant_row=1 if g == 0 else None) for g in range(groups)]
    # the grid keeps away from the threshold: no class depends on a rounding
    for s in sums:
        m = s[:, 0].double().cpu().mean(1)
        rng = (m.max(1, keepdim=True).values - m.min(1, keepdim=True).values)
        norm = ((m - m.min(1, keepdim=True).values) / rng)[(rng > 0).flatten()]
        assert (norm - threshold).abs().min().item() >= 1e-3
    rows = groups * B * (2 if cfg else 1)
    outs = [torch.full((rows, s * s), 7, dtype=torch.uint8, device=cuda) for s in sides]
    assert _hip.token_classes(sums, B, lh, res, threshold, sides, outs, cfg=cfg) is not None
    torch.cuda.synchronize()
    want = token_classes_ref(sums, threshold, sides, cfg=cfg)
    for side, o, w in zip(sides, outs, want):
        assert torch.equal(o, w), side
        if cfg:
            assert torch.equal(o[:rows // 2], o[rows // 2:])          # uncond rows copy the cond rows
    assert (outs[0][(B * groups if cfg else 0) + 1] == 0).all()       # the constant map: class 0
    assert outs[0].sum() > 0
