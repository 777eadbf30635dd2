"""The attention kernels on strided, padded and skewed operands (GPU).

The product reads every U-Net attention operand through strides (ptp_utils._project: q, k, v are
column slices of one [N, P, 3C] projection, or k, v of a cached [N, K, 2C] one); the other kernel
tests launch contiguous tensors, where ldq == ldk == ldv == ldo and mostly bsq == bsk == bsv == bso,
so a kernel that took one stride for another would pass them.  Here every production row of
csrc/p2p_select.h (all but the experiments build's STAMPS rows and SELF_WIDE, which has its own
strided test) runs at the smallest shape that selects it, asserted by name, under each layout of
tests/attn_layouts.py that applies:

1. the dense launch against the f32 torch reference, at the bound the kernel's own test uses (O:
   o_tol plus one output ulp for 16-bit outputs; kept probabilities PROB_TOL; word sums WORD_SUM_TOL,
   all from test_gpu_kernels.py);
2. every other layout: the same bound against the same reference, and bit-identical to the dense
   launch (the kernels reduce in a fixed order; strides change addresses only);
3. nothing outside o's view written, everything inside it written (the o buffer is pre-filled with a
   sentinel), the unused slot groups and the guard words around the kept maps, the materialised
   probabilities and the word sums intact.  Input padding is NaN: a kernel that folds a padding
   element into a sum, even times a zero probability, fails 1. or 2.

Each case prints its worst error over bound.  test_wrong_view_is_seen passes V's view built with
K's row stride and must FAIL the comparison: the data does tell the strides apart
(tests/test_attn_layouts.py proves the same for every case here, on the CPU).
"""
import pytest
import torch

from p2p_amd import _hip

import attn_layouts as al
from test_gpu_kernels import PROB_TOL, WORD_SUM_TOL, _edit_mapper, o_tol, ref_out, ref_probs

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
OUT_ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -10, F32: 0.0}   # one rounding of the stored output (test_gpu_f16.o_bar)


def o_bound(v, want, compute, dtype):
    return o_tol(v, compute) + OUT_ULP[dtype] * want.abs().max().item()


def fused(bk, waves, form=""):
    return "self_attn_fused_kernel<…,D,%d,%d%s>" % (bk, waves, "," + form if form else "")


class Case:
    """kind: self (O only) | maps (kept maps) | pv (materialise protocol) | cross.  cross cases: n_pg
    prompt groups of B = 2 entries, batch [uncond groups | cond groups]; edit: None | "dense" |
    "terms" (the cond groups' Replace program); store: the cond maps kept, word sums folded in."""

    def __init__(self, id, kernel, kind, N, P, K, H, d, dtype, compute="bf16", seed=0, qscale=1.0, mask=False,
                 n_pg=1, edit=None, store=False):
        self.id, self.kernel, self.kind = id, kernel, kind
        self.N, self.P, self.K, self.H, self.d = N, P, K, H, d
        self.dtype, self.compute, self.seed, self.qscale, self.mask = dtype, compute, seed, qscale, mask
        self.n_pg, self.edit, self.store = n_pg, edit, store
        self.cross = kind in ("pv", "cross")      # k, v come from the context projection
        self.scale = d ** -0.5

    def build(self, layout, dev="cpu", **kw):
        return al.build(self.N, self.P, self.K, self.H, self.d, self.dtype, self.seed, layout, qscale=self.qscale,
                        dev=dev, **kw)

    def layouts(self):
        """The layouts compared with the plain dense launch (broadcast_kv has its own baseline)."""
        return [x for x in al.LAYOUTS if x not in ("dense", "broadcast_kv") and al.applies(x, self.P, self.K, self.cross)]


def _self(id, kernel, P, K, d, dtype, compute="bf16", seed=51):
    return Case(id, kernel, "self", 2, P, K, 2, d, dtype, compute, seed)


SELF_CASES = [
    # p2p_self40.hip: d = 40 from P = 2048, d = 80 from P = 512, both from K = 256; ragged last tiles
    _self("self40_d40", "self40_kernel<40,8,2,256>", 2100, 2100, 40, BF16),
    _self("self40_d40_h16", "self40_kernel<40,8,2,256,H16>", 2100, 300, 40, F16),
    _self("self40_d80", "self40_kernel<80,8,1,128>", 600, 600, 80, BF16),
    _self("self40_d80_h16", "self40_kernel<80,8,1,128,H16>", 600, 300, 80, F16),
    # p2p_selfmulti.hip: d = 40, P >= 2048, what self40_kernel leaves (K < 256; f32 inputs)
    _self("multi_f16", "self_attn_multi_kernel<…,40,256,8,2,F16,PIPE>", 2100, 200, 40, BF16),
    _self("multi_128", "self_attn_multi_kernel<…,40,128,8,2>", 2100, 2100, 40, F32),
    # p2p_selfsplit.hip: d = 160, bf16, by K
    _self("split_1x1", "self_split_kernel<160,1,1>", 70, 20, 160, BF16),
    _self("split_2x1", "self_split_kernel<160,2,1>", 50, 50, 160, BF16),
    _self("split_2x2", "self_split_kernel<160,2,2>", 70, 100, 160, BF16),
    _self("halves", "self_halves_kernel", 200, 200, 160, BF16),
    _self("ring", "self_ring_kernel<160,4>", 300, 300, 160, BF16),
    # p2p_self.hip, every tile shape and form: 32-key tiles for the f32 P V, else 64; 2 waves up to
    # P = 64, above it 8 at d = 40 / 80 and 4 otherwise; NOMAX with a ones column (d % 32 != 0) and
    # bf16 P
    _self("fused_32x2", fused(32, 2), 50, 50, 40, F32, "f32"),
    _self("fused_32x4", fused(32, 4), 100, 77, 40, F32, "f32"),
    _self("fused_64x2", fused(64, 2), 50, 50, 64, BF16),
    _self("fused_64x4", fused(64, 4), 100, 100, 64, BF16),
    _self("fused_64x8_f16", fused(64, 8), 100, 77, 40, F16),
    _self("fused_64x2_nomax", fused(64, 2, "NOMAX"), 50, 50, 40, BF16),
    _self("fused_64x4_nomax", fused(64, 4, "NOMAX"), 100, 77, 16, BF16),
    _self("fused_64x8_nomax", fused(64, 8, "NOMAX"), 100, 100, 40, BF16),
]


def _maps(id, kernel, P, K, d, dtype, compute="bf16"):
    return Case(id, kernel, "maps", 3, P, K, 2, d, dtype, compute, seed=53, qscale=4.0)


MAPS_CASES = [   # the EXACT forms and the p2p_selfmaps.hip recompute
    _maps("maps_32x2", fused(32, 2, "EXACT"), 50, 50, 40, F32, "f32"),
    _maps("maps_32x4", fused(32, 4, "EXACT"), 100, 77, 40, F32, "f32"),
    _maps("maps_64x2", fused(64, 2, "EXACT"), 50, 50, 64, BF16),
    _maps("maps_64x4", fused(64, 4, "EXACT"), 100, 100, 64, BF16),
    _maps("maps_64x8", fused(64, 8, "EXACT"), 100, 77, 40, BF16),
]

PV_CASES = [     # p2p_attn_probs + p2p_attn_pv; the library has no name query for the P V mode: the
                 # rows are select_self's for MODE_PV_ (tests/test_attn_layouts.py asks p2p_select.h)
    Case("pv_32x4", "self_pv_kernel<…,D,32,4>", "pv", 2, 50, 77, 2, 40, F32, "f32", seed=55, qscale=4.0),
    Case("pv_64x4", "self_pv_kernel<…,D,64,4>", "pv", 2, 50, 77, 2, 64, BF16, seed=55, qscale=4.0),
    Case("pv_mask", "self_pv_kernel<…,D,32,4>", "pv", 3, 40, 77, 2, 16, F32, "f32", seed=55, mask=True),
]


def _cross(id, kernel, P, K, H, d, dtype, compute="bf16", n_pg=1, edit=None, store=False):
    return Case(id, kernel, "cross", 4 * n_pg, P, K, H, d, dtype, compute, seed=57, qscale=6.0, n_pg=n_pg, edit=edit,
                store=store)


def _group_cases(K):
    # the group kernel needs launch groups x heads x ceil(P / 128) >= 512: 8 groups of 2 entries, 8
    # heads, P = 1000 (8 query tiles, the last one ragged)
    return [_cross(f"group{form.replace(',', '_').lower()}_k{K}", f"cross_group_kernel<D,4{form}>", 1000, K, 8, 40, BF16,
                   n_pg=4, edit=edit, store=store)
            for form, edit, store in (("", None, False), (",STORE", None, True), (",EDIT", "dense", False),
                                      (",EDIT,STORE", "dense", True))]


CROSS_CASES = [
    _cross("entry_w2", "cross_attn_kernel<…,D,2>", 70, 77, 2, 160, F32, "f32", store=True),
    _cross("entry_w4_f32", "cross_attn_kernel<…,D,4>", 100, 77, 2, 40, F32, "f32", edit="dense", store=True),
    _cross("entry_w4_terms", "cross_attn_kernel<…,D,4>", 100, 77, 2, 40, BF16, edit="terms", store=True),
    _cross("entry_dense", "cross_attn_kernel<…,D,4,DENSE>", 100, 77, 2, 80, BF16, edit="dense", store=True),
    _cross("entry_dense_p300", "cross_attn_kernel<…,D,4,DENSE>", 300, 77, 2, 80, BF16, edit="dense"),   # LDS-staged O
] + _group_cases(77) + _group_cases(96)      # K = 96: no short key tail

ALL_CASES = SELF_CASES + MAPS_CASES + PV_CASES + CROSS_CASES

# Every production row of P2P_SELF_KERNELS (no STAMPS rows, no SELF_WIDE) and of P2P_CROSS_KERNELS,
# written out: a new table row fails test_cases_cover_the_selection_table here and, against the
# header itself, tests/test_attn_layouts.py.
EXPECTED_KERNELS = [
    "self_attn_fused_kernel<…,D,32,2>", "self_attn_fused_kernel<…,D,32,2,EXACT>",
    "self_attn_fused_kernel<…,D,32,4>", "self_attn_fused_kernel<…,D,32,4,EXACT>",
    "self_attn_fused_kernel<…,D,64,2>", "self_attn_fused_kernel<…,D,64,2,EXACT>", "self_attn_fused_kernel<…,D,64,2,NOMAX>",
    "self_attn_fused_kernel<…,D,64,4>", "self_attn_fused_kernel<…,D,64,4,EXACT>", "self_attn_fused_kernel<…,D,64,4,NOMAX>",
    "self_attn_fused_kernel<…,D,64,8>", "self_attn_fused_kernel<…,D,64,8,EXACT>", "self_attn_fused_kernel<…,D,64,8,NOMAX>",
    "self_pv_kernel<…,D,32,4>", "self_pv_kernel<…,D,64,4>",
    "self_attn_multi_kernel<…,40,256,8,2,F16,PIPE>", "self_attn_multi_kernel<…,40,128,8,2>",
    "self40_kernel<40,8,2,256>", "self40_kernel<40,8,2,256,H16>", "self40_kernel<80,8,1,128>", "self40_kernel<80,8,1,128,H16>",
    "self_split_kernel<160,1,1>", "self_split_kernel<160,2,1>", "self_split_kernel<160,2,2>",
    "self_halves_kernel", "self_ring_kernel<160,4>",
    "cross_group_kernel<D,4>", "cross_group_kernel<D,4,STORE>", "cross_group_kernel<D,4,EDIT>",
    "cross_group_kernel<D,4,EDIT,STORE>",
    "cross_attn_kernel<…,D,2>", "cross_attn_kernel<…,D,4>", "cross_attn_kernel<…,D,4,DENSE>",
]

GUARD = 256   # sentinel floats before and after the kept maps / probabilities / word sums


def test_cases_cover_the_selection_table():
    assert len(set(EXPECTED_KERNELS)) == len(EXPECTED_KERNELS) == 33
    assert {c.kernel for c in ALL_CASES} == set(EXPECTED_KERNELS)
    assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        assert c.N >= 2 and c.H >= 2, c.id


# ---------------------------------------------------------------------------- the launches
def launch_self(c, ops):
    t = _hip.make_tensors(ops.q, ops.k, ops.v, ops.o, c.H, c.scale, c.compute)
    assert _hip.self_attn_kernel(t) == c.kernel, (ops.layout, _hip.self_attn_kernel(t))
    _hip.self_attn(ops.q, ops.k, ops.v, ops.o, c.H, c.scale, compute=c.compute)
    return {"o": ops.o.contiguous()}, []


def reference_self(c, dense, base):
    p = ref_probs(dense["q"], dense["k"], c.H, c.scale)
    want = ref_out(p, dense["v"], c.H)
    return {"o": (want, o_bound(dense["v"], want, c.compute, c.dtype))}


MAPS_SRC = [0, 0, 2]     # entry 1 reads entry 0's probabilities (the self-attention injection)


def launch_maps(c, ops):
    """Entries 0 and 2 keep their maps, entry 1 does not; the store has one unused slot group before
    the used ones and one after, holding 7.0, and guard words around it.  Two calls: the first
    overwrites, the second accumulates."""
    H, P, K = c.H, c.P, c.K
    t = _hip.make_tensors(ops.q, ops.k, ops.v, ops.o, H, c.scale, c.compute)
    assert _hip.self_attn_kernel(t, keeps_maps=True) == c.kernel, (ops.layout, _hip.self_attn_kernel(t, keeps_maps=True))
    buf, used = al.guarded(4 * H * P * K, GUARD, ops.q.device, fill=7.0)
    store = used.view(4 * H, P, K)
    out, problems = {}, []
    for name, acc in (("maps", False), ("maps_accumulated", True)):
        _hip.self_attn(ops.q, ops.k, ops.v, ops.o, H, c.scale, compute=c.compute, qk_src=MAPS_SRC, store=store,
                       store_slot=[H, -1, 2 * H], accumulate=acc)
        out[name] = store[H:3 * H].clone()
    out["o"] = ops.o.contiguous()
    if not (store[:H] == 7.0).all() or not (store[3 * H:] == 7.0).all():
        problems.append("an unused slot group of the store was written")
    if not al.guards_intact(buf, 4 * H * P * K, GUARD):
        problems.append("written outside the store")
    return out, problems


def reference_maps(c, dense, base):
    p = ref_probs(dense["q"], dense["k"], c.H, c.scale, qk_src=MAPS_SRC)
    kept = torch.cat([p[0], p[2]])
    want = ref_out(p, dense["v"], c.H)
    tol = PROB_TOL[c.compute]
    return {"maps": (kept, tol), "maps_accumulated": (2 * kept, 2 * tol),
            "o": (want, o_bound(dense["v"], want, c.compute, c.dtype))}


def _key_mask(c, dev):
    mask = torch.ones(c.N, c.K, dtype=torch.bool, device=dev)
    mask[0, 50:] = False
    mask[1, :10] = False
    mask[2, :] = False
    return mask


def launch_pv(c, ops):
    H, P, K, N = c.H, c.P, c.K, c.N
    buf, used = al.guarded(N * H * P * K, GUARD, ops.q.device)
    probs = used.view(N * H, P, K)
    mask = _key_mask(c, ops.q.device).to(torch.uint8) if c.mask else None
    _hip.attn_probs(ops.q, ops.k, H, c.scale, probs, compute=c.compute, key_mask=mask)
    _hip.attn_pv(probs, ops.v, ops.o, H, compute=c.compute)
    problems = [] if al.guards_intact(buf, N * H * P * K, GUARD) else ["written outside the probabilities"]
    return {"probs": probs.clone(), "o": ops.o.contiguous()}, problems


def reference_pv(c, dense, base):
    N, P, K, H, d = c.N, c.P, c.K, c.H, c.d
    q, k, v = dense["q"], dense["k"], dense["v"]
    if c.mask:   # ptp_utils.py:197-201: row (n*H + h) takes mask row (n*H + h) % N
        sim = torch.einsum("nhid,nhjd->nhij", q.float().reshape(N, P, H, d).permute(0, 2, 1, 3),
                           k.float().reshape(N, K, H, d).permute(0, 2, 1, 3)).reshape(N * H, P, K) * c.scale
        sim.masked_fill_(~_key_mask(c, q.device)[:, None, :].repeat(H, 1, 1), -torch.finfo(sim.dtype).max)
        p = sim.softmax(-1)
    else:
        p = ref_probs(q, k, H, c.scale).reshape(N * H, P, K)
    # the second half is checked as test_probs_and_pv_materialise does: P V of the probabilities the
    # first half produced (the dense launch's: the other layouts' must be the same bits)
    want = ref_out(base["probs"].reshape(N, H, P, K), v, H)
    return {"probs": (p, PROB_TOL[c.compute]), "o": (want, o_bound(v, want, c.compute, c.dtype))}


B = 2            # entries per prompt group of the cross cases: the source and one edit


def _cross_program(c, dev):
    """(mapper [1, K, K], device program, alpha [1, K]) of the cond groups, or Nones."""
    if c.edit is None:
        return None, None, None
    from p2p_amd import programs
    mapper = _edit_mapper(B, c.K, 0.5 if c.edit == "dense" else 1.0 / 3.0)
    if c.edit == "terms":
        mapper[0, 5, 3] = 1.0 / 3.0
    host = programs.replace_program(mapper)
    assert (host.dense_f16() is not None) == (c.edit == "dense")
    alpha = torch.ones(B - 1, c.K, device=dev)
    alpha[0, 10:20] = 0.0                       # both halves of the blend
    return mapper.to(dev), host.to_device(dev), alpha


def _blend_rows(c, dev):
    balpha = torch.rand(B, c.K, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    bsub = torch.rand(B, c.K, device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    return balpha, bsub


def cross_groups(c, dev):
    """The launch's group tuples: [uncond groups | cond groups] of B entries; with c.store the cond
    entries keep their maps and fold LocalBlend's word sums in (columns 2H .. 3H of 5H; the substruct
    row for group 0 only), as test_cross_group_kernel_bf16 does.  Returns (groups, store buffer,
    store, slots, [(word-sum buffer, used part)])."""
    H, P, K = c.H, c.P, c.K
    BG, lh = B * c.n_pg, 5 * c.H
    _, prog, alpha = _cross_program(c, dev)
    balpha, bsub = _blend_rows(c, dev)
    groups = [(g * B, B, None, None) for g in range(c.n_pg)]
    sums_bufs, store_buf, store, slots = [], None, None, None
    if c.store:
        store_buf, used = al.guarded(BG * H * P * K, GUARD, dev)
        store = used.view(BG * H, P, K)
        slots = [-1] * BG + [i * H for i in range(BG)]
        sums_bufs = [al.guarded(B * 2 * lh * P, GUARD, dev) for _ in range(c.n_pg)]
    for g in range(c.n_pg):
        blend = (sums_bufs[g][1].view(B, 2, lh, P), balpha, bsub if g == 0 else None, 2 * H, lh) if c.store else None
        groups.append((BG + g * B, B, prog, alpha, blend))
    return groups, store_buf, store, slots, sums_bufs


def cross_kernel_name(c, ops, groups):
    t = _hip.make_tensors(ops.q, ops.k, ops.v, ops.o, c.H, c.scale, c.compute)
    return _hip.cross_attn_kernel(t, _hip._group_array(t, groups), c.store)


def launch_cross(c, ops):
    """With c.store two calls: the first overwrites the maps and word sums, the second accumulates."""
    H, P, K = c.H, c.P, c.K
    BG, lh = B * c.n_pg, 5 * c.H
    groups, store_buf, store, slots, sums_bufs = cross_groups(c, ops.q.device)
    name = cross_kernel_name(c, ops, groups)
    assert name == c.kernel, (ops.layout, name)
    for acc in ((False, True) if c.store else (False,)):
        _hip.cross_attn(ops.q, ops.k, ops.v, ops.o, H, c.scale, groups, compute=c.compute, store=store, store_slot=slots,
                        accumulate=acc)
    out, problems = {"o": ops.o.contiguous()}, []
    if c.store:
        out["maps_accumulated"] = store.clone()
        out["word_sums"] = torch.stack([used.view(B, 2, lh, P) for _, used in sums_bufs])
        if not al.guards_intact(store_buf, BG * H * P * K, GUARD):
            problems.append("written outside the store")
        if not all(al.guards_intact(buf, B * 2 * lh * P, GUARD) for buf, _ in sums_bufs):
            problems.append("written outside the word sums")
        s = out["word_sums"]
        if s[:, :, :, :2 * H].abs().max().item() != 0.0 or s[:, :, :, 3 * H:].abs().max().item() != 0.0:
            problems.append("another layer's word-sum columns were written")
    return out, problems


def reference_cross(c, dense, base):
    H, dev = c.H, dense["q"].device
    BG = B * c.n_pg
    mapper, _, alpha = _cross_program(c, dev)
    p = ref_probs(dense["q"], dense["k"], H, c.scale)               # [N, H, P, K]
    want = p.clone()
    if c.edit is not None:
        a = alpha[:, None, None, :]
        for g in range(c.n_pg):
            s0 = BG + g * B
            R = torch.einsum("hpw,bwn->bhpn", p[s0], mapper)
            want[s0 + 1:s0 + B] = R * a + (1 - a) * p[s0 + 1:s0 + B]
    o = ref_out(want, dense["v"], H)
    refs = {"o": (o, o_bound(dense["v"], o, c.compute, c.dtype))}
    if c.store:
        cond = want[BG:]
        refs["maps_accumulated"] = (2 * cond.reshape(BG * H, c.P, c.K), 2 * PROB_TOL[c.compute])
        balpha, bsub = _blend_rows(c, dev)
        sums = torch.zeros(c.n_pg, B, 2, 5 * H, c.P, device=dev)
        for g in range(c.n_pg):
            cg = cond[g * B:(g + 1) * B]                             # [B, H, P, K]
            sums[g, :, 0, 2 * H:3 * H] = 2 * torch.einsum("bhpk,bk->bhp", cg, balpha)
            if g == 0:
                sums[g, :, 1, 2 * H:3 * H] = 2 * torch.einsum("bhpk,bk->bhp", cg, bsub)
        refs["word_sums"] = (sums, WORD_SUM_TOL)
    return refs


KINDS = {"self": (launch_self, reference_self), "maps": (launch_maps, reference_maps),
         "pv": (launch_pv, reference_pv), "cross": (launch_cross, reference_cross)}


# ---------------------------------------------------------------------------- the check
def run_case(c, dev):
    """The dense launch against the reference; every other layout against the same reference and,
    bit for bit, against the dense launch; the o buffer's sentinels.  broadcast_kv computes with
    entry 0's k, v for every entry: its baseline is the dense launch on materialised copies."""
    launch, reference = KINDS[c.kind]
    problems, worst = [], {}

    def compare(ops, got, extra, refs, base):
        tag = ops.layout if base is not None else "dense"
        problems.extend(f"{tag}: {x}" for x in extra)
        for name, (want, bound) in refs.items():
            x = got[name].float()
            if not torch.isfinite(x).all():
                problems.append(f"{tag}: {name} has {int((~torch.isfinite(x)).sum())} non-finite elements")
                continue
            err = (x - want).abs().max().item()
            worst[name] = max(worst.get(name, 0.0), err / bound)
            if not err < bound:
                problems.append(f"{tag}: {name} off the reference by {err:.3e} (bound {bound:.3e})")
            if base is not None and not al.same_bits(got[name], base[name]):
                diff = (x - base[name].float()).abs().max().item()
                problems.append(f"{tag}: {name} is not bit-identical to the dense launch (max difference {diff:.3e})")
        problems.extend(f"{tag}: {x}" for x in al.padding_report(ops.views["o"]) + al.unwritten_report(ops.views["o"]))

    for kv_entry0 in ((False, True) if c.kind == "cross" else (False,)):
        dense = c.build("dense", dev, kv_entry0=kv_entry0)
        base, extra = launch(c, dense)
        refs = reference(c, dense.dense, base)
        compare(dense, base, extra, refs, None)
        for layout in (["broadcast_kv"] if kv_entry0 else c.layouts()):
            ops = c.build(layout, dev)
            got, extra = launch(c, ops)
            compare(ops, got, extra, refs, base)
    print(f"layouts {c.id} [{c.kernel}] worst error / bound: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    assert not problems, f"{c.id}: " + "; ".join(problems)


@pytest.mark.parametrize("c", SELF_CASES, ids=lambda c: c.id)
def test_self_layouts(cuda, c):
    run_case(c, cuda)


@pytest.mark.parametrize("c", MAPS_CASES, ids=lambda c: c.id)
def test_self_maps_layouts(cuda, c):
    run_case(c, cuda)


@pytest.mark.parametrize("c", PV_CASES, ids=lambda c: c.id)
def test_materialise_layouts(cuda, c):
    run_case(c, cuda)


@pytest.mark.parametrize("c", CROSS_CASES, ids=lambda c: c.id)
def test_cross_layouts(cuda, c):
    run_case(c, cuda)


def test_wrong_view_is_seen(cuda):
    """Negative control: V's view built with K's row stride -- a reinterpretation of a valid, finite
    buffer (finite filler, the smaller stride: nothing outside the buffer is touched) -- must fail
    the comparison the layout tests apply."""
    c = next(x for x in SELF_CASES if x.id == "fused_64x8_nomax")
    ops = c.build("skewed", cuda, filler=0.5)
    assert ops.views["k"].ld < ops.views["v"].ld
    v_wrong = ops.views["v"].tensor(ld=ops.views["k"].ld)
    refs = reference_self(c, ops.dense, None)
    want, bound = refs["o"]
    _hip.self_attn(ops.q, ops.k, ops.v, ops.o, c.H, c.scale, compute=c.compute)
    right = (ops.o.float() - want).abs().max().item()
    _hip.self_attn(ops.q, ops.k, v_wrong, ops.o, c.H, c.scale, compute=c.compute)
    wrong = (ops.o.float() - want).abs().max().item()
    print(f"wrong view: error / bound {right / bound:.3f} with V's stride, {wrong / bound:.1f} with K's")
    assert right < bound
    assert wrong > bound
