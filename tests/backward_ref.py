"""The attention autograd pair (p2p_attn_fwd_lse + p2p_attn_bwd) in plain torch -- test
infrastructure, never the product: a float64 reference with the absolute-value bounds the tests
hold the kernels to, a float32 restatement of the roundings the kernels make (with three seeded
faults), the shapes both test modules run, and the bounds themselves.

Layouts are the C ABI's: q / dout / O / dQ [N, P, H*d], k / v / dK / dV [N, K, H*d], lse / delta
[N*H, P] f32.  lse is in log2 units with the scale folded in: log2 sum_k exp2(scale * log2(e) * s_k).
"""
import functools

import torch

LOG2E = 1.4426950408889634
U = 2.0 ** -9          # bf16 unit roundoff

# ---------------------------------------------------------------------------- bounds
# bf16 tensors (derivation: DESIGN.md §5).  lse: l sums same-signed terms each within u, so log2 l
# moves by <= log2(e) * u ~ 2^-8.5; S from exact bf16 products in f32 adds ~ d * 2^-24 * |c S|;
# 2^-7 is more than twice that.  Elementwise: |got - ref| <= 8u * B with B the same product taken
# over absolute values (P, lse into P, the output and delta-from-rounded-O: <= 4u, doubled).
# Frobenius (K > 1): ||got - ref|| / ||ref|| <= 6u, which a uniform scale error cannot hide in.
LSE_ABS = 2.0 ** -7
ELEM_BF16 = 8 * U
FROB_BF16 = 6 * U
# f32 tensors: the backward reads V, dO and the K / Q that dS multiplies as bf16 (roundings that
# enter linearly) and recomputes S split-bf16, as the forward that wrote the lse forms it.  Each
# bound is 2x the maximum of emulate() against reference() over CASES on the CPU, and never above
# the project's 3e-2 (= 15.4 u) -- test_f32_bounds_follow_the_rule recomputes this:
#   elementwise maxima (units of u): O 3.08, delta 0.74, dQ 0.91, dK 1.05, dV 3.59 (case 6)
#   Frobenius maxima   (units of u): O 1.03, delta 1.04, dQ 4.49, dK 4.28 (case 9), dV 1.23
# (With S recomputed from Q and K rounded to bf16, as the kernels did before these tests, c S moves
# by ~|c S| 2^-9 and every P by as much: the same emulation gave dV 63.6 u elementwise and 21.9 u
# Frobenius on case 9, outside 3e-2, and so did the GPU.)
ELEM_F32 = 7.2 * U
FROB_F32 = 9 * U
QUANTITIES = ("O", "delta", "dQ", "dK", "dV")

# (N, P, K, heads, d, q-scale), and the query split of the key/value pass each must take
CASES = [
    (2, 70, 37, 2, 40, 2),      # 1  partial dQ workgroup, key blocks 32 + 5, direct store
    (1, 257, 50, 2, 40, 2),     # 2  one split of a single row, one empty split
    (1, 130, 130, 3, 64, 2),    # 3  K over 128 by 2, odd grid, d % 32 == 0 forward
    (2, 100, 77, 2, 80, 2),     # 4  cross-like, P < 2T
    (1, 129, 33, 2, 160, 2),    # 5  T = 32, two-pass dV / dK, K over 32 by 1, empty split
    (1, 129, 129, 2, 160, 8),   # 6  peaky
    (1, 257, 257, 2, 40, 12),   # 7  peaky, three key workgroups
    (2, 64, 1, 2, 64, 2),       # 8  K = 1 (reference dQ = dK = 0 exactly), 2-wave forward
    (1, 130, 130, 2, 80, 16),   # 9  peaky
    (64, 64, 20, 8, 40, 2),     # 10 N at the limit, 512 key workgroups: split 1 by the occupancy rule
    (1, 64, 3328, 8, 160, 2),   # 11 N*K*C = 4,259,840 > 4,194,304: the reduction's stride loop
]
SPLITS = [1, 4, 2, 1, 4, 4, 4, 1, 2, 1, 2]
CASE_IDS = ["%d-%s" % (i + 1, "x".join(map(str, c))) for i, c in enumerate(CASES)]


def make_inputs(index, dtype, device="cpu"):
    """q = q-scale * randn, k / v / dout = randn, seeded by the case: the same values on any device."""
    N, P, K, H, d, qs = CASES[index]
    g = torch.Generator().manual_seed(1000 + index)
    C = H * d
    q = (qs * torch.randn(N, P, C, generator=g)).to(dtype)
    k = torch.randn(N, K, C, generator=g).to(dtype)
    v = torch.randn(N, K, C, generator=g).to(dtype)
    dout = torch.randn(N, P, C, generator=g).to(dtype)
    return tuple(x.to(device) for x in (q, k, v, dout)) + (H, d ** -0.5)


def _heads(x, heads):
    N, T, C = x.shape
    return x.reshape(N, T, heads, C // heads).permute(0, 2, 1, 3)


def _tokens(x):
    N, H, T, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(N, T, H * d)


def reference(q, k, v, dout, heads, scale):
    """float64.  O, lse, delta, dQ, dK, dV and B_<name> for the five bounded quantities."""
    Q, K, V, G = (_heads(x.double(), heads) for x in (q, k, v, dout))
    N, H, P, _ = Q.shape
    s = Q @ K.transpose(-1, -2) * scale
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    Pr = e / l
    lse = ((m + l.log()) * LOG2E).reshape(N * H, P)
    O = Pr @ V
    delta = (G * O).sum(-1, keepdim=True)
    dP = G @ V.transpose(-1, -2)
    dS = Pr * (dP - delta)
    aP = G.abs() @ V.abs().transpose(-1, -2)
    dabs = (Pr * aP).sum(-1, keepdim=True)
    A = Pr * (aP + dabs)
    return {
        "O": _tokens(O), "lse": lse, "delta": delta.reshape(N * H, P),
        "dQ": _tokens(scale * dS @ K), "dK": _tokens(scale * dS.transpose(-1, -2) @ Q),
        "dV": _tokens(Pr.transpose(-1, -2) @ G),
        "B_O": _tokens(Pr @ V.abs()), "B_delta": dabs.reshape(N * H, P),
        "B_dQ": _tokens(scale * A @ K.abs()), "B_dK": _tokens(scale * A.transpose(-1, -2) @ Q.abs()),
        "B_dV": _tokens(Pr.transpose(-1, -2) @ G.abs()),
    }


def _bf(x):
    return x.bfloat16().float()


def _fma(a, b, c):
    """fmaf(a, b, c): one rounding (exact in f64 for f32 operands, then rounded once)."""
    return (a.double() * b.double() + c.double()).float()


def emulate(q, k, v, dout, heads, scale, mutant=None):
    """The kernels' roundings in float32 torch.  q.dtype (bfloat16 or float32) is the io type.
    mutant: "lse" (lse + 2^-5), "lastkey" (P's last key column zero in the dQ path), "lastquery"
    (P's last query row zero in the dK/dV path)."""
    assert mutant in (None, "lse", "lastkey", "lastquery")
    io = q.dtype
    f32 = io == torch.float32
    d = q.shape[-1] // heads
    Q, K, V, G = (_heads(x.float(), heads) for x in (q, k, v, dout))
    N, H, P, _ = Q.shape
    # c = scale * log2(e), both f32 (p2p_capi.hip:46, :367)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    sc = torch.tensor(scale, dtype=torch.float32)

    # ---- forward, self_attn_fused_kernel (p2p_self.hip)
    if f32:
        # split-bf16 Q K^T: hi = bf16(x), lo = bf16(x - hi) (p2p_device.h:203-210), three of the four
        # products (p2p_device.h:333-338), f32 accumulation
        Qh, Kh = _bf(Q), _bf(K)
        Ql, Kl = _bf(Q - Qh), _bf(K - Kh)
        S = Qh @ Kl.transpose(-1, -2) + Ql @ Kh.transpose(-1, -2) + Qh @ Kh.transpose(-1, -2)
    else:
        S = Q @ K.transpose(-1, -2)            # exact bf16 products, f32 accumulation (p2p_self.hip:289)
    # the running max lags the row max by < 8 (p2p_self.hip:309); bf16 and f32 roundings are
    # relative, so the model takes the row max itself: m = max(S) * c (p2p_self.hip:307)
    m = S.max(-1, keepdim=True).values * c
    e = torch.exp2(_fma(S, c, -m))             # p2p_self.hip:325
    eb = _bf(e)                                # P packed to bf16 for the PV MFMA (p2p_device.h:89, :496)
    # row sum: d % 32 != 0 has a ones column in V, so l sums the bf16-rounded exponentials
    # (p2p_self.hip:167, :381); otherwise the f32 sum of the unrounded ones (p2p_self.hip:327, :382)
    l = (eb if d % 32 else e).sum(-1, keepdim=True)
    Vb = _bf(V)                                # V staged as bf16 (p2p_self.hip:256)
    O = ((eb @ Vb) * (1.0 / l)).to(io)         # one rounding to the io type (p2p_self.hip:383, :392)
    lse = m + torch.log2(l)                    # p2p_self.hip:396
    if mutant == "lse":
        lse = lse + 2.0 ** -5

    # ---- backward (p2p_bwd.hip)
    # delta reads dO and the rounded O in the io type, f32 fma (p2p_bwd.hip:51)
    delta = (G * _heads(_tokens(O).float(), heads)).sum(-1, keepdim=True)
    # Q, K, V, dO to bf16 on load (row_frag p2p_bwd.hip:63, TileStage p2p_bwd.hip:118-124): exact for
    # bf16 tensors, a rounding for f32 tensors
    Qb, Kb, Gb = _bf(Q), _bf(K), _bf(G)
    # S: exact bf16 products (p2p_bwd.hip:199, :328); f32 tensors: the forward's split-bf16 sum of
    # three products again (p2p_bwd.hip:192-200, :321-329)
    Sb = S if f32 else Qb @ Kb.transpose(-1, -2)
    Pr = torch.exp2(_fma(Sb, c, -lse))         # p2p_bwd.hip:208, :340
    dP = Gb @ Vb.transpose(-1, -2)             # p2p_bwd.hip:201, :332
    Pq, Pk = Pr, Pr
    if mutant == "lastkey":
        Pq = Pr.clone()
        Pq[..., -1] = 0
    if mutant == "lastquery":
        Pk = Pr.clone()
        Pk[..., -1, :] = 0
    dSq = _bf(Pq * (dP - delta))               # p2p_bwd.hip:209, packed to bf16 in pv_block (:211)
    dSk = _bf(Pk * (dP - delta))               # p2p_bwd.hip:341, :344
    Pb = _bf(Pk)                               # p2p_bwd.hip:343
    dQ = ((dSq @ Kb) * sc).to(io)              # p2p_bwd.hip:227
    dK = ((dSk.transpose(-1, -2) @ Qb) * sc).to(io)   # p2p_bwd.hip:377 (split partials add in f32, :390)
    dV = (Pb.transpose(-1, -2) @ Gb).to(io)    # p2p_bwd.hip:376
    return {"O": _tokens(O), "lse": lse.reshape(N * H, P), "delta": delta.reshape(N * H, P),
            "dQ": _tokens(dQ), "dK": _tokens(dK), "dV": _tokens(dV)}


# ---------------------------------------------------------------------------- the checks
def elem_ratio(got, ref, bound):
    """max |got - ref| / B over the elements (B floored at 1e-30)."""
    return ((got.double() - ref).abs() / (bound + 1e-30)).max().item()


def frob_ratio(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def measure(got, ref):
    """{"lse": abs error, "elem:<name>": ..., "frob:<name>": ...} for whatever `got` holds.
    Frobenius only where the reference is not identically zero by construction (K > 1)."""
    out = {}
    if "lse" in got:
        out["lse"] = (got["lse"].double() - ref["lse"]).abs().max().item()
    many_keys = ref["dK"].shape[1] > 1
    for name in QUANTITIES:
        if name in got:
            out["elem:" + name] = elem_ratio(got[name], ref[name], ref["B_" + name])
            if many_keys:
                out["frob:" + name] = frob_ratio(got[name], ref[name])
    return out


def limits(io_dtype):
    f32 = io_dtype == torch.float32
    return {"lse": LSE_ABS, "elem": ELEM_F32 if f32 else ELEM_BF16, "frob": FROB_F32 if f32 else FROB_BF16}


def violations(figures, io_dtype):
    """The measured figures outside their bound, as {key: (figure, bound)}."""
    lim = limits(io_dtype)
    bad = {}
    for key, val in figures.items():
        bound = lim[key.split(":")[0]]
        if not val <= bound:            # (a NaN is a violation)
            bad[key] = (val, bound)
    return bad


def old_criterion_passes(got, ref):
    """What test_attention_backward asks of the gradients: max error <= 3e-2 * max |ref|, cosine
    >= 0.999 (K > 1: at K = 1 the reference dQ and dK are zero)."""
    for name in ("dQ", "dK", "dV"):
        g, r = got[name].double().flatten(), ref[name].flatten()
        if (g - r).abs().max().item() > 3e-2 * r.abs().max().item():
            return False
        if torch.nn.functional.cosine_similarity(g, r, dim=0).item() < 0.999:
            return False
    return True


@functools.lru_cache(maxsize=None)
def cpu_case(index, dtype):
    """Inputs and the f64 reference of a case on the CPU, computed once."""
    inp = make_inputs(index, dtype)
    return inp, reference(*inp)


def workspace_bytes(index):
    N, P, K, H, d, _ = CASES[index]
    s = SPLITS[index]
    return 0 if s == 1 else 2 * s * N * K * H * d * 4
