"""Operand layouts for the attention kernels' tests (plain torch; runs on the CPU and on the GPU).

Every U-Net launch of the product hands the kernels strided views (ptp_utils._project: q, k, v are
column slices of one [N, P, 3C] projection for self attention, k, v slices of a cached [N, K, 2C]
one for cross attention).  build() makes the same q / k / v values -- make_qkv's generator recipe,
so the bounds of tests/test_gpu_kernels.py apply unchanged -- available under a named layout:

  dense         contiguous tensors: the baseline the others are compared with
  fused_self    q, k, v column slices of one [N, P, 3C] buffer (P == K), o dense
  fused_cross   q dense, k, v column slices of one [N, K, 2C] buffer, o dense
  skewed        four padded buffers, all eight strides pairwise different: row strides C + 8, C + 16,
                C + 24, C + 32 elements for q, k, v, o, batch strides rows * row_stride plus a
                different multiple of 8 each, every view a non-zero multiple of 8 elements into its
                buffer -- a mix-up between any two strides moves data
  broadcast_kv  q, o dense, k and v one entry expanded over the batch (batch stride 0)

Every element of an input buffer that belongs to no view is `filler` (NaN on the GPU: a kernel may
load it only to discard it by select -- multiplied by a zero probability it still gives NaN).
Every element of the o buffer, inside and outside the view, starts as a fixed bit pattern (SENTINEL);
after a launch padding_report() names every element outside the view that changed and
unwritten_report() every element inside it that did not.  Each buffer is longer than its view
needs, by enough that a kernel which took any other operand's stride or row count for this one
still stays inside the allocation: the mistake shows as wrong data or a spoilt sentinel, never as
an access outside the buffer.
"""
from dataclasses import dataclass, field

import torch

LAYOUTS = ("dense", "fused_self", "fused_cross", "skewed", "broadcast_kv")

# finite in bf16 (2.1e36), f16 (63904) and f32 (2.1e36), far from any attention output, not a NaN:
# NaN-ness of the output is checked apart from "was it written"
SENTINEL = {2: 0x7BCD, 4: 0x7BCD1234}
_INT = {2: torch.int16, 4: torch.int32}

# skewed: (row-stride pad, batch-stride pad, lead-in) in elements, multiples of 8, per operand
_SKEW = {"q": (8, 40, 8), "k": (16, 24, 24), "v": (24, 56, 16), "o": (32, 8, 40)}
_TAIL = 64


@dataclass
class View:
    """One operand: a [N, rows, C] view of `buf` (1-D) at element `offset` with the given strides."""
    buf: torch.Tensor
    offset: int
    shape: tuple
    bs: int
    ld: int

    def tensor(self, ld=None, bs=None):
        """The view; ld / bs override a stride (the negative controls' deliberately wrong views)."""
        return self.buf.as_strided(self.shape, (self.bs if bs is None else bs, self.ld if ld is None else ld, 1),
                                   self.offset)


@dataclass
class Operands:
    layout: str
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    o: torch.Tensor
    views: dict                      # name -> View
    dense: dict                      # name -> contiguous [N, rows, C] copy of the input's values
    bufs: dict = field(default_factory=dict)   # distinct buffers by name ("qkv", "kv", "q", ...)


def applies(layout, P, K, cross):
    """Whether a case of this shape runs under `layout`."""
    if layout == "fused_self":
        return not cross and P == K
    if layout in ("fused_cross", "broadcast_kv"):
        return cross
    return layout in ("dense", "skewed")


def values(N, P, K, H, d, dtype, seed, qscale=1.0, dev="cpu"):
    """make_qkv's recipe (tests/test_gpu_kernels.py), on `dev`'s generator."""
    g = torch.Generator(device=dev).manual_seed(seed)
    C = H * d
    q = (torch.randn(N, P, C, device=dev, generator=g) * qscale).to(dtype)
    k = torch.randn(N, K, C, device=dev, generator=g).to(dtype)
    v = torch.randn(N, K, C, device=dev, generator=g).to(dtype)
    return q, k, v


def _geometry(layout, N, P, K, C):
    """name -> (buffer name, offset, rows, batch stride, row stride), strides in elements."""
    rows = {"q": P, "k": K, "v": K, "o": P}
    g = {n: (n, 0, rows[n], rows[n] * C, C) for n in "qkvo"}
    if layout == "fused_self":
        assert P == K, "fused_self: q, k, v are slices of one [N, P, 3C] projection"
        for i, n in enumerate("qkv"):
            g[n] = ("qkv", i * C, P, P * 3 * C, 3 * C)
    elif layout == "fused_cross":
        for i, n in enumerate("kv"):
            g[n] = ("kv", i * C, K, K * 2 * C, 2 * C)
    elif layout == "skewed":
        for n in "qkvo":
            pad, bpad, lead = _SKEW[n]
            g[n] = (n, lead, rows[n], rows[n] * (C + pad) + bpad, C + pad)
        strides = [g[n][3] for n in "qkvo"] + [g[n][4] for n in "qkvo"]
        assert len(set(strides)) == 8, strides
    elif layout == "broadcast_kv":
        for n in "kv":
            g[n] = (n, 0, K, 0, C)
    else:
        assert layout == "dense", layout
    return g


def build(N, P, K, H, d, dtype, seed, layout, qscale=1.0, dev="cpu", filler=float("nan"), kv_entry0=False):
    """kv_entry0: every entry's k, v hold entry 0's values (what broadcast_kv computes, materialised:
    the dense launch a broadcast_kv launch is compared with)."""
    C = H * d
    geo = _geometry(layout, N, P, K, C)
    q, k, v = values(N, P, K, H, d, dtype, seed, qscale, dev)
    if layout == "broadcast_kv" or kv_entry0:
        k, v = k[:1].expand(N, K, C).contiguous(), v[:1].expand(N, K, C).contiguous()
    dense = {"q": q, "k": k, "v": v}
    # the furthest element any mix of this case's strides and row counts reaches, from any lead-in
    reach = (max(x[1] for x in geo.values()) + (N - 1) * max(x[3] for x in geo.values()) +
             (max(P, K) - 1) * max(x[4] for x in geo.values()) + C + _TAIL)
    es = torch.empty((), dtype=dtype).element_size()
    bufs, views = {}, {}
    for n in "qkvo":
        bname, off, rows, bs, ld = geo[n]
        if bname not in bufs:
            if n == "o":
                bufs[bname] = torch.full((reach,), SENTINEL[es], dtype=_INT[es], device=dev).view(dtype)
            else:
                bufs[bname] = torch.full((reach,), filler, dtype=dtype, device=dev)
        views[n] = View(bufs[bname], off, (N, rows, C), bs, ld)
    for n in "qkv":
        src = dense[n][:1] if views[n].bs == 0 else dense[n]
        t = views[n].tensor()
        (t[:1] if views[n].bs == 0 else t).copy_(src)
    return Operands(layout, views["q"].tensor(), views["k"].tensor(), views["v"].tensor(), views["o"].tensor(),
                    views, dense, bufs)


def _bits(t):
    return t.view(_INT[t.element_size()])


def _inside(view):
    m = torch.zeros(view.buf.numel(), dtype=torch.bool, device=view.buf.device)
    m.as_strided(view.shape, (view.bs, view.ld, 1), view.offset).fill_(True)
    return m


def _where(view, i):
    """In words, where element i of the buffer lies relative to the view."""
    N, rows, C = view.shape
    rel = i - view.offset
    if rel < 0:
        return "before the view"
    n = min(rel // view.bs, N - 1) if view.bs > 0 else 0
    rel -= n * view.bs
    r, c = rel // view.ld, rel % view.ld
    if r >= rows:
        return f"after entry {n}'s last row" + (" (between batch entries)" if n < N - 1 else " (the tail)")
    return f"entry {n} row {r} column {c}" + (" (the padding after the row)" if c >= C else "")


def _report(view, bad, what, limit):
    idx = bad.nonzero().flatten()
    out = [f"{what}: buffer element {i} = {_where(view, i)}" for i in idx[:limit].tolist()]
    if idx.numel() > limit:
        out.append(f"... and {idx.numel() - limit} more")
    return out


def padding_report(view, limit=8):
    """The elements of an output buffer outside the view that no longer hold the sentinel."""
    bits = _bits(view.buf)
    return _report(view, (bits != SENTINEL[view.buf.element_size()]) & ~_inside(view), "written outside the view",
                   limit)


def unwritten_report(view, limit=8):
    """The elements inside the view that still hold the sentinel."""
    bits = _bits(view.buf)
    return _report(view, (bits == SENTINEL[view.buf.element_size()]) & _inside(view), "never written", limit)


def check_output(ops):
    """After a launch: nothing outside o's view was written, everything inside it was."""
    problems = padding_report(ops.views["o"]) + unwritten_report(ops.views["o"])
    assert not problems, f"{ops.layout}: " + "; ".join(problems)


# -- a guarded f32 buffer for the kept maps / materialised probabilities / word sums: `used` elements
# between two runs of sentinel floats that must survive the launch
GUARD = 12345.0


def guarded(numel, guard, dev, fill=0.0):
    """(buffer, used view): `guard` sentinel floats before and after `numel` elements of `fill`."""
    buf = torch.full((numel + 2 * guard,), GUARD, dtype=torch.float32, device=dev)
    buf[guard:guard + numel] = fill
    return buf, buf[guard:guard + numel]


def guards_intact(buf, numel, guard):
    return bool((buf[:guard] == GUARD).all() and (buf[guard + numel:] == GUARD).all())


def same_bits(a, b):
    """Bit-for-bit equality (a NaN equals the same NaN, -0.0 differs from 0.0)."""
    return a.shape == b.shape and bool(torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))
