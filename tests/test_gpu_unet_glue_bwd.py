"""The backward kernels of the U-Net glue (p2p_group_norm_bwd, p2p_geglu_bwd, p2p_nchw_to_tokens)
against torch autograd of the same formulas in f32 from the same 16-bit inputs and dy.  The bar is
``check`` of test_gpu_unet_glue.py -- |y - ref| <= u |ref| + u max|ref| 1e-2, u = 2^-8 (bf16) or
2^-10 (f16): f32 arithmetic and one rounding, the forward's contract.  torch's own 16-bit autograd
chain is printed beside each figure.  Every case also checks that a second launch gives the same
bits, that dy = 0 gives exact zeros, and that a sample's gradient has the bits it has when that
sample is launched alone (the batched null-text inversion relies on the last two).

The formulas evaluated in f32 on the CPU, rounded once, against f64 autograd sit at most at 0.97 of
the bar in bf16 and 0.49 in f16 (GroupNorm) and 0.975 / 0.48 (GEGLU); torch's 16-bit chain at 1.8 to
42.  Measured on an MI355X, worst over the cases of this file: GroupNorm backward 0.977 (bf16) and
0.488 (f16), torch's 16-bit chain 1.6 to 34 and 0.76 to 20; GEGLU backward 0.962 and 0.481, torch's
chain 1.7 to 1.8 and 0.83 to 0.85.
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_unet_glue import DTYPES, check, rand

from p2p_amd import _hip

pytestmark = pytest.mark.gpu

# from this many pixels a channel's row of the NCHW reduce takes a workgroup, below it a wave
# (kGnBwdWideRow, csrc/p2p_kernels.h)
WIDE_ROW = 2048


def bits(t):
    return t.contiguous().view(torch.int16)


def gn_bwd_case(dev, dtype, N, C, H, W, groups, silu, tokens, add, eps=1e-5):
    """add: None, "c" ([C]) or "nc+bias" ([N, C] and a [C] bias)."""
    x = rand((N, C, H, W), dtype, dev, 1, 2.0, 0.5)
    gamma, beta = rand((C,), dtype, dev, 2, 0.5, 1.0), rand((C,), dtype, dev, 3)
    chan_add = {None: None, "c": rand((C,), dtype, dev, 4), "nc+bias": rand((N, C), dtype, dev, 4)}[add]
    chan_bias = rand((C,), dtype, dev, 5) if add == "nc+bias" else None
    dy = rand((N, H * W, C) if tokens else (N, C, H, W), dtype, dev, 6)
    kw = dict(silu=silu, tokens=tokens)

    def run(x_, dy_, add_):
        y, stats = _hip.group_norm(x_, gamma, beta, groups, eps, chan_add=add_, chan_bias=chan_bias,
                                   return_stats=True, **kw)
        return _hip.group_norm_bwd(dy_, x_, stats, gamma, beta, groups, chan_add=add_, chan_bias=chan_bias, **kw)

    def formula(t, cast):
        if chan_add is not None:
            t = t + cast(chan_add).reshape((N, C, 1, 1) if chan_add.dim() == 2 else (1, C, 1, 1))
        if chan_bias is not None:
            t = t + cast(chan_bias).reshape(1, C, 1, 1)
        t = F.group_norm(t, groups, cast(gamma), cast(beta), eps)
        t = F.silu(t) if silu else t
        return t.permute(0, 2, 3, 1).reshape(N, H * W, C) if tokens else t

    def autograd(cast):
        leaf = cast(x).detach().requires_grad_(True)
        formula(leaf, cast).backward(cast(dy))
        return leaf.grad

    dx = run(x, dy, chan_add)
    assert dx.shape == x.shape and dx.dtype == dtype and dx.is_contiguous()
    ref, chain = autograd(lambda t: t.float()), autograd(lambda t: t)
    check(dx, ref, dtype, f"group_norm_bwd N={N} C={C} {H}x{W} g={groups} silu={silu} tokens={tokens} add={add} {dtype}",
          chain)
    assert torch.equal(bits(dx), bits(run(x, dy, chan_add))), "two launches on the same input differ"
    assert (run(x, torch.zeros_like(dy), chan_add) == 0).all(), "dy = 0 must give exact zeros"
    # one sample's dy zero in the batch: that sample's dx is exactly zero, the others keep their bits
    if N > 1:
        dy0 = dy.clone()
        dy0[1].zero_()
        dx0 = run(x, dy0, chan_add)
        assert (dx0[1] == 0).all() and torch.equal(bits(dx0[0]), bits(dx[0]))
        for b in range(N):
            add_b = chan_add[b:b + 1].contiguous() if chan_add is not None and chan_add.dim() == 2 else chan_add
            alone = run(x[b:b + 1].contiguous(), dy[b:b + 1].contiguous(), add_b)
            assert torch.equal(bits(alone[0]), bits(dx[b])), f"sample {b} alone differs from its place in N={N}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("add", [None, "c", "nc+bias"])
def test_group_norm_bwd_cpg10(cuda, dtype, tokens, silu, add):
    gn_bwd_case(cuda, dtype, 1, 320, 16, 16, 32, silu, tokens, add)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C,H,W,groups", [
    (2, 64, 8, 8, 32),
    (2, 72, 3, 8, 9),         # partial tiles in both directions of the transpose
    (3, 1920, 8, 8, 32),      # the widest real C; sample b against the N = 1 launch
    (1, 1024, 32, 32, 32),    # the two sides of the forward's statistics-width threshold
    (1, 1024, 127, 8, 32),
    (2, 64, 32, 64, 32),      # hw = WIDE_ROW: a workgroup per channel row in the NCHW reduce; 32 pixel tiles
    (1, 64, 255, 8, 32),      # hw just below it: one wave per row
])
def test_group_norm_bwd_shapes(cuda, dtype, N, C, H, W, groups):
    assert (N, C, H, W) != (2, 64, 32, 64) or H * W == WIDE_ROW
    assert (N, C, H, W) != (1, 64, 255, 8) or H * W == WIDE_ROW - 8
    gn_bwd_case(cuda, dtype, N, C, H, W, groups, True, False, "nc+bias")
    gn_bwd_case(cuda, dtype, N, C, H, W, groups, False, True, None, eps=1e-6)
    gn_bwd_case(cuda, dtype, N, C, H, W, groups, True, True, "c")


def test_group_norm_return_stats(cuda):
    """The statistics handed back are the ones the forward used, and asking for them changes nothing."""
    x = rand((2, 64, 8, 8), torch.bfloat16, cuda, 1, 2.0, 0.5)
    g, b = rand((64,), torch.bfloat16, cuda, 2, 0.5, 1.0), rand((64,), torch.bfloat16, cuda, 3)
    y, stats = _hip.group_norm(x, g, b, 32, 1e-5, silu=True, return_stats=True)
    assert torch.equal(y, _hip.group_norm(x, g, b, 32, 1e-5, silu=True))
    xs = x.float().reshape(2, 32, -1)
    st = stats[:2 * 32 * 2].reshape(2, 32, 2)
    torch.testing.assert_close(st[..., 0], xs.mean(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st[..., 1], (xs.var(-1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [64, 100])
def test_geglu_bwd(cuda, dtype, M):
    D = 1280
    buf = rand((M, 2 * D + 64), dtype, cuda, 7, 2.0)
    x = buf[:, :2 * D]                                  # row stride 2 D + 64
    dout = rand((M, D), dtype, cuda, 8)
    din = _hip.geglu_bwd(dout, x)
    assert din.shape == (M, 2 * D) and din.dtype == dtype and din.is_contiguous()

    def autograd(cast):
        leaf = cast(x).detach().requires_grad_(True)
        h, gate = leaf.chunk(2, dim=-1)
        (h * F.gelu(gate)).backward(cast(dout))
        return leaf.grad

    ref, chain = autograd(lambda t: t.float()), autograd(lambda t: t)
    check(din[:, :D], ref[:, :D], dtype, f"geglu_bwd d(h) M={M} D={D} {dtype}", chain[:, :D])
    check(din[:, D:], ref[:, D:], dtype, f"geglu_bwd d(gate) M={M} D={D} {dtype}", chain[:, D:])
    assert torch.equal(bits(din), bits(_hip.geglu_bwd(dout, x)))
    assert (_hip.geglu_bwd(torch.zeros_like(dout), x) == 0).all()
    # the dense 3-D input the module passes
    x3 = x.contiguous().reshape(2, M // 2, 2 * D)
    din3 = _hip.geglu_bwd(dout.reshape(2, M // 2, D), x3)
    assert din3.shape == x3.shape and torch.equal(bits(din3.reshape(M, 2 * D)), bits(din))
    # a row alone has the bits it has among the others
    assert torch.equal(bits(_hip.geglu_bwd(dout[3:4].contiguous(), x[3:4])), bits(din[3:4]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C,H,W", [(2, 320, 8, 8), (2, 72, 3, 8)])
def test_nchw_to_tokens(cuda, dtype, N, C, H, W):
    src = rand((N, C, H, W), dtype, cuda, 9)
    dst = _hip.nchw_to_tokens(src)
    assert dst.shape == (N, H * W, C) and dst.is_contiguous()
    assert torch.equal(bits(dst), bits(src.permute(0, 2, 3, 1).contiguous().reshape(N, H * W, C)))
    assert torch.equal(bits(dst), bits(_hip.nchw_to_tokens(src)))
    assert (_hip.nchw_to_tokens(torch.zeros_like(src)) == 0).all()
    assert torch.equal(bits(_hip.nchw_to_tokens(src[1:2].contiguous())[0]), bits(dst[1]))


def test_unsupported_backward_raises(cuda):
    """What the forward declines with None the backward bindings answer with HipError: the caller
    decides before the forward."""
    with pytest.raises(_hip.HipError):
        _hip.geglu_bwd(torch.zeros(4, 1280, device=cuda), torch.zeros(4, 2560, device=cuda))
    with pytest.raises(_hip.HipError):
        _hip.nchw_to_tokens(torch.zeros(1, 64, 3, 3, device=cuda, dtype=torch.bfloat16))
