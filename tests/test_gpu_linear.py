"""linear_kernel (csrc/p2p_linear.hip) against the same formulas evaluated in f64 from the same 16-bit
inputs, under the bar of tests/test_gpu_unet_glue.py's ``check``: |y - ref| <= u |ref| + u max|ref| 1e-2,
u = 2^-8 (bf16) or 2^-10 (f16) -- the kernel accumulates in f32 and rounds once, so it owes half an
ulp and the reordering of an f32 sum.  Inputs are randn, the weights scaled by K^-1/2.  torch's own
16-bit chain (F.linear, then the gating or the add, one rounding each) is measured on the same inputs
and printed beside the kernel's figure.

The shapes are the smallest at which each mechanism can go wrong: a partial 128-row tile (M = 136),
a partial column tile (N = 96 on BN = 128, D = 96 on the GEGLU form's 64-column tiles), BN = 160
(N = 320), BK = 32 (K = 96) and BK = 64 (K = 64, 320), more than one tile both ways, the K split with
bias and residual (with and without tails), row-strided x and res, a null bias, p_out.
Every compiled instantiation at a small shape: tests/kernel_matrix.py (a kernel change extends that table)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_unet_glue import DTYPES, check, rand

from p2p_amd import _hip

pytestmark = pytest.mark.gpu

BIAS, GEGLU, RES = _hip.LINEAR_BIAS, _hip.LINEAR_GEGLU, _hip.LINEAR_RESIDUAL


def bits(t):
    return t.contiguous().view(torch.int16)


def operands(dev, dtype, M, K, rows, N, strided=False):
    """x [M, K], W [rows, K] * K^-1/2, bias [rows], res [M, N]; ``strided``: x and res are column
    slices of wider tensors (row strides K + 8 and N + 16)."""
    if strided:
        x = rand((M, K + 8), dtype, dev, 11)[:, :K]
        res = rand((M, N + 16), dtype, dev, 14)[:, 8:8 + N]
    else:
        x, res = rand((M, K), dtype, dev, 11), rand((M, N), dtype, dev, 14)
    return x, rand((rows, K), dtype, dev, 12, K ** -0.5), rand((rows,), dtype, dev, 13), res


# (M, K, N): see the module docstring; the split rows are pinned in tests/test_select_linear.py
PLAIN = [(136, 64, 96), (136, 96, 96), (136, 320, 320), (128, 2560, 160), (136, 1024, 96)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("M,K,N", PLAIN)
def test_bias_and_residual(cuda, dtype, M, K, N, strided):
    x, w, b, res = operands(cuda, dtype, M, K, N, N, strided)
    acc = x.double() @ w.double().t()
    for bias in (b, None):
        ref = acc if bias is None else acc + bias.double()
        y = _hip.linear(x, w, bias)
        assert y is not None and y.shape == (M, N) and y.dtype == dtype and y.is_contiguous()
        check(y, ref, dtype, f"linear bias M={M} K={K} N={N} bias={bias is not None} {dtype}", F.linear(x, w, bias))
        assert torch.equal(bits(y), bits(_hip.linear(x, w, bias))), "two launches on the same input differ"
        yr = _hip.linear(x, w, bias, RES, res=res)
        assert yr is not None and yr.shape == (M, N) and yr.dtype == dtype
        check(yr, ref + res.double(), dtype, f"linear residual M={M} K={K} N={N} bias={bias is not None} {dtype}",
              F.linear(x, w, bias) + res)
        assert torch.equal(bits(yr), bits(_hip.linear(x, w, bias, RES, res=res))), "two launches on the same input differ"


def test_the_split_shapes_split(cuda):
    assert _hip.linear_split(RES, 128, 2560, 160) > 1 and _hip.linear_split(BIAS, 128, 2560, 160) > 1
    assert _hip.linear_split(RES, 136, 1024, 96) > 1
    assert all(_hip.linear_split(RES, M, K, N) == 1 for M, K, N in PLAIN[:3])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("M,K,D", [(136, 64, 96), (136, 96, 96), (264, 320, 160)])
def test_geglu(cuda, dtype, M, K, D, strided):
    x, w, b, _ = operands(cuda, dtype, M, K, 2 * D, D, strided)
    for bias in (b, None):
        p_ref = x.double() @ w.double().t() + (0 if bias is None else bias.double())
        ref = p_ref[:, :D] * F.gelu(p_ref[:, D:])
        h, gate = F.linear(x, w, bias).chunk(2, dim=-1)
        y = _hip.linear(x, w, bias, GEGLU)
        assert y is not None and y.shape == (M, D) and y.dtype == dtype and y.is_contiguous()
        check(y, ref, dtype, f"linear geglu M={M} K={K} D={D} bias={bias is not None} {dtype}", h * F.gelu(gate))
        assert torch.equal(bits(y), bits(_hip.linear(x, w, bias, GEGLU))), "two launches on the same input differ"
        y2, p = _hip.linear(x, w, bias, GEGLU, want_p=True)
        assert torch.equal(bits(y2), bits(y)), "asking for p_out changed out"
        assert p.shape == (M, 2 * D) and p.dtype == dtype and p.is_contiguous()
        check(p, p_ref, dtype, f"linear geglu p_out M={M} K={K} D={D} bias={bias is not None} {dtype}",
              F.linear(x, w, bias))


def test_leading_dimensions(cuda):
    """[2, M / 2, K] operands are the [M, K] call."""
    M, K, N = 136, 64, 96
    x, w, b, res = operands(cuda, torch.bfloat16, M, K, N, N)
    y = _hip.linear(x.reshape(2, M // 2, K), w, b, RES, res=res.reshape(2, M // 2, N))
    assert y.shape == (2, M // 2, N) and torch.equal(bits(y.reshape(M, N)), bits(_hip.linear(x, w, b, RES, res=res)))
    wg = rand((2 * N, K), torch.bfloat16, cuda, 15, K ** -0.5)
    g = _hip.linear(x.reshape(2, M // 2, K), wg, None, GEGLU)
    assert g.shape == (2, M // 2, N) and torch.equal(bits(g.reshape(M, N)), bits(_hip.linear(x, wg, None, GEGLU)))


def test_declined_operands(cuda):
    x, w, b, res = operands(cuda, torch.bfloat16, 136, 64, 96, 96)
    assert _hip.linear(x.float(), w.float(), b.float()) is None                  # f32
    assert _hip.linear(x.cpu(), w.cpu(), b.cpu()) is None                        # CPU
    assert _hip.linear(x, w.cpu(), b) is None and _hip.linear(x, w.half(), b) is None
    assert _hip.linear(x, w, None, RES, res=res.float()) is None
    assert _hip.linear(x[:, :48], w[:, :48].contiguous(), b) is None             # K % 32
    assert _hip.linear(x, w[:92], b[:92]) is None                                # N % 8
    assert _hip.linear(x.t().contiguous().t(), w, b) is None                     # no unit last stride
    with pytest.raises(_hip.HipError):
        _hip.linear(x, w, b, RES)                                                # the form wants its operand
