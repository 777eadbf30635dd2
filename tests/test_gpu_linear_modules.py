"""The feed-forward on p2p_linear inside the U-Net's modules (unet.LINEAR_HIP): GEGLU and
BasicTransformerBlock three ways -- with the switch on, the torch lines (switch off: hipBLASLt's
GEMMs, geglu_kernel and torch's add) and the same module in f32 -- at (2, 64 tokens, C = 64) and
(2, 256 tokens, C = 128) in both dtypes, attention stubbed to identity.

The new binding must have run, and the relative L2 error of the "on" output against the f32 module
may be at most the torch lines' on the same inputs: the kernel rounds once where the chain rounds the
pre-activation (and the GEMM's output before the add) as well.  Both errors are printed.  One
Transformer2DModel forward captured into a HIP graph must replay to the eager bits."""
import copy

import pytest
import torch

from test_gpu_unet_glue import DTYPES, rand

from p2p_amd import _hip, unet

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (256, 128)]   # (tokens, C)


@pytest.fixture
def linear_calls(monkeypatch):
    """The forms p2p_linear's binding served, in call order."""
    forms = []
    real = _hip.linear

    def counted(x, weight, bias=None, form=_hip.LINEAR_BIAS, **kw):
        out = real(x, weight, bias, form, **kw)
        if out is not None:
            forms.append(form)
        return out

    monkeypatch.setattr(_hip, "linear", counted)
    return forms


def rel_l2(a, ref):
    return ((a.double() - ref.double()).norm() / ref.double().norm()).item()


def three_ways(cuda, monkeypatch, linear_calls, make, x, dtype, expect):
    torch.manual_seed(0)
    m32 = make().to(cuda).eval().requires_grad_(False)
    m16 = copy.deepcopy(m32).to(dtype)
    with torch.no_grad():
        ref = m32(x.float())
        assert unet.LINEAR_HIP and not linear_calls
        on = m16(x)
        assert linear_calls == expect, f"p2p_linear forms that ran: {linear_calls}"
        monkeypatch.setattr(unet, "LINEAR_HIP", False)
        lines = m16(x)
        assert linear_calls == expect, "the torch lines called p2p_linear"
    e_on, e_lines = rel_l2(on, ref), rel_l2(lines, ref)
    print(f"{type(m32).__name__} {dtype} {tuple(x.shape)}: relative L2 error against the f32 module: "
          f"P2P_LINEAR on {e_on:.4e}, torch lines {e_lines:.4e} (ratio {e_on / e_lines:.2f})")
    assert on.dtype == dtype and on.shape == ref.shape and torch.isfinite(on).all()
    assert e_on <= e_lines


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,C", SIZES)
def test_geglu_module(cuda, monkeypatch, linear_calls, dtype, tokens, C):
    three_ways(cuda, monkeypatch, linear_calls, lambda: unet.GEGLU(C, 4 * C), rand((2, tokens, C), dtype, cuda, 61), dtype,
               [_hip.LINEAR_GEGLU])


def _block(C):
    blk = unet.BasicTransformerBlock(C, 8, C // 8, 32)
    blk.attn1.forward = blk.attn2.forward = lambda y, context=None: y
    return blk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,C", SIZES)
def test_transformer_block_module(cuda, monkeypatch, linear_calls, dtype, tokens, C):
    three_ways(cuda, monkeypatch, linear_calls, lambda: _block(C), rand((2, tokens, C), dtype, cuda, 62), dtype,
               [_hip.LINEAR_GEGLU, _hip.LINEAR_RESIDUAL])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,C", SIZES)
def test_graph_capture(cuda, linear_calls, dtype, tokens, C):
    torch.manual_seed(0)
    m = unet.Transformer2DModel(8, C // 8, C, context_dim=32).to(cuda, dtype).eval().requires_grad_(False)
    for blk in m.transformer_blocks:
        blk.attn1.forward = blk.attn2.forward = lambda y, context=None: y
    hw = int(tokens ** 0.5)
    x, ctx = rand((2, C, hw, hw), dtype, cuda, 63), rand((2, 5, 32), dtype, cuda, 64)
    with torch.no_grad():
        eager = m(x, ctx)
        assert linear_calls == [_hip.LINEAR_GEGLU, _hip.LINEAR_RESIDUAL]
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            m(x, ctx)                                   # warm-up on the capture stream
        torch.cuda.current_stream(cuda).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m(x, ctx)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(cuda)
    assert len(linear_calls) == 6
    assert torch.equal(out, eager)
