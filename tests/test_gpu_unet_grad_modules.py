"""The U-Net modules under autograd on the fused glue (unet.fused_glue_grad, p2p_amd/unet_grad.py):
the input gradient three ways -- the fused path, the torch lines (P2P_FUSE_UNET_GRAD off) and the
same module in f32 -- with the module's weights frozen, as the pipelines run it.

The fused path must have run (its backward bindings are counted), its forward output must have the
bits of the no-grad fused output, and its gradient's relative L2 error against the f32 module may be
at most twice the torch lines' on the same inputs (the margin test_gpu_null_batch.py gives two
equivalent paths; the fused chain rounds less often, so it is expected below 1x).  Both errors are
printed.  The convolutions run on PyTorch's native path, as in the other bit-identity tests: MIOpen's
default ones are not reproducible from run to run.
"""
import copy

import pytest
import torch

from test_gpu_unet_glue import DTYPES, rand

from p2p_amd import _hip, unet

pytestmark = pytest.mark.gpu

BWD = ("group_norm_bwd", "geglu_bwd", "nchw_to_tokens")


@pytest.fixture
def native_convs():
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = was


@pytest.fixture
def calls(monkeypatch):
    """How often each backward binding ran."""
    n = dict.fromkeys(BWD, 0)
    for name in BWD:
        fn = getattr(_hip, name)

        def counted(*a, _fn=fn, _name=name, **kw):
            n[_name] += 1
            return _fn(*a, **kw)

        monkeypatch.setattr(_hip, name, counted)
    return n


def _identity_attention(m):
    for blk in m.transformer_blocks:
        blk.attn1.forward = blk.attn2.forward = lambda y, context=None: y
    return m


def rel_l2(a, ref):
    return ((a.double() - ref.double()).norm() / ref.double().norm()).item()


def bits(t):
    return t.contiguous().view(torch.int16)


def three_ways(cuda, monkeypatch, calls, make, args, dtype, expect):
    """args: 16-bit tensors, the first is differentiated.  expect: the bindings that must have run."""
    torch.manual_seed(0)
    m32 = make().to(cuda).eval().requires_grad_(False)
    m16 = copy.deepcopy(m32).to(dtype)

    def grad_of(m, cast):
        leaf = cast(args[0]).detach().requires_grad_(True)
        out = m(leaf, *[cast(t) for t in args[1:]])
        dy = rand(tuple(out.shape), dtype, cuda, 77)
        out.backward(cast(dy))
        return out.detach(), leaf.grad

    _, ref = grad_of(m32, lambda t: t.float())
    with torch.no_grad():
        inference = m16(*args)
    assert unet.fused_glue_grad(args[0])
    out, fused = grad_of(m16, lambda t: t)
    ran = {k: v for k, v in calls.items() if v}
    assert set(ran) == set(expect), f"backward bindings that ran: {ran}"
    assert torch.equal(bits(out), bits(inference)), "the forward under autograd differs from the no-grad forward"
    # nothing requires grad: the inference call, no graph
    with torch.enable_grad():
        plain_out = m16(*args)
    assert plain_out.grad_fn is None and not plain_out.requires_grad and torch.equal(bits(plain_out), bits(inference))
    monkeypatch.setattr(unet, "FUSE_UNET_GRAD", False)
    assert not unet.fused_glue_grad(args[0])
    before = dict(calls)
    _, plain = grad_of(m16, lambda t: t)
    assert calls == before, "the torch lines called a backward binding"
    e_f, e_p = rel_l2(fused, ref), rel_l2(plain, ref)
    print(f"{type(m32).__name__} {dtype} {tuple(args[0].shape)}: relative L2 error of the input gradient: "
          f"fused {e_f:.4e}, torch lines {e_p:.4e} (ratio {e_f / e_p:.2f})")
    assert torch.isfinite(fused).all() and fused.dtype == dtype and fused.shape == args[0].shape
    assert e_f <= 2 * e_p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [8, 16])
def test_geglu_module(cuda, monkeypatch, calls, native_convs, dtype, hw):
    three_ways(cuda, monkeypatch, calls, lambda: unet.GEGLU(64, 256), (rand((2, hw * hw, 64), dtype, cuda, 51),), dtype,
               ["geglu_bwd"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [8, 16])
@pytest.mark.parametrize("cin,cout,temb", [(64, 128, True), (128, 128, True), (64, 64, False)],
                         ids=["shortcut", "no-shortcut", "no-temb"])
def test_resnet_block_module(cuda, monkeypatch, calls, native_convs, dtype, hw, cin, cout, temb):
    args = (rand((2, cin, hw, hw), dtype, cuda, 52),) + ((rand((2, 64), dtype, cuda, 53),) if temb else ())
    three_ways(cuda, monkeypatch, calls, lambda: unet.ResnetBlock2D(cin, cout, temb_ch=64 if temb else None), args,
               dtype, ["group_norm_bwd"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [8, 16])
@pytest.mark.parametrize("C", [64, 128])
def test_transformer_module(cuda, monkeypatch, calls, native_convs, dtype, hw, C):
    """Attention stubbed to identity (its backward has tests of its own and no f16 form): GroupNorm
    to tokens, GEGLU and the token-major residual all differentiate on the kernels."""
    args = (rand((2, C, hw, hw), dtype, cuda, 54), rand((2, 5, 32), dtype, cuda, 55))
    three_ways(cuda, monkeypatch, calls,
               lambda: _identity_attention(unet.Transformer2DModel(8, C // 8, C, context_dim=32)), args, dtype, BWD)


def test_trainable_parameters_keep_the_torch_lines(cuda, calls):
    """A module whose weights want gradients is declined before the forward, and gets them."""
    torch.manual_seed(0)
    m = unet.ResnetBlock2D(64, 64, temb_ch=64).to(cuda, torch.bfloat16)
    x = rand((2, 64, 8, 8), torch.bfloat16, cuda, 56).requires_grad_(True)
    m(x, rand((2, 64), torch.bfloat16, cuda, 57)).sum().backward()
    assert not any(calls.values())
    assert x.grad is not None and m.norm1.weight.grad is not None and m.conv2.bias.grad is not None
