"""The U-Net glue kernels (csrc/p2p_unet.hip) against the same formulas evaluated by torch in f32
from the same 16-bit inputs.  The bar is one output ulp plus a second-order term:
|y - ref| <= u |ref| + u max|ref| 1e-2, u = 2^-8 (bf16) or 2^-10 (f16): the kernels compute in f32
and round once, so they owe half an ulp; the absolute term covers f32 reordering near zero.
torch's own 16-bit chain (one rounding per op) is measured on the same inputs and printed."""
import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, unet

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# gn_stats_kernel runs 1024 threads from this many elements per (n, group) slab, 256 below
# (kGnStatsWide, csrc/p2p_kernels.h)
STATS_WIDE = 32768


def ulp(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -10


def check(y, ref, dtype, what, chain=None):
    u = ulp(dtype)
    tol = u * ref.abs() + u * ref.abs().max() * 1e-2
    err = (y.float() - ref).abs()
    worst = (err / tol).max().item()
    line = f"{what}: worst |y - ref| / bar = {worst:.3f}"
    if chain is not None:
        line += f"; torch's 16-bit chain = {((chain.float() - ref).abs() / tol).max().item():.3f}"
    print(line)
    assert worst <= 1.0, line


def rand(shape, dtype, dev, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, device=dev, generator=g) * scale + shift).to(dtype)


def gn_case(dev, dtype, N, C, H, W, groups, silu, tokens, add, eps=1e-5):
    """add: None, "c" ([C]), "nc" ([N, C]) or "nc+bias" ([N, C] and a [C] bias)."""
    x = rand((N, C, H, W), dtype, dev, 1, 2.0, 0.5)
    gamma, beta = rand((C,), dtype, dev, 2, 0.5, 1.0), rand((C,), dtype, dev, 3)
    chan_add = {None: None, "c": rand((C,), dtype, dev, 4), "nc": rand((N, C), dtype, dev, 4),
                "nc+bias": rand((N, C), dtype, dev, 4)}[add]
    chan_bias = rand((C,), dtype, dev, 5) if add == "nc+bias" else None
    y = _hip.group_norm(x, gamma, beta, groups, eps, silu=silu, tokens=tokens, chan_add=chan_add, chan_bias=chan_bias)
    assert y is not None, "unsupported: the kernel must serve this shape"

    def formula(t, cast):
        if chan_add is not None:
            t = t + cast(chan_add).reshape((N, C, 1, 1) if chan_add.dim() == 2 else (1, C, 1, 1))
        if chan_bias is not None:
            t = t + cast(chan_bias).reshape(1, C, 1, 1)
        t = F.group_norm(t, groups, cast(gamma), cast(beta), eps)
        t = F.silu(t) if silu else t
        return t.permute(0, 2, 3, 1).reshape(N, H * W, C) if tokens else t

    ref = formula(x.float(), lambda t: t.float())
    chain = formula(x, lambda t: t)
    assert y.shape == ref.shape and y.dtype == dtype and y.is_contiguous()
    check(y, ref, dtype, f"group_norm N={N} C={C} {H}x{W} g={groups} silu={silu} tokens={tokens} add={add} {dtype}",
          chain)
    y2 = _hip.group_norm(x, gamma, beta, groups, eps, silu=silu, tokens=tokens, chan_add=chan_add, chan_bias=chan_bias)
    assert torch.equal(y, y2), "two launches on the same input differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("add", [None, "c", "nc", "nc+bias"])
def test_group_norm_cpg10(cuda, dtype, tokens, silu, add):
    # 10 channels per group: 20-byte token runs
    gn_case(cuda, dtype, 1, 320, 16, 16, 32, silu, tokens, add)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C,H,W,groups", [
    (2, 64, 8, 8, 32),        # a group of 128 elements
    (1, 2560, 32, 32, 32),    # a 164 KB group, past LDS residency
    (3, 1920, 8, 8, 32),      # the widest real C
    (1, 1024, 32, 32, 32),    # slab = STATS_WIDE elements: the 1024-thread statistics launch
    (1, 1024, 127, 8, 32),    # slab just below STATS_WIDE: 256 threads; hw no multiple of the 64-pixel tile
    (2, 72, 3, 8, 9),         # partial tiles in both directions of the token-major transpose
])
def test_group_norm_shapes(cuda, dtype, N, C, H, W, groups):
    slab = C // groups * H * W
    assert (N, C, H, W) != (1, 1024, 32, 32) or slab == STATS_WIDE
    assert (N, C, H, W) != (1, 1024, 127, 8) or STATS_WIDE - 8 * C // groups <= slab < STATS_WIDE
    gn_case(cuda, dtype, N, C, H, W, groups, True, False, "nc+bias")
    gn_case(cuda, dtype, N, C, H, W, groups, False, True, None, eps=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [64, 100])
def test_geglu(cuda, dtype, M):
    D = 1280
    buf = rand((M, 2 * D + 64), dtype, cuda, 7, 2.0)
    x = buf[:, :2 * D]                                  # row stride 2 D + 64
    y = _hip.geglu(x)
    assert y is not None and y.shape == (M, D) and y.dtype == dtype
    ref = x[:, :D].float() * F.gelu(x[:, D:].float())
    h, gate = x.chunk(2, dim=-1)
    check(y, ref, dtype, f"geglu M={M} D={D} {dtype}", h * F.gelu(gate))
    assert torch.equal(y, _hip.geglu(x))
    # the dense 3-D input the module passes
    x3 = x.contiguous().reshape(2, M // 2, 2 * D)
    assert torch.equal(_hip.geglu(x3).reshape(M, D), y)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(8, 8), (16, 16)])
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("biases", [0, 1, 2])
def test_bias_residual(cuda, dtype, H, W, tokens, biases, N=2, C=320):
    a = rand((N, C, H, W), dtype, cuda, 11, 2.0)
    b = rand((N, H * W, C) if tokens else (N, C, H, W), dtype, cuda, 12, 2.0)
    bs = [rand((C,), dtype, cuda, 13 + i) for i in range(biases)]
    y = _hip.bias_residual(a, b, *bs, tokens=tokens)
    assert y is not None and y.shape == a.shape and y.dtype == dtype

    def formula(a_, b_, bs_):
        b_ = b_.reshape(N, H, W, C).permute(0, 3, 1, 2) if tokens else b_
        for v in bs_:
            b_ = b_ + v.reshape(1, C, 1, 1)
        return a_ + b_

    ref = formula(a.float(), b.float(), [v.float() for v in bs])
    check(y, ref, dtype, f"bias_residual {H}x{W} tokens={tokens} biases={biases} {dtype}", formula(a, b, bs))
    assert torch.equal(y, _hip.bias_residual(a, b, *bs, tokens=tokens))


def test_bias_residual_partial_tiles(cuda):
    N, C, H, W = 2, 72, 3, 8
    a, b = rand((N, C, H, W), torch.bfloat16, cuda, 21), rand((N, H * W, C), torch.bfloat16, cuda, 22)
    bias = rand((C,), torch.bfloat16, cuda, 23)
    ref = a.float() + b.float().reshape(N, H, W, C).permute(0, 3, 1, 2) + bias.float().reshape(1, C, 1, 1)
    check(_hip.bias_residual(a, b, bias, tokens=True), ref, torch.bfloat16, "bias_residual 72 x 24 tokens")


def test_unsupported_falls_back(cuda):
    # f32 and an odd pixel count are "unsupported", not errors: the binding returns None
    x = torch.randn(1, 64, 8, 8, device=cuda)
    w = torch.ones(64, device=cuda)
    assert _hip.group_norm(x, w, w, 32, 1e-5) is None
    xb = torch.randn(1, 64, 3, 3, device=cuda).bfloat16()
    assert _hip.group_norm(xb, w.bfloat16(), w.bfloat16(), 32, 1e-5) is None
    assert _hip.geglu(torch.randn(4, 2560, device=cuda)) is None


def _module_errors(cuda, make, args_of, monkeypatch):
    """max |out - f32 module| of the fused and of the unfused bf16 module, and max |ref|."""
    torch.manual_seed(0)
    m32 = make().to(cuda).eval()
    m16 = make().to(cuda).eval()
    m16.load_state_dict(m32.state_dict())
    m16 = m16.to(torch.bfloat16)
    args = args_of(cuda)
    with torch.no_grad():
        ref = m32(*[t.float() for t in args])
        assert unet.fused_glue(args[0])
        fused = m16(*args)
        monkeypatch.setattr(unet, "FUSE_UNET", False)
        assert not unet.fused_glue(args[0])
        plain = m16(*args)
    e_f, e_p = (fused.float() - ref).abs().max().item(), (plain.float() - ref).abs().max().item()
    print(f"{type(m32).__name__}: fused err {e_f:.4e}, unfused err {e_p:.4e}, max|ref| {ref.abs().max().item():.3f}")
    assert e_f <= e_p + 2.0 ** -8 * ref.abs().max().item()


@pytest.mark.parametrize("cout", [128, 64])
def test_resnet_block_module(cuda, monkeypatch, cout):
    _module_errors(cuda, lambda: unet.ResnetBlock2D(64, cout, temb_ch=64),
                   lambda d: (rand((2, 64, 16, 16), torch.bfloat16, d, 31), rand((2, 64), torch.bfloat16, d, 32)),
                   monkeypatch)


def test_transformer_module(cuda, monkeypatch):
    _module_errors(cuda, lambda: unet.Transformer2DModel(8, 8, 64, context_dim=32),
                   lambda d: (rand((2, 64, 16, 16), torch.bfloat16, d, 33), rand((2, 5, 32), torch.bfloat16, d, 34)),
                   monkeypatch)


def test_fused_resnet_block_captures(cuda):
    """A fused forward captured on a side stream and replayed is bit-equal to the eager call.  MIOpen's
    default convolutions are not run-to-run reproducible (tools/determinism_probe.py), so, as in
    test_gpu_pipeline.py's bit-identity tests, the two convolutions run on PyTorch's native path."""
    torch.manual_seed(0)
    m = unet.ResnetBlock2D(64, 128, temb_ch=64).to(cuda, torch.bfloat16).eval()
    x, temb = rand((2, 64, 16, 16), torch.bfloat16, cuda, 41), rand((2, 64), torch.bfloat16, cuda, 42)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with torch.no_grad():
            assert unet.fused_glue(x, temb)
            eager = m(x, temb)
            side = torch.cuda.Stream(device=cuda)
            side.wait_stream(torch.cuda.current_stream(cuda))
            with torch.cuda.stream(side):
                m(x, temb)                                  # warm-up on the capture stream
            torch.cuda.current_stream(cuda).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                out = m(x, temb)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize(cuda)
            again = m(x, temb)
    finally:
        torch.backends.cudnn.enabled = det
    print(f"replay vs eager max |diff| {(out.float() - eager.float()).abs().max().item():.3e}; "
          f"eager vs eager {(again.float() - eager.float()).abs().max().item():.3e}")
    assert torch.equal(again, eager), "the eager forward is not reproducible: the comparison cannot tell anything"
    assert torch.equal(out, eager)
