"""p2p_layer_norm at the U-Net's widths -- the grouped row mappings of csrc/p2p_text.hip (8 lanes per
row up to 320 channels, 16 up to 640, a wave above; 256 threads per workgroup: 32, 16 or 4 rows) --
and BasicTransformerBlock's fused path on it.  The kernel bar is test_gpu_unet_glue.check's, against
F.layer_norm in f32 from the rounded sum; sum_out holds exactly that sum."""
import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, unet
from test_gpu_unet_glue import _module_errors, check, rand

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
POISON = 6e4
# the issue's shapes, then the edges of each mapping: rows per wave (8 / 4 / 1) and per workgroup
# (32 / 16 / 4) minus one, exactly, plus one; the widths where the mapping switches (320 | 328,
# 640 | 648) and a width that leaves the last vector of a group's sweep to some lanes only (72)
SHAPES = [(1, 320), (37, 320), (4099, 320), (130, 640), (67, 1280), (5, 64),
          (7, 320), (8, 320), (9, 320), (31, 320), (32, 320), (33, 320),
          (3, 640), (4, 640), (5, 640), (15, 640), (16, 640), (17, 640),
          (3, 1280), (4, 1280), (5, 1280),
          (33, 328), (17, 648), (33, 72)]


def bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", ["plain", "add", "add+bias+sum", "alias"])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_layer_norm_unet_widths(cuda, rows, C, mode, dtype, eps=1e-5):
    extra = 3                                          # rows behind the tensor, poisoned
    def buf(seed, scale=1.0, shift=0.0):
        b = torch.full((rows + extra, C), POISON, dtype=dtype, device=cuda)
        b[:rows] = rand((rows, C), dtype, cuda, seed, scale, shift)
        return b

    xb = buf(1, 2.0, 0.5)
    x = xb[:rows]
    gamma, beta = rand((C,), dtype, cuda, 2, 0.5, 1.0), rand((C,), dtype, cuda, 3)
    add = rand((rows, C), dtype, cuda, 4) if mode != "plain" else None
    bias = rand((C,), dtype, cuda, 5) if mode in ("add+bias+sum", "alias") else None
    x_in_b = xb.clone()
    x_in = x_in_b[:rows]
    sum_b = torch.full((rows + extra, C), POISON, dtype=dtype, device=cuda)
    sum_out = {"plain": None, "add": None, "add+bias+sum": sum_b[:rows], "alias": x_in}[mode]
    s = x.float()
    if add is not None:
        s = s + add.float()
    if bias is not None:
        s = s + bias.float()
    s = s.to(dtype)                                    # the rounded sum: what LayerNorm normalises
    ref = F.layer_norm(s.float(), (C,), gamma.float(), beta.float(), eps)
    chain = F.layer_norm(s, (C,), gamma, beta, eps)

    def run():
        return _hip.layer_norm(x_in, gamma, beta, eps, add=add, add_bias=bias, sum_out=sum_out)

    y = run()
    assert y is not None and y.shape == x.shape and y.dtype == dtype
    check(y, ref, dtype, f"layer_norm {rows}x{C} {mode} {dtype}", chain)
    if sum_out is not None:
        assert torch.equal(bits(sum_out), bits(s))
    # the rows behind the tensors still hold the poison
    for b in (x_in_b, sum_b):
        assert torch.equal(bits(b[rows:]), bits(torch.full((extra, C), POISON, dtype=dtype, device=cuda)))
    if mode != "alias":                                # (in place, a second launch adds again)
        assert torch.equal(bits(x_in), bits(x))
        assert torch.equal(bits(run()), bits(y)), "two launches on the same input differ"
    else:
        x_in.copy_(x)
        assert torch.equal(bits(run()), bits(y)) and torch.equal(bits(x_in), bits(s))


def test_output_rows_beyond_the_tensor_stay(cuda):
    """y is the binding's own allocation, so the poison check on it goes through the C entry point:
    y is the head of a larger buffer."""
    import ctypes
    for rows, C in [(37, 320), (130, 640), (67, 1280)]:
        x = rand((rows, C), torch.bfloat16, cuda, 1)
        g, b = rand((C,), torch.bfloat16, cuda, 2), rand((C,), torch.bfloat16, cuda, 3)
        yb = torch.full((rows + 3, C), POISON, dtype=torch.bfloat16, device=cuda)
        a = _hip.LayerNormArgs()
        a.x, a.gamma, a.beta, a.y = x.data_ptr(), g.data_ptr(), b.data_ptr(), yb.data_ptr()
        a.rows, a.channels, a.eps, a.dtype = rows, C, 1e-5, _hip.P2P_DTYPE_BF16
        assert _hip.lib().p2p_layer_norm(ctypes.byref(a), torch.cuda.current_stream(cuda).cuda_stream) == 0
        torch.cuda.synchronize(cuda)
        assert torch.equal(bits(yb[:rows]), bits(_hip.layer_norm(x, g, b, 1e-5)))
        assert torch.equal(bits(yb[rows:]), bits(torch.full((3, C), POISON, dtype=torch.bfloat16, device=cuda)))


@pytest.mark.parametrize("dim,heads,d_head,ctx_dim,ctx_len", [(64, 8, 8, 32, 5), (320, 8, 40, 768, 77)])
def test_transformer_block_module(cuda, monkeypatch, dim, heads, d_head, ctx_dim, ctx_len):
    _module_errors(cuda, lambda: unet.BasicTransformerBlock(dim, heads, d_head, ctx_dim),
                   lambda d: (rand((2, 64, dim), torch.bfloat16, d, 51), rand((2, ctx_len, ctx_dim), torch.bfloat16, d, 52)),
                   monkeypatch)


def test_fused_block_leaves_its_input(cuda):
    torch.manual_seed(0)
    m = unet.BasicTransformerBlock(64, 8, 8, 32).to(cuda, torch.bfloat16).eval()
    x, ctx = rand((2, 64, 64), torch.bfloat16, cuda, 53), rand((2, 5, 32), torch.bfloat16, cuda, 54)
    keep = x.clone()
    with torch.no_grad():
        assert unet.fused_glue(x, m.norm1.weight)
        m(x, ctx)
    assert torch.equal(bits(x), bits(keep))


def test_fused_block_captures(cuda):
    """One fused block (the unpatched attention: the plain HIP path) captured on a side stream and
    replayed is bit-equal to the eager call."""
    torch.manual_seed(0)
    m = unet.BasicTransformerBlock(320, 8, 40, 768).to(cuda, torch.bfloat16).eval()
    x, ctx = rand((2, 64, 320), torch.bfloat16, cuda, 55), rand((2, 77, 768), torch.bfloat16, cuda, 56)
    with torch.no_grad():
        assert unet.fused_glue(x, m.norm1.weight)
        eager = m(x, ctx)
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
        again = m(x, ctx)
    assert torch.equal(again, eager), "the eager forward is not reproducible: the comparison cannot tell anything"
    assert torch.equal(out, eager)


def test_fused_block_under_autograd(cuda, monkeypatch):
    """Under autograd the block runs the same forward (the no-grad bits) and torch's own LayerNorm
    gradient at the stored sum: the input gradient is as close to the f32 block's as the torch
    lines' is (within a factor 2 of their relative L2 error, the bar of test_gpu_unet_grad_modules)."""
    torch.manual_seed(0)
    m32 = unet.BasicTransformerBlock(64, 8, 8, 32).to(cuda).eval().requires_grad_(False)
    m16 = unet.BasicTransformerBlock(64, 8, 8, 32).to(cuda).eval().requires_grad_(False)
    m16.load_state_dict(m32.state_dict())
    m16 = m16.to(torch.bfloat16)
    for m in (m32, m16):        # the norms and adds alone (the attention backward has its own tests)
        m.attn1.forward = m.attn2.forward = lambda y, context=None: y
    x, ctx = rand((2, 64, 64), torch.bfloat16, cuda, 57), rand((2, 5, 32), torch.bfloat16, cuda, 58)
    dy = rand((2, 64, 64), torch.bfloat16, cuda, 59)

    def grad_of(m, cast):
        leaf = cast(x).detach().requires_grad_(True)
        out = m(leaf, cast(ctx))
        out.backward(cast(dy))
        return out.detach(), leaf.grad

    _, ref = grad_of(m32, lambda t: t.float())
    with torch.no_grad():
        inference = m16(x, ctx)
    assert unet.fused_glue_grad(x)
    out, fused = grad_of(m16, lambda t: t)
    assert torch.equal(bits(out), bits(inference)), "the forward under autograd differs from the no-grad forward"
    monkeypatch.setattr(unet, "FUSE_UNET_GRAD", False)
    _, plain = grad_of(m16, lambda t: t)
    rel = lambda a: ((a.double() - ref.double()).norm() / ref.double().norm()).item()   # noqa: E731
    print(f"BasicTransformerBlock input gradient, relative L2 error: fused {rel(fused):.4e}, torch lines {rel(plain):.4e}")
    assert torch.isfinite(fused).all() and rel(fused) <= 2 * rel(plain)
