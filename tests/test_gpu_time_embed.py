"""The U-Net's time path on the HIP kernels (csrc/p2p_unet.hip time_linear_kernel): p2p_time_embed
against the formula in f32 from the same 16-bit weights, p2p_time_proj against f32 W . silu(emb) + b
from the kernel's own emb, both within test_gpu_unet_glue.check's bar, and the model's wiring."""
import math

import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, unet
from test_gpu_unet_glue import check, rand

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
STEPS = [981, 1, 500, 0, 999, 250, 37, 764]
POISON = 6e4
# the 22 time_emb_proj widths of the SD-v1.4 U-Net, in module order
SD_WIDTHS = [320, 320, 640, 640, 1280, 1280, 1280, 1280, 1280, 1280,
             1280, 1280, 1280, 1280, 1280, 1280, 640, 640, 640, 320, 320, 320]


def bits(t):
    return t.view(torch.int16)


def sinusoid(t, dim):
    half = dim // 2
    f = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
    arg = t[:, None].float() * f[None, :]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("d_in,D", [(32, 128), (320, 1280)])
@pytest.mark.parametrize("N", [1, 3, 8])
def test_time_embed(cuda, N, d_in, D, dtype):
    t = torch.tensor(STEPS[:N], dtype=torch.int64, device=cuda)
    w1, b1 = rand((D, d_in), dtype, cuda, 1, d_in ** -0.5), rand((D,), dtype, cuda, 2, 0.1)
    w2, b2 = rand((D, D), dtype, cuda, 3, D ** -0.5), rand((D,), dtype, cuda, 4, 0.1)
    emb = _hip.time_embed(t, w1, b1, w2, b2)
    assert emb is not None and emb.shape == (N, D) and emb.dtype == dtype and emb.is_contiguous()
    s = sinusoid(t, d_in)
    ref = F.linear(F.silu(F.linear(s, w1.float(), b1.float())), w2.float(), b2.float())
    chain = F.linear(F.silu(F.linear(s.to(dtype), w1, b1)), w2, b2)
    check(emb, ref, dtype, f"time_embed N={N} {d_in}->{D} {dtype}", chain)
    assert torch.equal(bits(emb), bits(_hip.time_embed(t, w1, b1, w2, b2))), "two launches differ"
    # one timestep expanded to N rows (stride 0) is read as it is
    one = _hip.time_embed(t[:1].expand(N), w1, b1, w2, b2)
    assert torch.equal(bits(one), bits(emb[:1].expand(N, D).contiguous()))


def test_time_embed_unsupported_falls_back(cuda):
    t = torch.tensor([5], dtype=torch.int64, device=cuda)
    w = lambda *s: torch.randn(*s, device=cuda)          # noqa: E731
    assert _hip.time_embed(t, w(128, 32), w(128), w(128, 128), w(128)) is None                    # f32
    h = lambda *s: torch.randn(*s, device=cuda).bfloat16()   # noqa: E731
    assert _hip.time_embed(t, h(132, 32), h(132), h(132, 132), h(132)) is None                    # D % 8
    assert _hip.time_embed(t.int(), h(128, 32), h(128), h(128, 128), h(128)) is None              # int32 steps


def proj_case(cuda, dtype, widths, D, N, gaps):
    emb = rand((N, D), dtype, cuda, 11, 1.5)
    pairs = [(rand((c, D), dtype, cuda, 20 + 2 * r, D ** -0.5), rand((c,), dtype, cuda, 21 + 2 * r, 0.1))
             for r, c in enumerate(widths)]
    table = _hip.TimeProjTable(pairs, gaps=gaps or ())
    tail = 24
    arena = torch.full((N * table.row_elems + tail,), POISON, dtype=dtype, device=cuda)
    outs = _hip.time_proj(emb, table, out=arena[:N * table.row_elems])
    assert outs is not None and len(outs) == len(widths)
    act = F.silu(emb.float())
    written = torch.zeros(arena.numel(), dtype=torch.bool, device=cuda)
    for r, ((w, b), o, c) in enumerate(zip(pairs, outs, widths)):
        assert o.shape == (N, c) and o.is_contiguous() and o.dtype == dtype          # dense [N, C_r]
        ref = F.linear(act, w.float(), b.float())
        check(o, ref, dtype, f"time_proj segment {r} C={c} D={D} N={N} {dtype}", F.linear(F.silu(emb), w, b))
        first = (o.data_ptr() - arena.data_ptr()) // arena.element_size()
        written[first:first + N * c] = True
    # bytes between and behind the segments still hold the poison
    assert (~written).sum().item() == N * sum(gaps or [0]) + tail
    assert torch.equal(bits(arena[~written]), bits(torch.full(((~written).sum().item(),), POISON, dtype=dtype,
                                                               device=cuda)))
    again = torch.full_like(arena, POISON)
    _hip.time_proj(emb, table, out=again[:N * table.row_elems])
    assert torch.equal(bits(again), bits(arena)), "two launches on the same input differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [1, 3, 64])
def test_time_proj_small_segments(cuda, N, dtype):
    # widths below, at and above the 16-channel tile, with unwritten gaps in front of each output
    proj_case(cuda, dtype, [64, 8, 320, 64], 128, N, gaps=[0, 8, 3, 40])


@pytest.mark.parametrize("N", [1, 3, 64])
def test_time_proj_model_widths(cuda, N):
    proj_case(cuda, torch.bfloat16, SD_WIDTHS, 1280, N, gaps=None)


def small_unet():
    # (64, 128) with the default 8 heads: head dims 8 and 16, the smallest the attention kernels take
    return unet.UNet2DConditionModel(block_out_channels=(64, 128), layers_per_block=1, cross_attention_dim=32)


@pytest.fixture
def native_convs():
    """PyTorch's native convolutions: reproducible from call to call, which MIOpen's are not."""
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = det


def test_model_takes_the_fused_time_path(cuda, monkeypatch, native_convs):
    """Two fused forwards at different timesteps stay within the module bound of the unfused ones
    (fused err <= unfused err + 2^-8 max|ref|, the f32 model as reference); after the weights have
    moved to other buffers the segment table follows them, seen through the output."""
    torch.manual_seed(0)
    m32 = small_unet().to(cuda).eval()
    m16 = small_unet().to(cuda).eval()
    m16.load_state_dict(m32.state_dict())
    m16 = m16.to(torch.bfloat16)
    with torch.no_grad():       # a projection parameter that requires grad keeps the torch lines
        assert m16._time_path_fused(torch.tensor([3, 4], device=cuda)) is None
    m16.requires_grad_(False)   # as the pipelines load their models
    x = rand((2, 4, 16, 16), torch.bfloat16, cuda, 61)
    ctx = rand((2, 5, 32), torch.bfloat16, cuda, 62)
    steps = [torch.tensor(981, device=cuda), torch.tensor([1, 500], device=cuda)]
    with torch.no_grad():
        fused = []
        for t in steps:
            ref = m32(x.float(), t, ctx.float())["sample"]
            assert unet.fused_glue(x)
            f = m16(x, t, ctx)["sample"]
            assert isinstance(m16._time_path_fused(t.reshape(-1).expand(2)), unet.TimeProjections)
            monkeypatch.setattr(unet, "FUSE_UNET", False)
            p = m16(x, t, ctx)["sample"]
            monkeypatch.setattr(unet, "FUSE_UNET", True)
            e_f, e_p = (f.float() - ref).abs().max().item(), (p.float() - ref).abs().max().item()
            print(f"U-Net t={t.tolist()}: fused err {e_f:.4e}, unfused err {e_p:.4e}, max|ref| {ref.abs().max().item():.3f}")
            assert e_f <= e_p + 2.0 ** -8 * ref.abs().max().item()
            fused.append(f)
        assert not torch.equal(fused[0], fused[1])       # the timestep reaches the output
        # the weights move to new buffers.  A stale table would still read the old ones, kept alive
        # and overwritten here
        old_data = [p.data for p in m16.parameters()]
        for p in m16.parameters():
            p.data = p.data.clone()
        for buf in old_data:
            buf.fill_(float("nan"))
        moved = m16(x, steps[1], ctx)["sample"]
        assert torch.equal(moved, fused[1])
        assert isinstance(m16._time_path_fused(steps[1]), unet.TimeProjections)


def test_resnet_block_alone_is_unchanged(cuda, native_convs):
    """ResnetBlock2D called on its own with a plain [N, temb_ch] tensor: the fused block computes its
    own projection, as before -- the same bits as with that projection handed in from outside."""
    torch.manual_seed(0)
    m = unet.ResnetBlock2D(64, 128, temb_ch=64).to(cuda, torch.bfloat16).eval()
    x, temb = rand((2, 64, 16, 16), torch.bfloat16, cuda, 71), rand((2, 64), torch.bfloat16, cuda, 72)
    with torch.no_grad():
        assert unet.fused_glue(x, temb)
        own = m(x, temb)
        want = m._forward_fused(x, temb, m.time_emb_proj(F.silu(temb)))
        none = m(x, None)
    assert torch.equal(own, want)
    assert not torch.equal(own, none)
