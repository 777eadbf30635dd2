"""conv3x3_kernel (csrc/p2p_conv.hip) against F.conv2d in f64 from the same 16-bit operands, under the
glue's bar (test_gpu_unet_glue.check: u |ref| + u max|ref| 1e-2, u = 2^-8 for bf16, 2^-10 for f16:
f32 accumulation and one rounding owe half an ulp); torch's own 16-bit convolution is measured
against the same reference and printed beside it.  The shapes are the smallest at which the kernel
can go wrong: two images in one 128-pixel tile, M below a tile, h != w, a c_out tail, a K step of
32, and the two largest K, which must take the split path.  Every call writes into a sentinel-
padded buffer, runs twice and must repeat its bits.  Then the ResnetBlock2D wiring: capture with
MIOpen left enabled, the P2P_CONV switch, and the packed-weight cache.
Every compiled instantiation at a small shape: tests/kernel_matrix.py (a kernel change extends that table)."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, unet

from test_gpu_unet_glue import check, rand

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
PAD = 256   # sentinel elements before and after y

# (id, n, h, w, c_in, c_out, must take the split path, the middle image is large)
CASES = [
    ("two_images_one_tile", 3, 8, 8, 64, 64, False, True),
    ("below_one_tile_cout_tail", 1, 8, 8, 64, 96, False, False),
    ("wide", 2, 8, 16, 64, 128, False, False),
    ("tall", 2, 16, 8, 64, 128, False, False),
    ("k_step_32_cout_320", 2, 16, 16, 96, 320, False, False),
    ("split_8x8_1280", 2, 8, 8, 1280, 1280, True, False),
    ("split_16x16_2560", 1, 16, 16, 2560, 1280, True, False),
]


@functools.lru_cache(maxsize=None)
def operands(dev, dtype, n, h, w, c_in, c_out, spike):
    """(x NCHW, weight, the f64 reference as f32, torch's own 16-bit convolution): computed once per
    case and shared; nobody writes to them."""
    x = rand((n, c_in, h, w), dtype, dev, 51)
    if spike:
        x[1] *= 64.0          # a leak across the image boundary would show in images 0 and 2
    wt = rand((c_out, c_in, 3, 3), dtype, dev, 52, scale=(9 * c_in) ** -0.5)
    ref = F.conv2d(x.double(), wt.double(), None, 1, 1).float()
    chain = F.conv2d(x, wt, None, 1, 1)
    return x, wt, ref, chain


def run_padded(x_tokens, packed, n, h, w, c_out):
    """p2p_conv3x3 into the middle of a sentinel-filled buffer; returns (y, the whole buffer)."""
    dev, dtype = x_tokens.device, x_tokens.dtype
    numel = n * c_out * h * w
    buf = torch.full((numel + 2 * PAD,), 7.0, dtype=dtype, device=dev)
    y = buf[PAD:PAD + numel].view(n, c_out, h, w)
    a = _hip.Conv3x3Args()
    a.x, a.weight, a.y = x_tokens.data_ptr(), packed.data_ptr(), y.data_ptr()
    n_ws = int(_hip.lib().p2p_conv3x3_workspace_floats(n, h, w, x_tokens.shape[2], c_out))
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    a.workspace = ws.data_ptr()
    a.n, a.height, a.width, a.c_in, a.c_out = n, h, w, x_tokens.shape[2], c_out
    a.dtype = _hip._glue_dtype(x_tokens)
    rc = _hip.lib().p2p_conv3x3(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    return y, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_conv3x3(cuda, dtype, case):
    name, n, h, w, c_in, c_out, splits, spike = case
    split = _hip.conv3x3_split(n, h, w, c_in, c_out)
    assert split > 1 if splits else split >= 1, split
    x, wt, ref, chain = operands(cuda, dtype, n, h, w, c_in, c_out, spike)
    tokens = x.permute(0, 2, 3, 1).reshape(n, h * w, c_in).contiguous()
    packed = _hip.conv3x3_pack(wt)
    assert packed is not None and torch.equal(packed, wt.permute(2, 3, 0, 1).reshape(9, c_out, c_in))
    y, buf = run_padded(tokens, packed, n, h, w, c_out)
    y2, _ = run_padded(tokens, packed, n, h, w, c_out)
    assert torch.equal(buf[:PAD], torch.full_like(buf[:PAD], 7.0)) and torch.equal(buf[-PAD:], torch.full_like(buf[-PAD:], 7.0))
    assert torch.equal(y, y2), "two launches on the same operands differ"
    if spike:   # per image: the small images' bar must not be hidden behind the large one's max |ref|
        for i in range(n):
            check(y[i], ref[i], dtype, f"conv3x3 {name} image {i} {dtype}", chain[i])
    else:
        check(y, ref, dtype, f"conv3x3 {name} {dtype} (K = {9 * c_in}, split {split})", chain)
    # the binding allocates its own output and workspace: the same bits
    assert torch.equal(_hip.conv3x3(tokens, packed, h, w), y)


def _block(cuda, seed=0):
    torch.manual_seed(seed)
    m = unet.ResnetBlock2D(64, 128, temb_ch=64).to(cuda, torch.bfloat16).eval()
    return m, rand((2, 64, 16, 16), torch.bfloat16, cuda, 41), rand((2, 64), torch.bfloat16, cuda, 42)


def test_resnet_block_takes_the_kernel(cuda, monkeypatch):
    """Both convolutions of the block go through p2p_conv3x3 when the switch is on, none when it is off."""
    m, x, temb = _block(cuda)
    calls = []
    real = _hip.conv3x3
    monkeypatch.setattr(_hip, "conv3x3", lambda *a, **k: calls.append(a[1].shape) or real(*a, **k))
    with torch.no_grad():
        m(x, temb)
        assert [tuple(s) for s in calls] == [(9, 128, 64), (9, 128, 128)]
        monkeypatch.setattr(unet, "CONV_HIP", False)
        m(x, temb)
        assert len(calls) == 2


def test_resnet_block_captures_with_miopen_enabled(cuda):
    """The fused forward captured and replayed is bit-equal to the eager call with cudnn (MIOpen) left
    enabled: the two 3x3 convolutions no longer depend on MIOpen's atomics."""
    m, x, temb = _block(cuda)
    assert torch.backends.cudnn.enabled
    with torch.no_grad():
        eager = m(x, temb)
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            m(x, temb)
        torch.cuda.current_stream(cuda).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m(x, temb)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(cuda)
        again = m(x, temb)
    assert torch.equal(again, eager)
    assert torch.equal(out, eager)


def test_resnet_block_switch_both_within_the_module_bar(cuda, monkeypatch):
    """P2P_CONV on and off against the f32 module: each within test_gpu_unet_glue's module bar (the
    unfused 16-bit module's error plus one bf16 ulp of max |ref|)."""
    torch.manual_seed(0)
    m32 = unet.ResnetBlock2D(64, 128, temb_ch=64).to(cuda).eval()
    m16 = copy.deepcopy(m32).to(torch.bfloat16)
    x, temb = rand((2, 64, 16, 16), torch.bfloat16, cuda, 31), rand((2, 64), torch.bfloat16, cuda, 32)
    with torch.no_grad():
        ref = m32(x.float(), temb.float())
        on = m16(x, temb)
        monkeypatch.setattr(unet, "CONV_HIP", False)
        off = m16(x, temb)
        monkeypatch.setattr(unet, "FUSE_UNET", False)
        plain = m16(x, temb)
    e_on, e_off, e_p = ((t.float() - ref).abs().max().item() for t in (on, off, plain))
    top = ref.abs().max().item()
    print(f"ResnetBlock2D: P2P_CONV on err {e_on:.4e}, off err {e_off:.4e}, unfused err {e_p:.4e}, max|ref| {top:.3f}")
    assert e_on <= e_p + 2.0 ** -8 * top and e_off <= e_p + 2.0 ** -8 * top


def test_packed_weights_follow_an_in_place_change(cuda):
    m, x, temb = _block(cuda)
    with torch.no_grad():
        before = m(x, temb)
        m.conv1.weight.mul_(-0.5)
        after = m(x, temb)
        fresh = copy.deepcopy(m)            # new modules: packed from the changed weights
        assert torch.equal(after, fresh(x, temb))
    assert not torch.equal(after, before)


def test_cache_miss_under_capture_falls_back(cuda, monkeypatch):
    """A convolution whose weights were never packed meets its first fused call under graph capture:
    that call runs MIOpen's convolution and packs nothing."""
    m, x, temb = _block(cuda)
    with torch.no_grad():
        monkeypatch.setattr(unet, "CONV_HIP", False)
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            want = m(x, temb)                  # warms MIOpen up; packs nothing
        torch.cuda.current_stream(cuda).wait_stream(side)
        monkeypatch.setattr(unet, "CONV_HIP", True)
        packs = []
        real = _hip.conv3x3_pack
        monkeypatch.setattr(_hip, "conv3x3_pack", lambda w: packs.append(w.shape) or real(w))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m(x, temb)
        graph.replay()
        torch.cuda.synchronize(cuda)
        assert not packs and m.conv1 not in _hip.CONV_WEIGHTS._packed and m.conv2 not in _hip.CONV_WEIGHTS._packed
        assert (out.float() - want.float()).abs().max().item() <= 2.0 ** -7 * want.float().abs().max().item()
        m(x, temb)                             # eager again: now it packs
        assert len(packs) == 2


def test_autograd_forward_has_the_no_grad_bits(cuda):
    """The forward under autograd (fused_glue_grad) runs the same kernel: the bits of the no-grad
    forward, and a gradient for x."""
    m, x, temb = _block(cuda)
    for p in m.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        want = m(x, temb)
    xg = x.clone().requires_grad_(True)
    with torch.enable_grad():
        got = m(xg, temb)
        got.float().square().mean().backward()
    assert torch.equal(got.detach(), want)
    assert xg.grad is not None and torch.isfinite(xg.grad).all() and xg.grad.abs().max().item() > 0
