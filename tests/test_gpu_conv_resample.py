"""conv3x3_kernel's Up2 and Down2 forms and its bias (csrc/p2p_conv.hip, p2p_conv3x3_ex) against F.conv2d
in f64 from the same 16-bit operands -- for Up2 of F.interpolate(scale_factor=2, mode="nearest") in
f64, for Down2 with stride=2, padding=1, the bias included where the case has one -- under the glue's
bar (test_gpu_unet_glue.check: u |ref| + u max|ref| 1e-2, u = 2^-8 for bf16, 2^-10 for f16: f32
accumulation and one rounding owe half an ulp, so the bar is derived, and no element is exempt);
torch's own 16-bit chain is measured against the same reference and printed beside it.  Sizes are
the INPUT map.  Every call writes into a sentinel-padded buffer, runs twice and must repeat its bits,
and the binding's own allocation gives the same bits.  The Same form through the new entry with a
null bias is bit-equal to p2p_conv3x3.  Then the Upsample2D / Downsample2D wiring: the switches,
capture with MIOpen left enabled, the packed-weight cache, and autograd with frozen parameters.
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
UP2, DOWN2, SAME = _hip.CONV_UP2, _hip.CONV_DOWN2, _hip.CONV_SAME

# (id, form, n, input h, input w, c_in, c_out, bias, must take the split path, the middle image is large)
CASES = [
    ("up2_two_images_one_tile", UP2, 3, 4, 4, 64, 64, True, False, True),
    ("up2_below_one_tile_cout_tail", UP2, 1, 4, 4, 64, 96, False, False, False),
    ("up2_odd_source", UP2, 2, 3, 4, 64, 64, False, False, False),
    ("up2_wide", UP2, 2, 4, 8, 64, 128, False, False, False),
    ("up2_tall", UP2, 2, 8, 4, 64, 128, False, False, False),
    ("up2_k_step_32", UP2, 2, 8, 8, 96, 320, True, False, False),
    ("up2_split_1280", UP2, 2, 4, 4, 1280, 1280, True, True, False),
    ("down2_two_images_one_tile", DOWN2, 3, 16, 16, 64, 64, True, False, True),
    ("down2_cout_tail", DOWN2, 1, 16, 16, 64, 96, False, False, False),
    ("down2_wide", DOWN2, 2, 16, 32, 64, 128, False, False, False),
    ("down2_tall", DOWN2, 2, 32, 16, 64, 128, False, False, False),
    ("down2_k_step_32", DOWN2, 2, 32, 32, 96, 320, False, False, False),
    ("down2_split_1280", DOWN2, 2, 16, 16, 1280, 1280, True, True, False),
]


def formula(x, wt, bias, form):
    """The module's lines in x's precision."""
    if form == UP2:
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, bias, 1, 1)
    return F.conv2d(x, wt, bias, 2 if form == DOWN2 else 1, 1)


@functools.lru_cache(maxsize=None)
def operands(dev, dtype, form, n, h, w, c_in, c_out, has_bias, spike):
    """(x NCHW, weight, bias, the f64 reference as f32, torch's own 16-bit chain): computed once per
    case and shared; nobody writes to them."""
    x = rand((n, c_in, h, w), dtype, dev, 61)
    if spike:
        x[1] *= 64.0          # a leak across the image boundary would show in images 0 and 2
    wt = rand((c_out, c_in, 3, 3), dtype, dev, 62, scale=(9 * c_in) ** -0.5)
    bias = rand((c_out,), dtype, dev, 63) if has_bias else None
    ref = formula(x.double(), wt.double(), None if bias is None else bias.double(), form).float()
    chain = formula(x, wt, bias, form)
    return x, wt, bias, ref, chain


def run_padded(x_tokens, packed, bias, form, n, h, w, c_out):
    """p2p_conv3x3_ex into the middle of a sentinel-filled buffer; returns (y, the whole buffer)."""
    dev, dtype = x_tokens.device, x_tokens.dtype
    oh, ow = _hip.conv3x3_out_map(form, h, w)
    numel = n * c_out * oh * ow
    buf = torch.full((numel + 2 * PAD,), 7.0, dtype=dtype, device=dev)
    y = buf[PAD:PAD + numel].view(n, c_out, oh, ow)
    a = _hip.Conv3x3ExArgs()
    a.x, a.weight, a.y = x_tokens.data_ptr(), packed.data_ptr(), y.data_ptr()
    if bias is not None:
        a.bias = bias.data_ptr()
    n_ws = int(_hip.lib().p2p_conv3x3_ex_workspace_floats(form, n, h, w, x_tokens.shape[2], c_out))
    assert n_ws >= 0, n_ws
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    a.workspace = ws.data_ptr()
    a.n, a.in_height, a.in_width, a.c_in, a.c_out = n, h, w, x_tokens.shape[2], c_out
    a.dtype, a.form = _hip._glue_dtype(x_tokens), form
    rc = _hip.lib().p2p_conv3x3_ex(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    return y, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_conv3x3_resample(cuda, dtype, case):
    name, form, n, h, w, c_in, c_out, has_bias, splits, spike = case
    split = _hip.conv3x3_ex_split(form, n, h, w, c_in, c_out)
    assert split > 1 if splits else split >= 1, split
    x, wt, bias, ref, chain = operands(cuda, dtype, form, n, h, w, c_in, c_out, has_bias, spike)
    tokens = x.permute(0, 2, 3, 1).reshape(n, h * w, c_in).contiguous()
    packed = _hip.conv3x3_pack(wt)
    assert packed is not None
    y, buf = run_padded(tokens, packed, bias, form, n, h, w, c_out)
    y2, _ = run_padded(tokens, packed, bias, form, n, h, w, c_out)
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(buf[:PAD], torch.full_like(buf[:PAD], 7.0)) and torch.equal(buf[-PAD:], torch.full_like(buf[-PAD:], 7.0))
    assert torch.equal(y, y2), "two launches on the same operands differ"
    if spike:   # per image: the small images' bar must not be hidden behind the large one's max |ref|
        for i in range(n):
            check(y[i], ref[i], dtype, f"conv3x3_ex {name} image {i} {dtype}", chain[i])
    else:
        check(y, ref, dtype, f"conv3x3_ex {name} {dtype} (K = {9 * c_in}, split {split})", chain)
    # the binding allocates its own output and workspace: the same bits
    fn = _hip.conv3x3_up2 if form == UP2 else _hip.conv3x3_down2
    assert torch.equal(fn(tokens, packed, bias, h, w), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(3, 8, 8, 64, 64), (2, 8, 8, 1280, 1280)], ids=["one_launch", "split"])
def test_same_form_through_the_new_entry_has_the_old_bits(cuda, dtype, shape):
    n, h, w, c_in, c_out = shape
    x = rand((n, c_in, h, w), dtype, cuda, 51)
    wt = rand((c_out, c_in, 3, 3), dtype, cuda, 52, scale=(9 * c_in) ** -0.5)
    tokens = x.permute(0, 2, 3, 1).reshape(n, h * w, c_in).contiguous()
    packed = _hip.conv3x3_pack(wt)
    assert _hip.conv3x3_ex_split(SAME, n, h, w, c_in, c_out) == _hip.conv3x3_split(n, h, w, c_in, c_out)
    old = _hip.conv3x3(tokens, packed, h, w)
    new, buf = run_padded(tokens, packed, None, SAME, n, h, w, c_out)
    assert old is not None and torch.equal(new, old)
    assert torch.equal(buf[:PAD], torch.full_like(buf[:PAD], 7.0)) and torch.equal(buf[-PAD:], torch.full_like(buf[-PAD:], 7.0))


# ---------------------------------------------------------------------------- the modules
MODULES = [("up", unet.Upsample2D, (2, 64, 8, 8)), ("down", unet.Downsample2D, (2, 64, 16, 16))]


def _module(cuda, cls, shape, flag=True, dtype=torch.bfloat16, seed=0):
    torch.manual_seed(seed)
    m = cls(shape[1], conv_hip=flag).to(cuda, dtype).eval()
    return m, rand(shape, dtype, cuda, 41)


@pytest.fixture
def calls(monkeypatch):
    n = []
    real = _hip.conv3x3_ex
    monkeypatch.setattr(_hip, "conv3x3_ex", lambda *a, **k: n.append(a[-1]) or real(*a, **k))
    return n


@pytest.mark.parametrize("which", MODULES, ids=lambda m: m[0])
def test_module_takes_the_kernel(cuda, monkeypatch, calls, which):
    """The kernel runs when the switch is on; not with CONV_HIP off, for a module built without the
    flag (the VAE's), or in f32."""
    _, cls, shape = which
    m, x = _module(cuda, cls, shape)
    form = UP2 if cls is unet.Upsample2D else DOWN2
    with torch.no_grad():
        m(x)
        assert calls == [form]
        plain, _ = _module(cuda, cls, shape, flag=False)
        plain(x)
        m32, _ = _module(cuda, cls, shape, dtype=torch.float32)
        m32(x.float())
        monkeypatch.setattr(unet, "CONV_HIP", False)
        m(x)
        assert calls == [form]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("which", MODULES, ids=lambda m: m[0])
def test_module_within_the_bar_of_the_f64_formula(cuda, calls, dtype, which):
    _, cls, shape = which
    m, _ = _module(cuda, cls, shape, dtype=dtype)
    x = rand(shape, dtype, cuda, 41)
    form = UP2 if cls is unet.Upsample2D else DOWN2
    with torch.no_grad():
        y = m(x)
        ref = formula(x.double(), m.conv.weight.double(), m.conv.bias.double(), form).float()
        chain = formula(x, m.conv.weight, m.conv.bias, form)
    assert calls == [form]
    check(y, ref, dtype, f"{cls.__name__} {dtype}", chain)


@pytest.mark.parametrize("which", MODULES, ids=lambda m: m[0])
def test_module_captures_with_miopen_enabled(cuda, calls, which):
    """Captured and replayed with cudnn (MIOpen) left enabled: bit-equal to the eager call."""
    _, cls, shape = which
    m, x = _module(cuda, cls, shape)
    assert torch.backends.cudnn.enabled
    with torch.no_grad():
        eager = m(x)
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream(cuda).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m(x)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(cuda)
    assert len(calls) == 3
    assert torch.equal(out, eager)


@pytest.mark.parametrize("which", MODULES, ids=lambda m: m[0])
def test_module_cache_miss_under_capture_falls_back(cuda, monkeypatch, calls, which):
    """A weight that was never packed meets its first fused call under capture: the module's own
    lines run, nothing is packed, and the result still matches."""
    _, cls, shape = which
    m, x = _module(cuda, cls, shape)
    with torch.no_grad():
        monkeypatch.setattr(unet, "CONV_HIP", False)
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            want = m(x)                        # warms MIOpen up; packs nothing
        torch.cuda.current_stream(cuda).wait_stream(side)
        monkeypatch.setattr(unet, "CONV_HIP", True)
        packs = []
        real = _hip.conv3x3_pack
        monkeypatch.setattr(_hip, "conv3x3_pack", lambda w: packs.append(w.shape) or real(w))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = m(x)
        graph.replay()
        torch.cuda.synchronize(cuda)
        assert not packs and not calls and m.conv not in _hip.CONV_WEIGHTS._packed
        assert (out.float() - want.float()).abs().max().item() <= 2.0 ** -7 * want.float().abs().max().item()
        m(x)                                   # eager again: now it packs and takes the kernel
        assert len(packs) == 1 and len(calls) == 1


def rel_l2(a, ref):
    return ((a.double() - ref.double()).norm() / ref.double().norm()).item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("which", MODULES, ids=lambda m: m[0])
def test_module_under_autograd_with_frozen_parameters(cuda, monkeypatch, calls, dtype, which):
    """The forward bits are the no-grad forward's; the input gradient against the f32 module is within
    the bar of test_gpu_unet_grad_modules: at most twice the relative L2 error of the torch lines."""
    _, cls, shape = which
    torch.manual_seed(0)
    m32 = cls(shape[1], conv_hip=True).to(cuda).eval().requires_grad_(False)
    m16 = copy.deepcopy(m32).to(dtype)
    x = rand(shape, dtype, cuda, 52)

    def grad_of(m, cast):
        leaf = cast(x).detach().requires_grad_(True)
        out = m(leaf)
        dy = rand(tuple(out.shape), dtype, cuda, 77)
        out.backward(cast(dy))
        return out.detach(), leaf.grad

    _, ref = grad_of(m32, lambda t: t.float())
    assert not calls
    with torch.no_grad():
        inference = m16(x)
    out, fused = grad_of(m16, lambda t: t)
    assert len(calls) == 2, "the kernel did not run under autograd"
    assert torch.equal(out, inference), "the forward under autograd differs from the no-grad forward"
    monkeypatch.setattr(unet, "FUSE_UNET_GRAD", False)
    _, plain = grad_of(m16, lambda t: t)
    assert len(calls) == 2
    e_f, e_p = rel_l2(fused, ref), rel_l2(plain, ref)
    print(f"{cls.__name__} {dtype}: relative L2 error of the input gradient: kernel path {e_f:.4e}, torch lines {e_p:.4e}")
    assert torch.isfinite(fused).all() and fused.dtype == dtype and fused.shape == x.shape
    assert e_f <= 2 * e_p


@pytest.mark.parametrize("which", MODULES, ids=lambda m: m[0])
def test_module_with_trainable_weight_runs_the_torch_lines(cuda, calls, which):
    _, cls, shape = which
    m, x = _module(cuda, cls, shape)
    m.conv.weight.requires_grad_(True)
    m.conv.bias.requires_grad_(False)
    with torch.enable_grad():
        y = m(x.clone().requires_grad_(True))
        y.float().square().mean().backward()
    assert not calls and m.conv.weight.grad is not None
