"""conv3x3_pipe_kernel (csrc/p2p_conv.hip on csrc/p2p_mma_pipe.h): the global_load_lds ring forms of
the 3x3 convolution, forced through p2p_conv3x3_set_loop, against the register-staged loop -- the bits
must be equal -- and against F.conv2d in f64 from the same 16-bit operands under the glue's bar
(test_gpu_unet_glue.check: u |ref| + u max|ref| 1e-2, u = 2^-8 for bf16, 2^-10 for f16).  Every plan
here is 64 channels a step and 160 output channels a tile, the only tile the ring is built for.  The
shapes are the smallest at which this loop can go wrong: a full 256-row tile plus a 64-row tail with
four images in one tile, M below any tile, h != w with two column tiles, an odd step count above the
ring's depth, a K split into ranges of 10 and 11 steps (the ring's prologue and drain meet even and
odd counts), and the Up2 / Down2 source addressing with a bias.  Every call writes into a sentinel-
padded buffer, runs twice and must repeat its bits.  Sizes of the Up2 / Down2 cases are the INPUT map.
Every compiled instantiation at a small shape: tests/kernel_matrix.py (a kernel change extends that table)."""
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
SAME, UP2, DOWN2 = _hip.CONV_SAME, _hip.CONV_UP2, _hip.CONV_DOWN2
AUTO, TILE, PIPE128, PIPE256 = _hip.CONV_LOOP_AUTO, _hip.CONV_LOOP_TILE, _hip.CONV_LOOP_PIPE128, _hip.CONV_LOOP_PIPE256
PIPES = [PIPE128, PIPE256]

# (id, form, n, input h, input w, c_in, c_out, bias, split, the image scaled x 64 or None)
CASES = [
    ("tile_and_tail_four_images", SAME, 5, 8, 8, 64, 160, False, 1, 2),
    ("below_any_tile", SAME, 1, 8, 8, 64, 160, False, 1, None),
    ("wide_two_column_tiles", SAME, 2, 8, 16, 128, 320, False, 2, None),
    ("tall_two_column_tiles", SAME, 2, 16, 8, 128, 320, False, 2, None),
    ("split_8_of_81_steps", SAME, 1, 8, 8, 576, 160, False, 8, None),
    ("up2_bias", UP2, 2, 4, 4, 64, 160, True, 1, None),
    ("down2_bias", DOWN2, 2, 16, 16, 64, 160, True, 1, None),
]


def formula(x, wt, bias, form):
    if form == UP2:
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, bias, 1, 1)
    return F.conv2d(x, wt, bias, 2 if form == DOWN2 else 1, 1)


@functools.lru_cache(maxsize=None)
def operands(dev, dtype, form, n, h, w, c_in, c_out, has_bias, spike):
    """(token-major x, packed weight, bias, the f64 reference as f32, torch's own 16-bit chain): computed
    once per case and shared; nobody writes to them."""
    x = rand((n, c_in, h, w), dtype, dev, 71)
    if spike is not None:
        x[spike] *= 64.0      # a leak across an image boundary would show in the neighbours
    wt = rand((c_out, c_in, 3, 3), dtype, dev, 72, scale=(9 * c_in) ** -0.5)
    bias = rand((c_out,), dtype, dev, 73) if has_bias else None
    ref = formula(x.double(), wt.double(), None if bias is None else bias.double(), form).float()
    chain = formula(x, wt, bias, form)
    tokens = x.permute(0, 2, 3, 1).reshape(n, h * w, c_in).contiguous()
    packed = _hip.conv3x3_pack(wt)
    assert packed is not None
    return tokens, packed, bias, ref, chain


def run_padded(x_tokens, packed, bias, form, n, h, w, c_out):
    """p2p_conv3x3 (Same, no bias) or p2p_conv3x3_ex into the middle of a sentinel-filled buffer;
    returns (y, the whole buffer)."""
    dev, dtype = x_tokens.device, x_tokens.dtype
    oh, ow = _hip.conv3x3_out_map(form, h, w)
    numel = n * c_out * oh * ow
    buf = torch.full((numel + 2 * PAD,), 7.0, dtype=dtype, device=dev)
    y = buf[PAD:PAD + numel].view(n, c_out, oh, ow)
    c_in = x_tokens.shape[2]
    n_ws = int(_hip.lib().p2p_conv3x3_ex_workspace_floats(form, n, h, w, c_in, c_out))
    assert n_ws >= 0, n_ws
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if form == SAME and bias is None:
        a = _hip.Conv3x3Args()
        a.n, a.height, a.width, a.c_in, a.c_out = n, h, w, c_in, c_out
        entry = _hip.lib().p2p_conv3x3
    else:
        a = _hip.Conv3x3ExArgs()
        a.n, a.in_height, a.in_width, a.c_in, a.c_out, a.form = n, h, w, c_in, c_out, form
        if bias is not None:
            a.bias = bias.data_ptr()
        entry = _hip.lib().p2p_conv3x3_ex
    a.x, a.weight, a.y, a.workspace = x_tokens.data_ptr(), packed.data_ptr(), y.data_ptr(), ws.data_ptr()
    a.dtype = _hip._glue_dtype(x_tokens)
    rc = entry(ctypes.byref(a), stream)
    assert rc == 0, rc
    return y, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("loop", PIPES, ids=["pipe128", "pipe256"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_conv3x3_pipe(cuda, dtype, loop, case):
    name, form, n, h, w, c_in, c_out, has_bias, want_split, spike = case
    assert _hip.conv3x3_ex_split(form, n, h, w, c_in, c_out) == want_split
    tokens, packed, bias, ref, chain = operands(cuda, dtype, form, n, h, w, c_in, c_out, has_bias, spike)
    try:
        _hip.conv3x3_set_loop(loop)
        y, buf = run_padded(tokens, packed, bias, form, n, h, w, c_out)
        y2, _ = run_padded(tokens, packed, bias, form, n, h, w, c_out)
        _hip.conv3x3_set_loop(TILE)
        old, _ = run_padded(tokens, packed, bias, form, n, h, w, c_out)
    finally:
        _hip.conv3x3_set_loop(AUTO)
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(buf[:PAD], torch.full_like(buf[:PAD], 7.0)) and torch.equal(buf[-PAD:], torch.full_like(buf[-PAD:], 7.0))
    assert torch.equal(y, y2), "two launches on the same operands differ"
    assert torch.equal(y, old), "the ring's bits are not the register-staged loop's"
    if spike is not None:   # per image: the small images' bar must not be hidden behind the large one's max |ref|
        for i in range(n):
            check(y[i], ref[i], dtype, f"conv3x3 pipe {loop} {name} image {i} {dtype}", chain[i])
    else:
        check(y, ref, dtype, f"conv3x3 pipe {loop} {name} {dtype} (K = {9 * c_in}, split {want_split})", chain)


def test_resnet_block_has_the_same_bits_under_every_loop(cuda):
    """ResnetBlock2D(64, 160) at 2 x 16 x 16 (conv1 takes the bk = 64, bn = 160 plan): equal bits under
    the selection's choice, the register-staged loop and both forced ring forms, eager and from a
    captured graph (the switch is set before the capture, never under it)."""
    torch.manual_seed(0)
    m = unet.ResnetBlock2D(64, 160, temb_ch=64).to(cuda, torch.bfloat16).eval()
    x, temb = rand((2, 64, 16, 16), torch.bfloat16, cuda, 41), rand((2, 64), torch.bfloat16, cuda, 42)
    outs = {}
    try:
        with torch.no_grad():
            for loop in (TILE, AUTO, PIPE128, PIPE256):
                _hip.conv3x3_set_loop(loop)
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
                outs[loop] = (eager, out.clone())
                del graph
    finally:
        _hip.conv3x3_set_loop(AUTO)
    want = outs[TILE][0]
    assert torch.isfinite(want.float()).all() and want.float().abs().max().item() > 0
    for loop, (eager, replayed) in outs.items():
        assert torch.equal(eager, want), f"loop {loop}, eager"
        assert torch.equal(replayed, want), f"loop {loop}, captured"
