"""Every row of tests/kernel_matrix.py's CONV_ROWS -- every instantiation of conv3x3_kernel and
conv3x3_pipe_kernel (csrc/p2p_conv.hip) and both bias states of conv3x3_reduce_kernel, as
tests/test_select_instances.py proves on the CPU -- in bf16 and f16 against the formula in f64 from the
same 16-bit operands (F.conv2d; of F.interpolate(nearest, 2x) for Up2; stride 2 for Down2; bias included)
under the glue's bar (test_gpu_unet_glue.check: u |ref| + u max|ref| 1e-2, u = 2^-8 for bf16, 2^-10 for
f16); torch's own 16-bit chain is printed beside it.  Each row is 3 images on an 8 x 8 output map, image
1 scaled by 64 and every image checked against its own bar, so that a leak across an image boundary
shows.  The C entry is called through ctypes with y AND the f32 workspace (sized exactly by
p2p_conv3x3_ex_workspace_floats) each in the middle of a sentinel-filled buffer; the call runs twice and
must repeat its bits, the binding that allocates its own buffers must give the same bits, and on the
bk = 64, bn = 160 tile the three loops must agree bit for bit.  The loop switch is set eagerly, never
under graph capture, and put back to CONV_LOOP_AUTO in a ``finally``."""
import ctypes
import functools

import pytest
import torch

import kernel_matrix as km
from p2p_amd import _hip

from test_gpu_conv_pipe import formula
from test_gpu_unet_glue import check, rand

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
PAD = 256        # sentinel elements before and after y and the workspace
SENTINEL = 7.0
LOOPS = (km.LOOP_TILE, km.LOOP_PIPE128, km.LOOP_PIPE256)


def test_the_table_has_the_library_constants(cuda):
    assert (km.SAME, km.UP2, km.DOWN2) == (_hip.CONV_SAME, _hip.CONV_UP2, _hip.CONV_DOWN2)
    assert (km.LOOP_AUTO, km.LOOP_TILE, km.LOOP_PIPE128, km.LOOP_PIPE256) == \
           (_hip.CONV_LOOP_AUTO, _hip.CONV_LOOP_TILE, _hip.CONV_LOOP_PIPE128, _hip.CONV_LOOP_PIPE256)


@functools.lru_cache(maxsize=None)
def operands(dev, dtype, form, n, h, w, c_in, c_out, has_bias):
    """(token-major x, packed weight, bias, the f64 reference as f32, torch's own 16-bit chain): computed
    once per (dtype, shape, bias) and shared by the rows that differ in the loop only; nobody writes to them."""
    x = rand((n, c_in, h, w), dtype, dev, 81)
    x[1] *= 64.0              # a leak across an image boundary would show in images 0 and 2
    wt = rand((c_out, c_in, 3, 3), dtype, dev, 82, scale=(9 * c_in) ** -0.5)
    bias = rand((c_out,), dtype, dev, 83) if has_bias else None
    ref = formula(x.double(), wt.double(), None if bias is None else bias.double(), form).float()
    chain = formula(x, wt, bias, form)
    tokens = x.permute(0, 2, 3, 1).reshape(n, h * w, c_in).contiguous()
    packed = _hip.conv3x3_pack(wt)
    assert packed is not None
    return tokens, packed, bias, ref, chain


def guarded(numel, dtype, dev):
    """(a view of ``numel`` elements, the sentinel-filled buffer around it with PAD elements on each side)"""
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=dev)
    return buf[PAD:PAD + numel], buf


def untouched(buf, numel):
    want = torch.full((PAD,), SENTINEL, dtype=buf.dtype, device=buf.device)
    return torch.equal(buf[:PAD], want) and torch.equal(buf[PAD + numel:], want)


def run_guarded(tokens, packed, bias, form, n, h, w, c_out):
    """p2p_conv3x3_ex with y and the workspace each inside a sentinel-filled buffer; returns y after
    asserting that every sentinel still stands."""
    dev, dtype = tokens.device, tokens.dtype
    c_in = tokens.shape[2]
    oh, ow = _hip.conv3x3_out_map(form, h, w)
    numel = n * c_out * oh * ow
    y, y_buf = guarded(numel, dtype, dev)
    n_ws = int(_hip.lib().p2p_conv3x3_ex_workspace_floats(form, n, h, w, c_in, c_out))
    assert n_ws >= 0, n_ws
    split = _hip.conv3x3_ex_split(form, n, h, w, c_in, c_out)
    assert n_ws == (split * numel if split > 1 else 0), (n_ws, split)
    _, ws_buf = guarded(n_ws, torch.float32, dev)    # (no split: an empty workspace, the kernel must not touch it)
    a = _hip.Conv3x3ExArgs()
    a.n, a.in_height, a.in_width, a.c_in, a.c_out, a.form = n, h, w, c_in, c_out, form
    a.x, a.weight, a.y, a.workspace = tokens.data_ptr(), packed.data_ptr(), y.data_ptr(), ws_buf.data_ptr() + 4 * PAD
    if bias is not None:
        a.bias = bias.data_ptr()
    a.dtype = _hip._glue_dtype(tokens)
    rc = _hip.lib().p2p_conv3x3_ex(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    assert untouched(y_buf, numel), "a store past y"
    assert untouched(ws_buf, n_ws), "a store past the f32 workspace"
    return y.view(n, c_out, oh, ow), split


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("row", km.CONV_ROWS, ids=km.conv_id)
def test_conv3x3_instance(cuda, dtype, row):
    form, n, h, w, c_in, c_out, has_bias, loop = row
    tokens, packed, bias, ref, chain = operands(cuda, dtype, form, n, h, w, c_in, c_out, has_bias)
    assert not torch.cuda.is_current_stream_capturing()
    others = {}
    try:
        _hip.conv3x3_set_loop(loop)
        y, split = run_guarded(tokens, packed, bias, form, n, h, w, c_out)
        y2, _ = run_guarded(tokens, packed, bias, form, n, h, w, c_out)
        bound = _hip.conv3x3_ex(tokens, packed, bias, h, w, form)
        if c_out == 160:      # the tile with three loops: the other two, on the same operands
            for other in LOOPS:
                if other != loop:
                    _hip.conv3x3_set_loop(other)
                    others[other] = run_guarded(tokens, packed, bias, form, n, h, w, c_out)[0]
    finally:
        _hip.conv3x3_set_loop(km.LOOP_AUTO)
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y, y2), "two launches on the same operands differ"
    assert bound is not None and torch.equal(bound, y), "the binding's own buffers give other bits"
    for other, yo in others.items():
        assert torch.equal(yo, y), f"loop {km.LOOP_NAMES[other]} and loop {km.LOOP_NAMES[loop]} give different bits"
    for i in range(n):        # per image: the small images' bar must not be hidden behind the large one's max |ref|
        check(y[i], ref[i], dtype, f"conv3x3 matrix {km.conv_id(row)} split {split} image {i} {dtype}", chain[i])
