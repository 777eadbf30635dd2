"""Every row of tests/kernel_matrix.py's LINEAR_ROWS -- every instantiation of linear_kernel
(csrc/p2p_linear.hip) and every (bias, residual) state of linear_reduce_kernel, as
tests/test_select_instances.py proves on the CPU -- in bf16 and f16 against the formula in f64 from the
same 16-bit operands (x W^T + bias + res; GEGLU as h * gelu(g) with the erf GELU, p_out as the
pre-activation) under the glue's bar (test_gpu_unet_glue.check: u |ref| + u max|ref| 1e-2, u = 2^-8 for
bf16, 2^-10 for f16), over every output row; torch's own 16-bit chain is printed beside it.  Operands
are test_gpu_linear.operands'.  The C entry is called through ctypes with y, p_out and the f32 workspace
(sized exactly by p2p_linear_workspace_floats) each in the middle of a sentinel-filled buffer; the call
runs twice and must repeat its bits, the binding that allocates its own buffers must give the same
bits, and asking for p_out must not change out's."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import kernel_matrix as km
from p2p_amd import _hip

from test_gpu_linear import operands
from test_gpu_unet_glue import check

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
PAD = 256        # sentinel elements before and after y, p_out and the workspace
SENTINEL = 7.0


def test_the_table_has_the_library_constants(cuda):
    assert (km.LIN_BIAS, km.LIN_GEGLU, km.LIN_RESIDUAL) == (_hip.LINEAR_BIAS, _hip.LINEAR_GEGLU, _hip.LINEAR_RESIDUAL)


@functools.lru_cache(maxsize=None)
def case(dev, dtype, geglu, M, K, N, strided):
    """(x, W, bias, res, x W^T in f64): computed once per shape and shared by the rows that differ in
    form, bias or p_out only; nobody writes to them."""
    x, w, b, res = operands(dev, dtype, M, K, 2 * N if geglu else N, N, strided)
    return x, w, b, res, x.double() @ w.double().t()


def guarded(numel, dtype, dev):
    """(a view of ``numel`` elements, the sentinel-filled buffer around it with PAD elements on each side)"""
    buf = torch.full((numel + 2 * PAD,), SENTINEL, dtype=dtype, device=dev)
    return buf[PAD:PAD + numel], buf


def untouched(buf, numel):
    want = torch.full((PAD,), SENTINEL, dtype=buf.dtype, device=buf.device)
    return torch.equal(buf[:PAD], want) and torch.equal(buf[PAD + numel:], want)


def run_guarded(x, w, bias, res, form, N, want_p):
    """p2p_linear with y, p_out and the workspace each inside a sentinel-filled buffer; returns (y, p or
    None) after asserting that every sentinel still stands."""
    dev, dtype = x.device, x.dtype
    M, K = x.shape
    y, y_buf = guarded(M * N, dtype, dev)
    p, p_buf = guarded(M * 2 * N if want_p else 0, dtype, dev)
    n_ws = int(_hip.lib().p2p_linear_workspace_floats(form, M, K, N))
    assert n_ws >= 0, n_ws
    split = _hip.linear_split(form, M, K, N)
    assert split >= 1 and n_ws == (split * N * ((M + 127) // 128 * 128) if split > 1 else 0), (n_ws, split)
    _, ws_buf = guarded(n_ws, torch.float32, dev)    # (no split: an empty workspace, the kernel must not touch it)
    a = _hip.LinearArgs()
    a.x, a.weight, a.y, a.workspace = x.data_ptr(), w.data_ptr(), y.data_ptr(), ws_buf.data_ptr() + 4 * PAD
    a.x_row_stride = x.stride(0) if M > 1 else K     # as the binding passes them
    if bias is not None:
        a.bias = bias.data_ptr()
    if form == km.LIN_RESIDUAL:
        a.res, a.res_row_stride = res.data_ptr(), (res.stride(0) if M > 1 else N)
    if want_p:
        a.p_out = p.data_ptr()
    a.m, a.k, a.n, a.form, a.dtype = M, K, N, form, _hip._glue_dtype(x)
    rc = _hip.lib().p2p_linear(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    assert untouched(y_buf, M * N), "a store past y"
    assert untouched(p_buf, p.numel()), "a store past p_out (or into a p_out nobody asked for)"
    assert untouched(ws_buf, n_ws), "a store past the f32 workspace"
    return y.view(M, N), (p.view(M, 2 * N) if want_p else None), split


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("row", km.LINEAR_ROWS, ids=km.linear_id)
def test_linear_instance(cuda, dtype, row):
    form, M, K, N, has_bias, strided, want_p = row
    geglu = form == km.LIN_GEGLU
    x, w, b, res, acc = case(cuda, dtype, geglu, M, K, N, strided)
    bias = b if has_bias else None
    res = res if form == km.LIN_RESIDUAL else None
    assert x.stride(0) == (K + 8 if strided else K) and (res is None or res.stride(0) == (N + 16 if strided else N))

    y, p, split = run_guarded(x, w, bias, res, form, N, want_p)
    y2, p2, _ = run_guarded(x, w, bias, res, form, N, want_p)
    assert torch.equal(y, y2) and (p is None or torch.equal(p, p2)), "two launches on the same operands differ"
    bound = _hip.linear(x, w, bias, form, res=res, want_p=want_p)
    assert bound is not None
    by, bp = bound if want_p else (bound, None)
    assert by.shape == (M, N) and torch.equal(by, y), "the binding's own buffers give other bits"
    assert p is None or (bp.shape == (M, 2 * N) and torch.equal(bp, p)), "the binding's own p_out has other bits"

    what = f"linear matrix {km.linear_id(row)} split {split} {dtype}"
    pre = acc if bias is None else acc + bias.double()
    if geglu:
        ref = pre[:, :N] * F.gelu(pre[:, N:])          # (the erf form)
        h, gate = F.linear(x, w, bias).chunk(2, dim=-1)
        chain = h * F.gelu(gate)
        other, _, _ = run_guarded(x, w, bias, None, form, N, not want_p)
        assert torch.equal(other, y), "asking for p_out changed out"
        if want_p:
            check(p, pre, dtype, what + " p_out", F.linear(x, w, bias))
    elif res is not None:
        ref, chain = pre + res.double(), F.linear(x, w, bias) + res
    else:
        ref, chain = pre, F.linear(x, w, bias)
    assert tuple(y.shape) == tuple(ref.shape) == (M, N)   # every output row stands in the comparison
    check(y, ref, dtype, what, chain)
