"""float16 inputs at the shapes of the tuned d = 40 / d = 80 self-attention kernels
(p2p_self40.hip: P >= 2048 / 512, K >= 256, O only) -- GPU.  The bit-exact selection cases of
test_gpu_f16.py at those shapes (fast path, a late peak that takes the exact recompute, a ragged last
tile), and test_self_attention_f16_form / test_self_attention_d80_pipelined mirrored with fp16
tensors."""
import pytest
import torch

from p2p_amd import _hip

from test_gpu_f16 import F16, check_selection_self, o_bar
from test_gpu_kernels import make_qkv, ref_out, ref_probs

pytestmark = pytest.mark.gpu

TUNED_KERNEL = {40: "self40_kernel<40,8,2,256,H16>", 80: "self40_kernel<80,8,1,128,H16>"}
SELECT_TUNED = [  # (N, P, K, H, d, j)
    (2, 2048, 2048, 2, 40, 5), (2, 2048, 2048, 2, 40, 2000), (2, 2100, 2100, 2, 40, 2090),
    (2, 1024, 1024, 2, 80, 5), (2, 1100, 1100, 2, 80, 1090),
]


@pytest.mark.parametrize("geom", SELECT_TUNED, ids=lambda g: "x".join(map(str, g)))
def test_selection_self_bit_exact_tuned_shapes(cuda, geom):
    N, P, K, H, d, _ = geom
    q, kv = torch.empty(N, P, H * d, dtype=F16, device=cuda), torch.empty(N, K, H * d, dtype=F16, device=cuda)
    assert _hip.self_attn_kernel(_hip.make_tensors(q, kv, kv, q, H, d ** -0.5, "bf16")) == TUNED_KERNEL[d]
    check_selection_self(geom)


# ------------------------------------------------------------------ 2. accuracy at the tuned shapes
def _check_self(q, k, v, H, d, src=None):
    o = torch.empty_like(q)
    # the launch below takes the tuned kernel's fp16 form (the library's own answer)
    assert _hip.self_attn_kernel(_hip.make_tensors(q, k, v, o, H, d ** -0.5, "bf16")) == TUNED_KERNEL[d]
    _hip.self_attn(q, k, v, o, H, d ** -0.5, compute="bf16", qk_src=src)
    want = ref_out(ref_probs(q, k, H, d ** -0.5, qk_src=src), v, H)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - want).abs().max().item()
    bound = o_bar(v, want)
    print(f"fp16 self d={d}: |O - want| {err:.3e} (bar {bound:.3e})")
    assert err < bound, (err, bound)


@pytest.mark.parametrize("case", ["plain", "peaky32", "late_peak", "remap", "ragged", "k_max"])
def test_self_attention_d40_f16_inputs(cuda, case):
    """test_self_attention_f16_form with fp16 tensors; k_max (the largest fp16 value as a key
    element, its logits kept moderate by a small q) stands where the bf16 test has its
    past-the-f16-range cases, which fp16 cannot express."""
    N, P, K, H, d = (2, 2100, 2100, 2, 40) if case == "ragged" else (2, 2048, 2048, 2, 40)
    q, k, v = make_qkv(N, P, K, H, d, F16, qscale=32.0 if case == "peaky32" else 1.0, seed=31)
    if case == "k_max":
        k[1, 100, 3] = 65504.0
        q[1, :, 3] = 2.0 ** -10
    if case == "late_peak":
        q[0, 7, :d] = 250.0
        k[0, 1500, :d] = 250.0
    _check_self(q, k, v, H, d, [0, 0] if case == "remap" else None)


@pytest.mark.parametrize("case", ["plain", "peaky32", "late_peak", "remap", "ragged", "k_max"])
def test_self_attention_d80_f16_inputs(cuda, case):
    """test_self_attention_d80_pipelined with fp16 tensors."""
    N, P, K, H, d = (2, 1100, 1100, 2, 80) if case == "ragged" else (2, 1024, 1024, 2, 80)
    q, k, v = make_qkv(N, P, K, H, d, F16, qscale=32.0 if case == "peaky32" else 1.0, seed=33)
    if case == "k_max":
        k[1, 100, 3] = 65504.0
        q[1, :, 3] = 2.0 ** -10
    if case == "late_peak":
        q[0, 7, :d] = 60.0
        k[0, 700, :d] = 60.0
    _check_self(q, k, v, H, d, [0, 0] if case == "remap" else None)
