"""Which mutual_attn_kernel shape runs (select_mutual, csrc/p2p_select.h), pinned on the CPU through
p2p_mutual_attn_kernel: it validates and selects as p2p_mutual_attn_fwd does and launches nothing.
The production self kernels' selection is untouched."""
import pytest

from p2p_amd import _hip

from test_select import BF16, C16, C32, F16, F32, _tensors


def mutual(bk, waves, masked):
    return "mutual_attn_kernel<…,D,%d,%d%s>" % (bk, waves, ",MASKED" if masked else "")


ROWS = [  # (id, io, compute, d, P, key tile, waves)
    ("g1_bf16", BF16, C16, 40, 4096, 64, 8),
    ("g1_f16", F16, C16, 40, 4096, 64, 8),
    ("g1_split", F32, C16, 40, 4096, 64, 8),
    ("g1_f32", F32, C32, 40, 4096, 32, 4),
    ("g2_bf16", BF16, C16, 80, 1024, 64, 8),
    ("g2_f16", F16, C16, 80, 1024, 64, 8),
    ("g2_split", F32, C16, 80, 1024, 64, 8),
    ("g2_f32", F32, C32, 80, 1024, 32, 4),
    ("g3_bf16", BF16, C16, 160, 256, 32, 4),
    ("g3_f16", F16, C16, 160, 256, 32, 4),
    ("g3_split", F32, C16, 160, 256, 32, 4),
    ("g3_f32", F32, C32, 160, 256, 32, 4),
    ("d8_bf16", BF16, C16, 8, 4096, 64, 4),
    ("d8_f16", F16, C16, 8, 4096, 64, 4),
    ("d8_split", F32, C16, 8, 4096, 64, 4),
    ("d8_f32", F32, C32, 8, 4096, 32, 4),
    ("d16_bf16", BF16, C16, 16, 1024, 64, 4),
    ("d16_f16", F16, C16, 16, 1024, 64, 4),
    ("d16_split", F32, C16, 16, 1024, 64, 4),
    ("d16_f32", F32, C32, 16, 1024, 32, 4),
    ("d40_p64", BF16, C16, 40, 64, 64, 4),           # P <= 64: four waves
    ("d40_p65", BF16, C16, 40, 65, 64, 8),
    ("d64", BF16, C16, 64, 1024, 64, 4),
    ("d128", BF16, C16, 128, 1024, 32, 4),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
@pytest.mark.parametrize("masked", [False, True])
def test_mutual_kernel_selected(row, masked):
    _, io, compute, d, P, bk, waves = row
    assert _hip.mutual_attn_kernel(_tensors(io, compute, d, P, P), masked) == mutual(bk, waves, masked)


@pytest.mark.parametrize("masked", [False, True])
def test_no_kernel(masked):
    assert _hip.mutual_attn_kernel(_tensors(BF16, C16, 44, 1024, 1024), masked) is None      # not a compiled head dim
    assert _hip.mutual_attn_kernel(_tensors(BF16, C32, 40, 4096, 4096), masked) is None      # f32 compute on 16-bit tensors
    assert _hip.mutual_attn_kernel(_tensors(F16, C32, 40, 4096, 4096), masked) is None
    assert _hip.mutual_attn_kernel(_tensors(BF16, C16, 40, 4096, 77), masked) is None        # n_query != n_key
    assert _hip.mutual_attn_kernel(_tensors(BF16, C16, 512, 1024, 1024), masked) is None     # the VAE's width: self only


def test_production_self_kernels_keep_their_selection():
    assert _hip.self_attn_kernel(_tensors(BF16, C16, 40, 4096, 4096)) == "self40_kernel<40,8,2,256>"
    assert _hip.self_attn_kernel(_tensors(BF16, C16, 80, 1024, 1024)) == "self40_kernel<80,8,1,128>"
    assert _hip.self_attn_kernel(_tensors(F16, C16, 40, 4096, 4096)) == "self40_kernel<40,8,2,256,H16>"
