"""HIP-event time per backward call of the U-Net glue at the U-Net's shapes (N = 1): the HIP kernels
(p2p_group_norm_bwd, p2p_geglu_bwd, p2p_nchw_to_tokens; forward outputs and statistics prepared
outside the timed region) against torch autograd's backward of the lines they replace on the same
inputs, with the algorithmic bytes of the fused form, its TB/s and its share of the measured
6.29 TB/s copy rate.  Events bracket REPEAT back-to-back calls; the median of ROUNDS is printed.
Under `rocprofv3 --kernel-trace --stats` the same run gives the per-kernel times.
Usage: python tools/glue_bwd_bench.py [bf16|f16]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from p2p_amd import _hip  # noqa: E402

COPY_TBS = 6.29
REPEAT, ROUNDS = 20, 7


def timed(fn):
    """Median over ROUNDS of the event time of REPEAT calls, in us per call."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPEAT):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / REPEAT)
    return statistics.median(out)


def line(what, nbytes, t_hip, t_torch):
    tbs = nbytes / t_hip / 1e6
    print(f"{what:<44} {nbytes / 1e6:8.2f} MB  hip {t_hip:8.2f} us  {tbs:5.2f} TB/s ({tbs / COPY_TBS * 100:5.1f}% of copy)"
          f"  torch {t_torch:8.2f} us  x{t_torch / t_hip:.2f}", flush=True)


def group_norm(dev, dtype, C, hw, tokens, silu, groups=32, eps=1e-5):
    side = int(hw ** 0.5)
    x = torch.randn(1, C, side, side, device=dev).to(dtype)
    gamma, beta = torch.randn(C, device=dev).to(dtype), torch.randn(C, device=dev).to(dtype)
    dy = torch.randn((1, hw, C) if tokens else (1, C, side, side), device=dev).to(dtype)
    _, stats = _hip.group_norm(x, gamma, beta, groups, eps, silu=silu, tokens=tokens, return_stats=True)
    leaf = x.clone().requires_grad_(True)
    y = F.group_norm(leaf, groups, gamma, beta, eps)
    y = F.silu(y) if silu else y
    y = y.permute(0, 2, 3, 1).reshape(1, hw, C) if tokens else y
    t_hip = timed(lambda: _hip.group_norm_bwd(dy, x, stats, gamma, beta, groups, silu=silu, tokens=tokens))
    t_torch = timed(lambda: torch.autograd.grad(y, leaf, dy, retain_graph=True))
    # reduce reads x and dy, apply reads both again and writes dx
    line(f"group_norm_bwd C={C} {side}x{side} silu={silu} tokens={tokens}", 5 * x.numel() * 2, t_hip, t_torch)


def geglu(dev, dtype, M, D):
    x = torch.randn(M, 2 * D, device=dev).to(dtype)
    dout = torch.randn(M, D, device=dev).to(dtype)
    leaf = x.clone().requires_grad_(True)
    h, gate = leaf.chunk(2, dim=-1)
    y = h * F.gelu(gate)
    t_hip = timed(lambda: _hip.geglu_bwd(dout, x))
    t_torch = timed(lambda: torch.autograd.grad(y, leaf, dout, retain_graph=True))
    line(f"geglu_bwd M={M} D={D}", (2 * x.numel() + dout.numel()) * 2, t_hip, t_torch)


def to_tokens(dev, dtype, C, hw):
    side = int(hw ** 0.5)
    src = torch.randn(1, C, side, side, device=dev).to(dtype)
    t_hip = timed(lambda: _hip.nchw_to_tokens(src))
    t_torch = timed(lambda: src.permute(0, 2, 3, 1).contiguous())
    line(f"nchw_to_tokens C={C} {side}x{side}", 2 * src.numel() * 2, t_hip, t_torch)


def main(dtype="bf16"):
    dev = torch.device("cuda")
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    _hip.check_source_hash()
    print(f"{dtype}, N = 1; bytes are the fused form's algorithmic traffic", flush=True)
    group_norm(dev, dt, 320, 4096, False, True)
    group_norm(dev, dt, 640, 1024, False, True)
    group_norm(dev, dt, 320, 4096, True, False, eps=1e-6)
    geglu(dev, dt, 4096, 1280)
    to_tokens(dev, dt, 320, 4096)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main(*sys.argv[1:2])
