"""VAE timing: encode and decode of the SD-shaped AutoencoderKL at 512 x 512, and its mid-block
attention alone.  Prints one JSON line.

Per image, for N = 1 and 4, in three forms: "fused" (the HIP glue and the d = 512 attention
kernel), "torch" (unet.FUSE_UNET off: the module's torch lines) and "fused_torch_attn" (the fused
glue with the attention proper on its torch lines).  Then the attention at 4096 x 4096 x 512 on its
own: the wide kernel against the torch lines on the same q / k / v, with the kernel's fraction of
the dense 16-bit MFMA peak (4 P K d FLOP over its time).  HIP events around eager calls, warmed up,
no graphs; the forms are timed in turn within each repeat, so drift hits them alike.

    python tools/vae_bench.py [--iters 5] [--warmup 2] [--dtype bf16|f16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "prompt-to-prompt_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from p2p_amd import _hip, unet, vae  # noqa: E402

MFMA_PEAK_16BIT_TFLOPS = 2500.0   # dense bf16 / f16, as bench.py


def timed(fn, iters):
    """Median milliseconds of fn() between two HIP events."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


FORMS = {"fused": (True, True), "torch": (False, True), "fused_torch_attn": (True, False)}


def set_form(name):
    unet.FUSE_UNET, vae.FUSED_ATTENTION = FORMS[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vae_bench needs a GPU")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    _hip.lib()
    _hip.check_source_hash()
    torch.manual_seed(0)
    model = vae.AutoencoderKL().to(dev, dtype).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    out = {"tool": "vae_bench", "dtype": args.dtype, "iters": args.iters, "unit": "ms per image"}
    with torch.no_grad():
        for n in (1, 4):
            z = torch.randn(n, 4, 64, 64, device=dev, generator=g).to(dtype)
            img = torch.rand(n, 3, 512, 512, device=dev, generator=g).mul(2).sub(1).to(dtype)
            calls = {"decode": lambda: model.decode(z), "encode": lambda: model.encode(img)}
            for what, fn in calls.items():
                for form in FORMS:
                    set_form(form)
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                for form in FORMS:
                    set_form(form)
                    out[f"{what}_n{n}_{form}"] = round(timed(fn, args.iters) / n, 4)
        set_form("fused")
        # the mid-block attention alone: one head of 512 over 4096 tokens, strided q / k / v views
        P = 4096
        att = model.decoder.mid_block.attentions[0]
        qkv = torch.randn(1, P, 3 * 512, device=dev, generator=g).to(dtype)
        q, k, v = qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]
        o = torch.empty(1, P, 512, device=dev, dtype=dtype)
        t = _hip.make_tensors(q, k, v, o, 1, att.scale, "bf16")
        out["attn_kernel"] = _hip.self_attn_kernel(t)
        wide = lambda: _hip.self_attn(q, k, v, o, 1, att.scale)       # noqa: E731
        lines = lambda: att.attend(q, k, v)                            # noqa: E731
        for fn in (wide, lines):
            for _ in range(max(args.warmup, 3)):
                fn()
        torch.cuda.synchronize()
        reps = 20
        out["attn_4096x4096x512_wide_ms"] = round(timed(lambda: [wide() for _ in range(reps)], args.iters) / reps, 5)
        out["attn_4096x4096x512_torch_ms"] = round(timed(lambda: [lines() for _ in range(reps)], args.iters) / reps, 5)
        flop = 4.0 * P * P * 512
        tf = flop / (out["attn_4096x4096x512_wide_ms"] * 1e-3) / 1e12
        out["attn_wide_tflops"] = round(tf, 2)
        out["attn_wide_frac_of_16bit_mfma_peak"] = round(tf / MFMA_PEAK_16BIT_TFLOPS, 4)
        err = (o.float() - lines().float()).abs().max().item()
        out["attn_wide_vs_torch_max_abs"] = round(err, 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
