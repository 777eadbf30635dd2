"""One seeded U-Net forward (N = 8, 64x64 latents, bf16, random-init SD-v1.4 shape) with MIOpen's
deterministic convolutions, written as a float32 .npy -- the run-to-run reproducible A/B that
bench.py --dump-outputs cannot be (MIOpen's default convolutions differ in the last bits from
process to process, profiles/r06/determinism_probe.log, and 50 DDIM steps amplify that).
Two trees, or the two settings of P2P_FUSE_UNET, are compared by comparing their files:
    P2P_FUSE_UNET=0 python tools/unet_switch_check.py off.npy
    python tools/unet_switch_check.py off.npy --compare parent.npy      # prints max |delta|
--pkg DIR imports p2p_amd from another checkout's prompt-to-prompt_amd directory.
--vs-f32 prints, instead of writing a file, the distance of that forward to the same model run in
float32, for the setting of the switches the process was started with (P2P_FUSE_UNET, P2P_CONV, P2P_LINEAR)."""
import argparse
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "prompt-to-prompt_amd"))
    ap.add_argument("--compare", default=None, help="an earlier file: print the distance instead of running")
    ap.add_argument("--vs-f32", action="store_true", help="print the distance to the float32 model; `out` is a label")
    args = ap.parse_args()
    if args.compare:
        a, b = np.load(args.out), np.load(args.compare)
        d = np.abs(a - b)
        print(f"{args.out} vs {args.compare}: " + ("bit-equal" if np.array_equal(a, b) else
                                                    f"max |delta| {d.max():.4e}, mean {d.mean():.4e}, max |a| {np.abs(a).max():.3f}"))
        return
    sys.path.insert(0, args.pkg)
    import torch
    torch.backends.cudnn.deterministic = True
    from p2p_amd import _hip, unet
    _hip.lib()
    _hip.check_source_hash()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    # (frozen, as the pipelines load it: the fused time path declines parameters that require grad)
    model = unet.UNet2DConditionModel().to(dev, torch.bfloat16).eval().requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(8, 4, 64, 64, device=dev, generator=g)
    ctx = torch.randn(8, 77, 768, device=dev, generator=g)
    with torch.no_grad():
        y = model(x, 501, ctx)["sample"]
        again = model(x, 501, ctx)["sample"]
    torch.cuda.synchronize()
    assert torch.equal(y, again), "two forwards in one process differ: the check cannot tell anything"
    if args.vs_f32:
        with torch.no_grad():
            ref = model.float()(x, 501, ctx)["sample"]
        d = (y.float() - ref).abs()
        print(f"{args.out}: fused glue {getattr(unet, 'FUSE_UNET', None)}, HIP conv3x3 {getattr(unet, 'CONV_HIP', None)}, "
              f"HIP linear {getattr(unet, 'LINEAR_HIP', None)}: "
              f"against the f32 U-Net max |delta| {d.max().item():.4e}, mean {d.mean().item():.4e}, "
              f"max |ref| {ref.abs().max().item():.3f}")
        return
    np.save(args.out, y.float().cpu().numpy())
    print(f"{args.out}: fused glue {getattr(unet, 'FUSE_UNET', None)}, max |y| {y.abs().max().item():.3f}")


if __name__ == "__main__":
    main()
