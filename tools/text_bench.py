"""Text-encoder timing: an encoder on N prompts of 77 tokens, and its attention alone.  Prints one
JSON line.

--encoder clip (the default): the SD-shaped CLIPTextModel, N = 8, and its causal attention.
--encoder ldmbert: the LDM-256-shaped LDMBertModel (all 32 layers, 1280 wide, 8 heads of 64, 5120
MLP), N = 4, and its bidirectional attention.

The encoder in three forms on the same weights: "fused" (the HIP glue and the attention kernel),
"torch" (unet.FUSE_UNET off: the module's torch lines) and "fused_torch_attn" (the fused glue with
the attention proper on its torch lines).  Then one layer's attention on its own (N, T = 77, the
encoder's heads of 64, strided q / k / v views of one QKV tensor): the kernel against the torch
lines.  HIP events around eager calls, warmed up, no graphs; the forms are timed in turn within each
repeat, so drift hits them alike; each figure is the median of --iters repeats.

    python tools/text_bench.py [--encoder clip|ldmbert] [--iters 20] [--warmup 3] [--dtype bf16|f16] [--prompts N]
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

from p2p_amd import _hip, unet  # noqa: E402
from p2p_amd import ldm_bert as lb  # noqa: E402
from p2p_amd import text_encoder as te  # noqa: E402
from p2p_amd.tokenizer import StandInTokenizer  # noqa: E402

FORMS = {"fused": (True, True), "torch": (False, True), "fused_torch_attn": (True, False)}
PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger",
           "a painting of a cat eating a burger", "a painting of a squirrel eating a lasagna"]


def clip_encoder():
    model = te.CLIPTextModel(generator=torch.Generator().manual_seed(1))
    # the masked half is not computed: T (T + 1) / 2 score and weight pairs per head
    return model, te, model.text_model.encoder.layers[0].self_attn, _hip.causal_attn, 77 * 78 / 2


def ldmbert_encoder():
    # (the token table on the stand-in tokenizer's ids, as the pipeline builds it)
    model = lb.LDMBertModel(vocab_size=49408, generator=torch.Generator().manual_seed(1))
    return model, lb, model.model.layers[0].self_attn, _hip.text_attn, 77 * 77


# name: (builder -> (model, the module whose FUSED_ATTENTION it reads, one attention, its kernel's
# binding, score and weight pairs per head), default prompts)
ENCODERS = {"clip": (clip_encoder, 8), "ldmbert": (ldmbert_encoder, 4)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, iters):
    """Median milliseconds of each fn, the fns run in turn within every repeat."""
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    return {k: sorted(v)[len(v) // 2] for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", default="clip", choices=sorted(ENCODERS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--prompts", type=int, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_bench needs a GPU")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    _hip.lib()
    _hip.check_source_hash()
    build, default_n = ENCODERS[args.encoder]
    model, switch, att, kernel, pairs = build()
    model = model.to(dev, dtype).eval()
    N = args.prompts or default_n
    ids = StandInTokenizer()([PROMPTS[i % len(PROMPTS)] for i in range(N)], padding="max_length",
                             max_length=77).input_ids.to(dev)
    out = {"tool": "text_bench", "encoder": args.encoder, "device": torch.cuda.get_device_name(0), "dtype": args.dtype,
           "prompts": N, "tokens": 77, "layers": sum(1 for m in model.modules() if hasattr(m, "fused_calls")),
           "iters": args.iters, "warmup": args.warmup, "unit": "ms, median"}

    def set_form(name):
        unet.FUSE_UNET, switch.FUSED_ATTENTION = FORMS[name]

    def encoder(form):
        def run():
            set_form(form)
            model(ids)
        return run

    with torch.no_grad():
        fns = {form: encoder(form) for form in FORMS}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for form, ms in alternated(fns, args.iters).items():
            out[f"encoder_{form}_ms"] = round(ms, 4)
        set_form("fused")
        fused = model(ids)[0].float()
        set_form("torch")
        out["encoder_fused_vs_torch_max_abs"] = round((fused - model(ids)[0].float()).abs().max().item(), 6)
        set_form("fused")
        # one layer's attention alone, on strided views of one QKV tensor
        H, C = att.num_heads, att.num_heads * att.head_dim
        g = torch.Generator(device=dev).manual_seed(2)
        qkv = torch.randn(N, 77, 3 * C, device=dev, generator=g).to(dtype)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        reps = 50
        fns = {"kernel": lambda: [kernel(q, k, v, H, att.scale) for _ in range(reps)],
               "torch": lambda: [att.attend(q, k, v) for _ in range(reps)]}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for name, ms in alternated(fns, args.iters).items():
            out[f"attn_{name}_ms"] = round(ms / reps, 5)
        out["attn_heads"] = H
        flop = 4.0 * N * H * pairs * att.head_dim
        out["attn_kernel_causal_gflops" if args.encoder == "clip" else "attn_kernel_gflops"] = \
            round(flop / (out["attn_kernel_ms"] * 1e-3) / 1e9, 1)
        err = (kernel(q, k, v, H, att.scale).float() - att.attend(q, k, v).float()).abs().max().item()
        out["attn_kernel_vs_torch_max_abs"] = round(err, 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
