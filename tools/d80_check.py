"""d = 80 self-attention parity probe (experiments build): max |O - ref| / bound for the cases of
tests/test_gpu_kernels.py::test_self_attention_d80_pipelined (P2P_SELF_VARIANT=164 in the environment
checks the stamped kernel instead of the default)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prompt-to-prompt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from p2p_amd import _hip  # noqa: E402
from test_gpu_kernels import make_qkv, o_tol, ref_out, ref_probs  # noqa: E402

for case in ("plain", "peaky32", "peaky8", "late_peak"):
    N, P, K, H, d = 2, 1024, 1024, 2, 80
    qs = {"peaky32": 32.0, "peaky8": 8.0}.get(case, 1.0)
    q, k, v = make_qkv(N, P, K, H, d, torch.bfloat16, qscale=qs, seed=33, dev="cuda")
    if case == "late_peak":
        q[0, 7, :d] = 60.0
        k[0, 700, :d] = 60.0
    o = torch.empty_like(q)
    _hip.self_attn(q, k, v, o, H, d ** -0.5, compute="bf16")
    want = ref_out(ref_probs(q, k, H, d ** -0.5), v, H)
    err = (o.float() - want).abs()
    bound = o_tol(v, "bf16") + 2.0 ** -8 * want.abs().max().item()
    idx = torch.nonzero(err == err.max())[0].tolist()
    print(case, "max err", err.max().item(), "bound", bound, "at", idx, "got", o.float()[tuple(idx)].item(),
          "want", want[tuple(idx)].item(), "bad rows", int((err.amax(-1) > bound).sum()), flush=True)

# detail of the failing rows of peaky32: ratio got / want per d, the row's logit range
N, P, K, H, d = 2, 1024, 1024, 2, 80
q, k, v = make_qkv(N, P, K, H, d, torch.bfloat16, qscale=32.0, seed=33, dev="cuda")
o = torch.empty_like(q)
_hip.self_attn(q, k, v, o, H, d ** -0.5, compute="bf16")
want = ref_out(ref_probs(q, k, H, d ** -0.5), v, H)
err = (o.float() - want).abs().reshape(N, P, H, d).amax(-1)
bad = torch.nonzero(err > 0.1).tolist()
c = d ** -0.5 * 1.4426950408889634
s_all = torch.einsum("nphd,nkhd->nhpk", q.float().reshape(N, P, H, d), k.float().reshape(N, K, H, d)) * c
m32_all = s_all[..., :32].amax(-1)
tmax = s_all.reshape(N, H, P, 8, 128).amax(-1) - m32_all[..., None]
resc = (tmax > 64).any(-1).permute(0, 2, 1)   # n p h
failing = (err > 0.1)
print("rows with a tile max > 64 above m32:", int(resc.sum()), "failing:", int(failing.sum()),
      "failing among them:", int((failing & resc).sum()), flush=True)
for n, p, h in bad[:6]:
    qh = q[n, p, h * d:(h + 1) * d].float()
    kh = k[n, :, h * d:(h + 1) * d].float()
    s = (kh @ qh) * c
    m32 = s[:32].max().item()
    tiles = [round(s[t * 128:(t + 1) * 128].max().item() - m32, 1) for t in range(8)]
    r = (o[n, p, h * d:(h + 1) * d].float() / want[n, p, h * d:(h + 1) * d])
    rl = r.tolist()
    print("   ratio by d (hh0 | hh1):", [round(rl[i], 2) for i in range(d) if (i >> 2) & 1 == 0][:12], "|",
          [round(rl[i], 2) for i in range(d) if (i >> 2) & 1][:12])
    print(f"n {n} p {p} h {h}: m32 {m32:.1f}, tile max - m32 {tiles}, ratio got/want median {r.median().item():.4g}")
