"""float64 reference of mutual self-attention (include/p2p_hip.h, p2p_mutual_attn_fwd), plain torch:

    s = kv_src[n]  (None = identity);  s < 0: entry n is skipped, out[n] keeps what it held
    O[n] = softmax(Q[n] K[s]^T * scale + M) V[s]

With token classes and s != n, key j is admitted for query p iff token_class[s][j] ==
token_class[n][p]; a query whose class has no key in entry s admits every key.  M = 0 on admitted
keys, -inf elsewhere.  s == n: plain self-attention.

mutual_ref() walks the entries and heads in loops; mutual_ref_dense() is a second, loop-free
formulation (one batched masked softmax) that the CPU tests hold it against.  token_classes_ref()
is the torch lines of p2p_token_classes."""
import torch


def admitted(token_class, n, s):
    """bool [P, P]: row p, column j -- whether query p of entry n reads key j of entry s."""
    P = token_class.shape[1]
    cq = token_class[n].bool()
    ck = token_class[s].bool()
    adm = cq[:, None] == ck[None, :]
    has = torch.stack([(~ck).any(), ck.any()])            # entry s holds a key of class 0 / 1
    fallback = ~has[cq.long()]                            # the query's class is absent from s
    return adm | fallback[:, None].expand(P, P)


def mutual_ref(q, k, v, heads, scale, kv_src=None, token_class=None, out=None):
    """[N, P, C] float64.  ``out``: what the skipped entries keep (default zeros)."""
    N, P, C = q.shape
    d = C // heads
    q, k, v = q.double(), k.double(), v.double()
    res = torch.zeros(N, P, C, dtype=torch.float64, device=q.device) if out is None else out.double().clone()
    for n in range(N):
        s = n if kv_src is None else int(kv_src[n])
        if s < 0:
            continue
        mask = None
        if token_class is not None and s != n:
            mask = admitted(token_class, n, s)
        for h in range(heads):
            c = slice(h * d, (h + 1) * d)
            logits = q[n, :, c] @ k[s, :, c].T * scale
            if mask is not None:
                logits = logits.masked_fill(~mask, float("-inf"))
            res[n, :, c] = logits.softmax(-1) @ v[s, :, c]
    return res


def mutual_ref_dense(q, k, v, heads, scale, kv_src=None, token_class=None, out=None):
    """The same without loops: gather K / V rows by kv_src, one masked softmax over [N, H, P, P]."""
    N, P, C = q.shape
    d = C // heads
    src = torch.arange(N) if kv_src is None else torch.as_tensor(list(kv_src), dtype=torch.long)
    run = src >= 0
    g = src.clamp(min=0).to(q.device)
    qh = q.double().reshape(N, P, heads, d).transpose(1, 2)
    kh = k.double()[g].reshape(N, P, heads, d).transpose(1, 2)
    vh = v.double()[g].reshape(N, P, heads, d).transpose(1, 2)
    logits = torch.einsum("nhpd,nhjd->nhpj", qh, kh) * scale
    if token_class is not None:
        cq = token_class.long()                                   # [N, P]
        ck = token_class.long()[g]                                # [N, P] keys of the source
        same = cq[:, :, None] == ck[:, None, :]                   # [N, P, P]
        count = torch.stack([(ck == 0).sum(1), (ck == 1).sum(1)], 1)      # [N, 2]
        absent = count.gather(1, cq) == 0                         # [N, P]
        own = (g == torch.arange(N, device=q.device))[:, None, None]
        adm = same | absent[:, :, None] | own
        logits = logits + torch.where(adm, 0.0, float("-inf")).double()[:, None]
    o = torch.einsum("nhpj,nhjd->nhpd", logits.softmax(-1), vh).transpose(1, 2).reshape(N, P, C)
    keep = torch.zeros_like(o) if out is None else out.double()
    return torch.where(run.to(q.device)[:, None, None], o, keep)


def token_classes_ref(sums, threshold, sides, cfg=True, dtype=torch.float32):
    """The torch lines of p2p_token_classes for a list of per-group word sums [B, 2, lh, res^2]:
    per side a uint8 [rows, side^2] tensor, rows = (uncond | cond) x groups x B with cfg."""
    per_prompt = []
    for s in sums:
        B, _, lh, R2 = s.shape
        res = int(round(R2 ** 0.5))
        m = s[:, 0].to(dtype).sum(1) / lh                                   # [B, res^2]
        mn, mx = m.min(1, keepdim=True).values, m.max(1, keepdim=True).values
        rng = mx - mn
        cls = torch.where(rng > 0, ((m - mn) / rng) >= threshold, torch.zeros_like(m, dtype=torch.bool))
        per_prompt.append(cls.reshape(B, res, res))
    cls = torch.cat(per_prompt, 0)
    res = cls.shape[-1]
    outs = []
    for side in sides:
        idx = (torch.arange(side, device=cls.device) * res) // side        # nearest: floor(dst * res / side)
        up = cls[:, idx][:, :, idx].reshape(cls.shape[0], side * side).to(torch.uint8)
        outs.append(torch.cat([up, up], 0) if cfg else up)
    return outs
