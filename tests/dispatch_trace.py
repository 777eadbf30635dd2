"""The controllers' fused dispatch as a CPU trace: what every HIP binding is handed.

controllers.py turns the reference's controller semantics into the kernels' arguments (prompt-group
tuples, ``qk_src`` remaps, AttentionStore targets and slots, LocalBlend fold tuples) and ptp_utils
into the latent step's.  None of that needs a GPU: with the bindings of ``p2p_amd._hip`` replaced by
recorders the fused paths run on CPU tensors.  ``trace()`` drives every scenario below through
``controller.attention()`` in the SD U-Net's layer order and returns the recorded calls;
tests/test_dispatch_trace.py compares them with tests/golden/dispatch_trace.json.

    python tests/dispatch_trace.py --write [--tree PATH]     (re)generate the golden
    python tests/dispatch_trace.py --time N [--tree PATH]    host cost of the drive, recorders off

``--tree`` selects the checkout whose ``p2p_amd`` is imported (default: this file's).
"""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dispatch_trace.json")

# the SD U-Net's transformer blocks in call order (place, queries); each is a self call followed by
# a cross call
LAYERS = ([("down", 4096)] * 2 + [("down", 1024)] * 2 + [("down", 256)] * 2 + [("mid", 64)]
          + [("up", 256)] * 3 + [("up", 1024)] * 3 + [("up", 4096)] * 3)
HEADS, CHANNELS, STEPS = 2, 8, 4
BOUND = ("cross_attn", "self_attn", "attn_probs", "attn_pv", "localblend", "latent_step", "plms_step")

PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger",
           "a painting of a cat eating a burger", "a painting of a squirrel eating a lasagna"]
WORDS = (("squirrel", "burger"), ("lion",), ("cat",), ("lasagna",))
REFINE = ["a photo of a house on a mountain", "a photo of a house on a snowy mountain",
          "a photo of a wooden house on a mountain"]


def load(tree=None):
    """The product modules of the checkout at ``tree``."""
    pkg = os.path.join(os.path.abspath(tree or os.path.dirname(HERE)), "prompt-to-prompt_amd")
    if "p2p_amd" in sys.modules and not os.path.abspath(sys.modules["p2p_amd"].__file__).startswith(pkg):
        raise RuntimeError("p2p_amd is already imported from another tree")
    sys.path.insert(0, pkg)
    names = ("_hip", "config", "controllers", "null_text", "pipeline", "ptp_utils", "tokenizer")
    mods = SimpleNamespace(**{n: importlib.import_module(f"p2p_amd.{n}") for n in names})
    mods.tok = mods.tokenizer.StandInTokenizer()
    return mods


# ------------------------------------------------------------------------------ the recorder
def _digest(t):
    return [list(t.shape), hashlib.sha1(t.detach().contiguous().numpy().tobytes()).hexdigest()[:12]]


class Recorder:
    """Stands in for the bindings and keeps what they were handed.  Tensors the kernels write or
    keep across calls (stores, programs, word sums) are numbered by first appearance of their
    storage; every one is held, so no address is used twice."""

    def __init__(self):
        self.held, self.numbers, self.events = [], {}, []

    def number(self, t):
        key = t.untyped_storage().data_ptr()
        if key not in self.numbers:
            self.numbers[key] = len(self.held)
            self.held.append(t)
        return self.numbers[key]

    def ref(self, t):
        return None if t is None else [self.number(t), t.storage_offset(), list(t.shape)]

    def _store(self, store, store_slot, accumulate):
        return {"store": self.ref(store), "slots": None if store_slot is None else [int(s) for s in store_slot],
                "accumulate": bool(accumulate)}

    def _group(self, grp):
        first, count, prog, alpha = grp[:4]
        blend = grp[4] if len(grp) > 4 else None
        if prog is not None:
            prog = {"t": self.number(prog), "flags": int(getattr(prog, "p2p_flags", 0)),
                    "n_edits": int(getattr(prog, "p2p_n_edits", 0))}
        if blend is not None:
            sums, balpha, bsub, col, lh = blend
            blend = {"sums": self.ref(sums), "alpha": _digest(balpha), "sub": None if bsub is None else _digest(bsub),
                     "col": int(col), "lh": int(lh)}
        return [int(first), int(count), prog, None if alpha is None else _digest(alpha), blend,
                int(grp[5]) if len(grp) > 5 else 0]

    def cross_attn(self, q, k, v, o, heads, scale, groups, compute="bf16", store=None, store_slot=None,
                   accumulate=False):
        self.events.append({"fn": "cross_attn", "q": list(q.shape), "K": k.shape[1], "heads": heads, "compute": compute,
                            "groups": [self._group(g) for g in groups], **self._store(store, store_slot, accumulate)})

    def self_attn(self, q, k, v, o, heads, scale, compute="bf16", qk_src=None, store=None, store_slot=None,
                  accumulate=False):
        src = list(range(q.shape[0])) if qk_src is None else [int(s) for s in qk_src]
        self.events.append({"fn": "self_attn", "q": list(q.shape), "K": k.shape[1], "heads": heads, "compute": compute,
                            "qk_src": src, **self._store(store, store_slot, accumulate)})

    def attn_probs(self, q, k, heads, scale, probs, compute="bf16", key_mask=None):
        self.events.append({"fn": "attn_probs", "q": list(q.shape), "K": k.shape[1], "heads": heads,
                            "probs": list(probs.shape), "key_mask": None if key_mask is None else list(key_mask.shape)})

    def attn_pv(self, probs, v, o, heads, compute="bf16"):
        self.events.append({"fn": "attn_pv", "probs": list(probs.shape), "o": list(o.shape), "heads": heads})

    def localblend(self, maps, heads_per_map, alpha_layers, substruct_layers, th_pool, th_sub, x_t, word_sums,
                   mask_out=None, word_sums_ready=False):
        self.events.append({"fn": "localblend", "maps": [self.ref(m) for m in maps], "heads": heads_per_map,
                            "alpha": _digest(alpha_layers),
                            "sub": None if substruct_layers is None else _digest(substruct_layers),
                            "th": [float(th_pool), float(th_sub)], "x_t": None if x_t is None else list(x_t.shape),
                            "word_sums": self.ref(word_sums), "ready": bool(word_sums_ready),
                            "mask_out": None if mask_out is None else list(mask_out.shape)})

    def _latent(self, fn, eps, x, guidance, mask, group_size, group_blend, blend, **more):
        if blend is not None:
            blend = [None if e is None else [self.ref(e[0]), float(e[1]), float(e[2]), bool(e[3])] for e in blend]
        self.events.append({"fn": fn, "eps": list(eps.shape), "x": list(x.shape), "guidance": guidance,
                            "mask": None if mask is None else [list(mask.shape), str(mask.dtype)],
                            "group_size": int(group_size),
                            "group_blend": None if group_blend is None else [int(b) for b in group_blend.tolist()],
                            "blend": blend, **more})

    def latent_step(self, eps, x, out, coeffs, guidance=None, mask=None, group_size=0, group_blend=None, blend=None):
        self._latent("latent_step", eps, x, guidance, mask, group_size, group_blend, blend,
                     coeffs=[float(c) for c in coeffs])
        return out

    def plms_step(self, eps, x, out, plan, guidance=None, mask=None, group_size=0, group_blend=None, blend=None,
                  hist=(), hist_out=None):
        self._latent("plms_step", eps, x, guidance, mask, group_size, group_blend, blend, n_hist=len(hist),
                     hist_out=hist_out is not None)
        return out


class NoRecorder:
    """The bindings as no-ops (host-cost timing)."""
    events = ()

    def __getattr__(self, name):
        if name in ("latent_step", "plms_step"):
            return lambda eps, x, out, *a, **k: out
        return lambda *a, **k: None

    def ref(self, t):
        return None


# ------------------------------------------------------------------------------ the drive
_ZEROS = {}


def _zeros(*shape):
    if shape not in _ZEROS:
        _ZEROS[shape] = torch.zeros(*shape)
    return _ZEROS[shape]


def _members(ctrl):
    return list(getattr(ctrl, "members", [ctrl]))


def _watch_blends(ctrl, kinds):
    """Note, per prompt group, the kind of step mask its LocalBlend makes (the step-mask protocol)."""
    for g, m in enumerate(_members(ctrl)):
        lb = getattr(m, "local_blend", None)
        if lb is None or not hasattr(lb, "step_mask"):
            continue

        def step_mask(store, size, folded=None, g=g, orig=lb.step_mask):
            mk = orig(store, size, folded=folded)
            kinds[g] = "none" if mk is None else ("mask" if isinstance(mk, torch.Tensor) else type(mk).__name__)
            return mk
        lb.step_mask = step_mask


def _state(rec, ctrl):
    out = []
    for c in ([ctrl] if _members(ctrl) == [ctrl] else [ctrl] + _members(ctrl)):
        store = getattr(c, "attention_store", None)
        out.append({"type": type(c).__name__, "cur_step": getattr(c, "cur_step", None),
                    "blend_valid": getattr(c, "_blend_valid", None),
                    "store": None if store is None else {k: [rec.ref(t) for t in v] for k, v in sorted(store.items())}})
    return out


def drive(mods, ctrl, n_cond, rec, steps=STEPS, K=77, low_resource=False, hw=(64, 64), plms=False, n_batch=None,
          mask=None):
    """``steps`` denoising steps of ``ctrl`` over ``n_cond`` prompts: the U-Net's 32 attention calls
    (twice, per CFG half, under LOW_RESOURCE), then the fused latent step; the recorded events."""
    for name in BOUND:
        setattr(mods._hip, name, getattr(rec, name))
    mods.config.LOW_RESOURCE = low_resource
    ctrl.num_att_layers = 2 * len(LAYERS)
    kinds = {}
    _watch_blends(ctrl, kinds)
    events = rec.events
    x, eps = _zeros(n_cond, 4, *hw), _zeros(2 * n_cond, 4, *hw)
    hist = (_zeros(n_cond, 4, *hw).clone(),) if plms else ()
    sched = SimpleNamespace(prev_coeffs=lambda t: (0.25, 0.5, 0.75, 1.0))
    plan = SimpleNamespace(n_hist=1) if plms else None
    try:
        for step in range(steps):
            if low_resource:
                passes = [(n_cond, (0,) * n_cond), (n_cond, tuple(range(n_cond)))]
            else:
                N = 2 * n_cond if n_batch is None else n_batch
                passes = [(N, (0,) * (N // 2) + tuple(range(N // 2, N)))]
            for N, rows in passes:
                k, v = _zeros(N, K, HEADS * CHANNELS).clone(), _zeros(N, K, HEADS * CHANNELS).clone()
                k._p2p_rows = v._p2p_rows = rows
                for place, P in LAYERS:
                    h = _zeros(N, P, HEADS * CHANNELS)
                    ctrl.attention(h, h, h, HEADS, 0.125, False, place, mask)
                    ctrl.attention(h, k, v, HEADS, 0.125, True, place, mask)
            kinds.clear()
            ok, mask_fn = ctrl.fused_step_mask()
            if ok:
                out = torch.empty_like(x)
                mods.ptp_utils._launch_latent_step(sched, mask_fn, eps, x, x, out, 0, 7.5, plan, hist,
                                                   out if plms else None)
            else:
                ctrl.step_callback(x)
            if events != ():
                events.append({"step": step, "fused_step": ok,
                               "mask_kinds": [kinds.get(g, "none") for g in range(len(_members(ctrl)))],
                               "state": _state(rec, ctrl)})
    except Exception as err:      # a refused call ends the scenario: the exception's type is the record
        if events == ():
            raise
        events.append({"raises": type(err).__name__})
    finally:
        mods.config.LOW_RESOURCE = False
    return events


# ------------------------------------------------------------------------------ the scenarios
def scenarios(mods):
    """name -> (make() -> controller, drive keywords).  Controllers are built per run."""
    c, nt, pl, tok = mods.controllers, mods.null_text, mods.pipeline, mods.tok
    two = PROMPTS[:2]
    kw = dict(tokenizer=tok, device="cpu")

    def replace(blend=None, fold=True, prompts=PROMPTS, th=(.3, .3)):
        lb = None
        if blend == "main":
            lb = c.LocalBlend(prompts, WORDS[:len(prompts)], **kw)
        elif blend == "null":
            lb = nt.LocalBlend(prompts, WORDS[:len(prompts)], start_blend=0.04, th=th, **kw)
        cls = c.AttentionReplace if blend != "null" else nt.AttentionReplace
        ctrl = cls(prompts, STEPS, 0.5, 0.5, local_blend=lb, **kw)
        ctrl.fold_local_blend = fold
        return ctrl

    def refine_blend():
        lb = nt.LocalBlend(REFINE, (("house",), ("snowy",), ("wooden",)), substruct_words=(("mountain",),) * 3,
                           start_blend=0.04, th=(.3, .4), **kw)
        return nt.AttentionRefine(REFINE, STEPS, 0.5, 0.5, local_blend=lb, **kw)

    def refine_reweight():
        return pl.make_refine_reweight_controller(REFINE, STEPS, **kw)

    def store(self_maps):
        s = c.AttentionStore()
        s.store_self_maps = self_maps
        return s

    def user_forward():
        class Mine(c.AttentionStore):
            def forward(self, attn, is_cross, place_in_unet):
                return super().forward(attn, is_cross, place_in_unet)
        return Mine()

    def unfusable_program():
        class Mine(c.AttentionReplace):
            def replace_cross_attention(self, attn_base, att_replace):
                return super().replace_cross_attention(attn_base, att_replace)
        inner = Mine(two, STEPS, 0.5, 0.5, **kw)
        eq = c.get_equalizer(two[1], ("lion",), (2.0,), tokenizer=tok)
        return c.AttentionReweight(two, STEPS, 0.5, 0.5, equalizer=eq, controller=inner, **kw)

    def late_self_maps():
        g = c.GroupBatch([store(False), store(False)], group_size=2)
        g.members[1].store_self_maps = True
        return g

    def group_raises(make):
        def run():
            try:
                return make()
            except ValueError as err:
                return err
        return run

    return {
        "empty": (c.EmptyControl, dict(n_cond=2)),
        "store_self": (lambda: store(True), dict(n_cond=2)),
        "store_cross_only": (lambda: store(False), dict(n_cond=2)),
        "replace": (replace, dict(n_cond=4)),
        "replace_blend_main": (lambda: replace("main", prompts=two), dict(n_cond=2)),
        "replace_blend_main_nofold": (lambda: replace("main", fold=False, prompts=two), dict(n_cond=2)),
        "replace_blend_null": (lambda: replace("null"), dict(n_cond=4)),
        "replace_blend_null_small_latent": (lambda: replace("null"), dict(n_cond=4, hw=(8, 8))),
        "replace_blend_null_plms": (lambda: replace("null"), dict(n_cond=4, plms=True)),
        "refine_blend_substruct": (refine_blend, dict(n_cond=3)),
        "refine_reweight": (refine_reweight, dict(n_cond=3)),
        "replace_low_resource": (lambda: replace("null"), dict(n_cond=4, low_resource=True)),
        "group_2x_replace_blend": (lambda: c.GroupBatch([replace("null"), replace("null")]), dict(n_cond=8)),
        "group_2x_replace_blend_small_latent": (lambda: c.GroupBatch([replace("null"), replace("null")]),
                                                dict(n_cond=8, hw=(8, 8))),
        "group_3x_refine_reweight": (lambda: c.GroupBatch([refine_reweight() for _ in range(3)]), dict(n_cond=9)),
        "group_2x_empty": (lambda: c.GroupBatch([c.EmptyControl(), c.EmptyControl()], group_size=2), dict(n_cond=4)),
        "group_blend_and_none": (lambda: c.GroupBatch([replace("null"), replace()]), dict(n_cond=8)),
        "group_blend_nofold_and_none": (lambda: c.GroupBatch([replace("null", fold=False), replace()]),
                                        dict(n_cond=8)),
        "group_two_thresholds": (lambda: c.GroupBatch([replace("null"), replace("null", th=(.4, .3))]),
                                 dict(n_cond=8)),
        "group_2x_store": (lambda: c.GroupBatch([store(True), store(True)], group_size=2), dict(n_cond=4)),
        "group_2x_store_cross_only": (lambda: c.GroupBatch([store(False), store(False)], group_size=2),
                                      dict(n_cond=4)),
        # the fallbacks to the materialised protocol
        "fallback_100_keys": (lambda: replace(prompts=two), dict(n_cond=2, K=100, steps=2)),
        "fallback_50_keys": (lambda: replace(prompts=two), dict(n_cond=2, K=50, steps=2)),
        "fallback_unfusable_program": (unfusable_program, dict(n_cond=2, steps=2)),
        "fallback_user_forward": (user_forward, dict(n_cond=1, steps=2)),
        "store_100_keys": (lambda: store(False), dict(n_cond=2, K=100, steps=2)),
        # the refusals
        "raises_single_wrong_batch": (replace, dict(n_cond=3, steps=1)),
        "raises_group_low_resource": (lambda: c.GroupBatch([replace(), replace()]),
                                      dict(n_cond=8, low_resource=True, steps=1)),
        "raises_group_mask": (lambda: c.GroupBatch([replace(), replace()]),
                              dict(n_cond=8, steps=1, mask=torch.ones(16, 77))),
        "raises_group_wrong_batch": (lambda: c.GroupBatch([replace(), replace()]), dict(n_cond=8, n_batch=12, steps=1)),
        "raises_group_edit_tables": (lambda: c.GroupBatch([replace(), replace()]), dict(n_cond=8, K=50, steps=1)),
        "group_100_keys": (lambda: c.GroupBatch([replace(), replace()]), dict(n_cond=8, K=100, steps=2)),
        "raises_group_self_maps_late": (late_self_maps, dict(n_cond=4, steps=1)),
        "raises_group_self_maps_built": (group_raises(lambda: c.GroupBatch([store(True), store(False)], group_size=2)),
                                         None),
        "raises_group_mixed_storing": (group_raises(lambda: c.GroupBatch([store(True), c.EmptyControl()],
                                                                         group_size=2)), None),
        "raises_group_sizes": (group_raises(lambda: c.GroupBatch([replace(), replace(prompts=two)])), None),
    }


def trace(mods, only=None):
    """{scenario: its events}, each scenario with a recorder (and tensor numbers) of its own."""
    out = {}
    saved = {name: getattr(mods._hip, name) for name in BOUND}
    try:
        for name, (make, kw) in scenarios(mods).items():
            if only is not None and name not in only:
                continue
            ctrl = make()
            if kw is None:      # the constructor is the scenario
                out[name] = [{"raises": type(ctrl).__name__ if isinstance(ctrl, Exception) else None}]
            else:
                out[name] = drive(mods, ctrl, rec=Recorder(), **kw)
    finally:
        for name, fn in saved.items():
            setattr(mods._hip, name, fn)
    return out


def pack(traces):
    """The golden's form: every distinct record once, each scenario as indices into them."""
    records, index, runs = [], {}, {}
    for name, events in traces.items():
        run = []
        for ev in events:
            key = json.dumps(ev, sort_keys=True)
            if key not in index:
                index[key] = len(records)
                records.append(json.loads(key))
            run.append(index[key])
        runs[name] = run
    return {"records": records, "scenarios": runs}


def host_cost(mods, name, runs):
    """Seconds of ``runs`` drives of scenario ``name`` with the bindings as no-ops."""
    make, kw = scenarios(mods)[name]
    saved = {n: getattr(mods._hip, n) for n in BOUND}
    times = []
    try:
        for _ in range(runs):
            ctrl = make()
            t0 = time.perf_counter()
            drive(mods, ctrl, rec=NoRecorder(), **kw)
            times.append(time.perf_counter() - t0)
    finally:
        for n, fn in saved.items():
            setattr(mods._hip, n, fn)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="write tests/golden/dispatch_trace.json")
    ap.add_argument("--time", type=int, default=0, metavar="N", help="time N no-op drives of the two blend scenarios")
    ap.add_argument("--tree", default=None, help="checkout whose p2p_amd is imported")
    args = ap.parse_args()
    mods = load(args.tree)
    if args.time:
        for name in ("group_2x_replace_blend", "replace_blend_null"):
            host_cost(mods, name, 1)     # (first-use costs: imports, program tables)
            ts = host_cost(mods, name, args.time)
            print(json.dumps({"scenario": name, "median_ms": round(1e3 * statistics.median(ts), 3),
                              "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3),
                              "runs_ms": [round(1e3 * t, 3) for t in ts]}))
        return
    packed = pack(trace(mods))
    text = json.dumps(packed, sort_keys=True, separators=(",", ":")) + "\n"
    if args.write:
        with open(GOLDEN, "w") as f:
            f.write(text)
    print(f"{len(packed['records'])} distinct records, {sum(map(len, packed['scenarios'].values()))} events, "
          f"{len(text)} bytes")


if __name__ == "__main__":
    main()
