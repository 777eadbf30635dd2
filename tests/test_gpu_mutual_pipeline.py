"""MutualSelfAttentionControl through the pipeline (GPU): SMALL_UNET (head dims 8 and 16), 10 steps,
3 prompts, bf16.

Teacher-forced: a recording hook keeps q, k, v, the classes and the output of every mutual launch of
an eager run, and each is held to tests/mutual_ref.py with the kernel bound of tests/test_gpu_mutual.py
(o_tol; for the fp16 model test_gpu_f16's) -- the classes are the ones the run built, so no threshold
flip enters the comparison."""
import pytest
import torch

from mutual_ref import mutual_ref, token_classes_ref
from p2p_amd import config, controllers
from p2p_amd import pipeline as pl
from test_gpu_kernels import o_tol

pytestmark = pytest.mark.gpu

SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128))     # tests/test_gpu_pndm.py: head dims 8 and 16
STEPS, SEED = 10, 3
PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a squirrel jumping over a burger",
           "a painting of a squirrel sleeping on a burger"]
REF_WORDS = ("squirrel", "squirrel", "squirrel")
B = len(PROMPTS)
KV_SRC = [0, 0, 0, 3, 3, 3]
EDIT_SRC = [-1, 0, 0, -1, 3, 3]


class Recorder:
    """controllers.MUTUAL_OBSERVER: the operands of every mutual launch (kept alive, not copied: the
    run does not write them again; the classes live in a tensor refilled every step, so a copy)."""

    def __init__(self):
        self.launches = []

    def __call__(self, info):
        tc = info["token_class"]
        self.launches.append({**info, "token_class": None if tc is None else tc.clone()})

    def __enter__(self):
        controllers.MUTUAL_OBSERVER = self
        return self

    def __exit__(self, *exc):
        controllers.MUTUAL_OBSERVER = None


def plain_store():
    ctrl = controllers.AttentionStore()
    ctrl.store_self_maps = False            # as the mutual controller: the self layers keep no maps
    return ctrl


def run(model, ctrl, steps=STEPS, seed=SEED):
    """One eager group.  MIOpen off, as in the other bit-identity tests (tests/test_gpu_dpm.py): the
    convolutions left to torch then run its own deterministic kernels."""
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"):
            lat = pl.run_edit_group(model, PROMPTS, ctrl, pl.seed_latent(seed), num_steps=steps)
        torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.enabled = det
    return lat


def check_launches(launches, fp16=False):
    worst = 0.0
    for rec in launches:
        assert rec["kv_src"] == KV_SRC and rec["edit_src"] == EDIT_SRC
        q, k, v, o = rec["q"], rec["k"], rec["v"], rec["out"]
        want = mutual_ref(q, k, v, rec["heads"], rec["scale"], EDIT_SRC, rec["token_class"])
        tol = o_tol(v, "bf16") + (2.0 ** -10 * want.abs().max().item() if fp16 else 0.0)
        edits = [n for n, s in enumerate(EDIT_SRC) if s >= 0]
        err = (o[edits].double() - want[edits]).abs().max().item()
        worst = max(worst, err / tol)
        assert torch.isfinite(o).all()
        assert err < tol, (rec["step"], q.shape, err, tol)
    return worst


@pytest.fixture(scope="module")
def model(cuda):
    return pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=SMALL_UNET)


@pytest.fixture(scope="module")
def runs(model, cuda):
    r = {"plain": run(model, plain_store()), "plain_again": run(model, plain_store())}
    for name, words in (("unmasked", None), ("masked", REF_WORDS)):
        ctrl = pl.make_mutual_controller(PROMPTS, STEPS, ref_words=words, device=cuda)
        with Recorder() as rec:
            r[name] = run(model, ctrl)
        r[name + "_launches"], r[name + "_ctrl"] = rec.launches, ctrl
    r["never"] = run(model, pl.make_mutual_controller(PROMPTS, STEPS, start_step=STEPS, ref_words=REF_WORDS, device=cuda))
    return r


@pytest.mark.parametrize("name", ["unmasked", "masked"])
def test_teacher_forced_every_launch(runs, name):
    launches = runs[name + "_launches"]
    # steps 4..9, self layers 10..15 (three 32x32 layers of d = 16, three 64x64 layers of d = 8)
    assert len(launches) == 6 * 6
    assert sorted({rec["step"] for rec in launches}) == list(range(4, STEPS))
    assert sorted({(rec["q"].shape[1], rec["q"].shape[2] // rec["heads"]) for rec in launches}) == [(1024, 16), (4096, 8)]
    masked = [rec["token_class"] is not None for rec in launches]
    assert all(masked) if name == "masked" else not any(masked)
    if name == "masked":
        for rec in launches:
            tc = rec["token_class"]
            assert tc.shape == rec["q"].shape[:2] and torch.equal(tc[:B], tc[B:])
            assert 0 < tc.sum().item() < tc.numel()
    worst = check_launches(launches)
    print(f"{name}: worst |O - ref| / bound = {worst:.3f} over {len(launches)} launches")


@pytest.mark.parametrize("name", ["unmasked", "masked"])
def test_source_row_keeps_its_bits(runs, name):
    assert torch.isfinite(runs[name]).all()
    assert torch.equal(runs["plain"], runs["plain_again"])      # the yardstick repeats itself
    assert torch.equal(runs[name][0], runs["plain"][0])


@pytest.mark.parametrize("name", ["unmasked", "masked"])
def test_effect_and_negative_control(runs, name):
    for b in range(1, B):
        assert (runs[name][b] - runs["plain"][b]).abs().max().item() > 1e-3
    assert not torch.equal(runs["masked"][1:], runs["unmasked"][1:])
    assert torch.equal(runs["never"], runs["plain"])          # start_step = num_steps: the whole batch


def test_classes_match_the_torch_lines(runs):
    """The classes of the last step against the torch lines on the controller's own word sums: the
    LocalBlend bar, 99.9 % of the tokens -- after checking, on the CPU, that the torch lines in f32
    and in f64 agree within that bar themselves for this prompt and seed."""
    ctrl = runs["masked_ctrl"]
    sums = ctrl._blend_sums
    assert sums.shape[0] == B and sums.shape[1] == 2 and sums.shape[3] == 256
    sides = sorted(ctrl._mutual_cls["rows"])
    assert sides == [32, 64]
    lo = token_classes_ref([sums.cpu()], 0.1, sides, dtype=torch.float32)
    hi = token_classes_ref([sums.cpu()], 0.1, sides, dtype=torch.float64)
    for side, a, b in zip(sides, lo, hi):
        assert (a == b).float().mean().item() >= 0.999
        got = ctrl._mutual_cls["rows"][side].cpu()
        agree = (got == a).float().mean().item()
        print(f"side {side}: classes agree on {agree:.5f} of the tokens, class 1 on {got.float().mean().item():.3f}")
        assert agree >= 0.999
    # the word sums are the ref words' columns of the five 16x16 cross maps the store kept
    maps = ctrl.attention_store["down_cross"][2:4] + ctrl.attention_store["up_cross"][:3]
    heads = maps[0].shape[0] // B
    for slot, m in enumerate(maps):
        words = torch.einsum("bhpw,bw->bhp", m.reshape(B, heads, 256, -1), ctrl._ref_alpha)
        got = sums[:, 0, slot * heads:(slot + 1) * heads]
        assert (got - words).abs().max().item() < 2e-2 * STEPS      # test_gpu_kernels.WORD_SUM_TOL per call


def test_graphed_runner_replays_bit_identically(model, cuda):
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"):
            def make_ctrl():
                return pl.make_mutual_controller(PROMPTS, STEPS, ref_words=REF_WORDS, device=cuda)
            eager = pl.edit_batch_runner(model, PROMPTS, make_ctrl, STEPS)
            graphed = pl.edit_batch_runner(model, PROMPTS, make_ctrl, STEPS, graphed=True)
            assert isinstance(graphed, pl.GraphedEditRunner)
            for G in (1, 2):
                first = [100 + g for g in range(G)]
                want0 = graphed(first)                # eager on the capture stream, then the capture
                plan = graphed.plans[G]
                assert len(plan["graphs"]) == STEPS and all(m.cur_step == STEPS for m in plan["members"])
                assert isinstance(plan["ctrl"], controllers.GroupBatch) == (G > 1)
                seeds = [200 + g for g in range(G)]
                for want, got in ((eager(seeds), graphed(seeds)), (want0, graphed(first))):
                    for w, g_ in zip(want, got):
                        assert w.shape == g_.shape and torch.isfinite(w).all()
                        assert torch.equal(w, g_), (G, (w - g_).abs().max().item())
    finally:
        torch.backends.cudnn.enabled = det


def test_group_batch_is_one_launch_per_layer(model, cuda, runs):
    """Two groups in one U-Net batch: one mutual launch per layer for both groups, every launch
    within the kernel bound, each group's source row its plain run's (same U-Net batch size)."""
    def make_ctrl():
        return pl.make_mutual_controller(PROMPTS, STEPS, ref_words=REF_WORDS, device=cuda)
    src = [0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9]
    torch.backends.cudnn.enabled, det = False, torch.backends.cudnn.enabled
    try:
        both, plain, rec = _two_groups(model, make_ctrl)
    finally:
        torch.backends.cudnn.enabled = det
    assert len(rec.launches) == 6 * 6 and rec.launches[0]["q"].shape[0] == 4 * B
    for r in rec.launches[::7]:
        assert r["kv_src"] == src and r["token_class"].shape[0] == 4 * B
        edit_src = [-1 if s == n else s for n, s in enumerate(src)]
        want = mutual_ref(r["q"], r["k"], r["v"], r["heads"], r["scale"], edit_src, r["token_class"])
        edits = [n for n, s in enumerate(edit_src) if s >= 0]
        assert (r["out"][edits].double() - want[edits]).abs().max().item() < o_tol(r["v"], "bf16")
    assert torch.isfinite(both).all()
    for g in range(2):
        assert torch.equal(both[g, 0], plain[g, 0])
        assert (both[g, 1:] - plain[g, 1:]).abs().max().item() > 1e-3


def _two_groups(model, make_ctrl):
    with config.compute_mode("bf16"):
        with Recorder() as rec:
            both, _ = pl.edit_batch_runner(model, PROMPTS, make_ctrl, STEPS)([SEED, SEED + 1])
        plain = pl.run_edit_groups(model, [PROMPTS] * 2, controllers.GroupBatch([plain_store(), plain_store()], B),
                                   [pl.seed_latent(SEED), pl.seed_latent(SEED + 1)], num_steps=STEPS).reshape(both.shape)
    torch.cuda.synchronize()
    return both, plain, rec


def test_fp16_model(cuda):
    m16 = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.float16, unet_config=SMALL_UNET)
    ctrl = pl.make_mutual_controller(PROMPTS, 4, start_step=1, ref_words=REF_WORDS, device=cuda)
    with Recorder() as rec:
        lat = run(m16, ctrl, steps=4)
    assert torch.isfinite(lat).all()
    assert len(rec.launches) == 3 * 6 and rec.launches[0]["q"].dtype == torch.float16
    assert all(r["token_class"] is not None for r in rec.launches)
    print(f"fp16: worst |O - ref| / bound = {check_launches(rec.launches, fp16=True):.3f}")
