"""Null-text inversion end to end with the U-Net glue fused under autograd (unet.fused_glue_grad):
a narrow bf16 U-Net whose head dims all have a compiled attention backward (the shape set of
test_gpu_null_batch.py), 32 x 32 latents, 4 DDIM x 3 inner steps, against a deep copy of the model
upcast to f32.  The convolutions run on PyTorch's native path, as in the other bit-identity tests.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from p2p_amd import _hip, config, null_text, unet
from p2p_amd import pipeline as pl

pytestmark = pytest.mark.gpu

NARROW = dict(block_out_channels=(160, 320, 320, 320), heads=4)
STEPS, INNER = 4, 3
PROMPTS = ["a painting of a squirrel eating a burger", "a photo of a cat on a sofa", "a lion in the snow"]
STOP, NEVER = 1e9, -1.0
BWD = ("group_norm_bwd", "geglu_bwd", "nchw_to_tokens")


def cos(a, b):
    return F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Runs:
    """The inversions the tests compare, each computed once on first use."""

    def __init__(self, dev):
        self.dev = dev
        self.model = pl.SyntheticStableDiffusion(device=dev, dtype=torch.bfloat16, unet_config=NARROW)
        self.model32 = copy.deepcopy(self.model)
        self.model32.unet.float()
        self.x0 = [torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(11 + b)).to(dev) for b in range(3)]
        self.cache = {}

    def _counted(self, fn):
        """fn() with the backward bindings counted."""
        counts = dict.fromkeys(BWD, 0)
        saved = {name: getattr(_hip, name) for name in BWD}

        def wrap(name):
            def counted(*a, **kw):
                counts[name] += 1
                return saved[name](*a, **kw)
            return counted

        for name in BWD:
            setattr(_hip, name, wrap(name))
        try:
            return fn(), counts
        finally:
            for name in BWD:
                setattr(_hip, name, saved[name])

    def _run(self, fused, fn):
        was_fused, was_cudnn = unet.FUSE_UNET_GRAD, torch.backends.cudnn.enabled
        unet.FUSE_UNET_GRAD, torch.backends.cudnn.enabled = fused, False
        try:
            with config.compute_mode("bf16"):
                out, counts = self._counted(fn)
            torch.cuda.synchronize()
            return out, counts
        finally:
            unet.FUSE_UNET_GRAD, torch.backends.cudnn.enabled = was_fused, was_cudnn

    def single(self, which, use_graphs=True, fused=True):
        key = ("single", which, use_graphs, fused)
        if key not in self.cache:
            def fn():
                inv = null_text.NullInversion(self.model32 if which == "f32" else self.model, num_ddim_steps=STEPS,
                                              use_graphs=use_graphs)
                _, x_T, embs = inv.invert(self.x0[0], PROMPTS[0], num_inner_steps=INNER, early_stop_epsilon=NEVER)
                assert inv.inner_steps_run == STEPS * INNER
                return dict(x_T=x_T.clone(), embs=[e.clone() for e in embs], u0=inv.context.chunk(2)[0].clone())
            out, counts = self._run(fused, fn)
            out["counts"] = counts
            self.cache[key] = out
        return self.cache[key]

    def batch(self, use_graphs):
        key = ("batch", use_graphs)
        if key not in self.cache:
            def fn():
                inv = null_text.NullInversion(self.model, num_ddim_steps=STEPS, use_graphs=use_graphs)
                out = inv.invert_batch(self.x0, PROMPTS, num_inner_steps=INNER, early_stop_epsilon=(STOP, NEVER, NEVER))
                return dict(steps=list(inv.inner_steps_run_per_image),
                            images=[(x_T.clone(), [e.clone() for e in embs]) for _, x_T, embs in out])
            out, counts = self._run(True, fn)
            out["counts"] = counts
            self.cache[key] = out
        return self.cache[key]


@pytest.fixture(scope="module")
def runs(cuda):
    return Runs(cuda)


def test_fused_updates_are_as_close_to_f32_as_the_torch_lines(runs):
    """Per DDIM step: 1 - cos(update, the f32 model's update) with the path on is at most twice that
    with it off (floor 1e-6, below which cosines of f32 data cannot be told apart).  The update is
    the optimised null embedding minus the initial one."""
    ref, on, off = runs.single("f32"), runs.single("bf16"), runs.single("bf16", fused=False)
    u0 = ref["u0"]
    assert torch.equal(on["u0"], u0) and torch.equal(off["u0"], u0)
    for i in range(STEPS):
        w = ref["embs"][i] - u0
        e_on, e_off = 1 - cos(on["embs"][i] - u0, w), 1 - cos(off["embs"][i] - u0, w)
        print(f"step {i}: 1-cos(update, f32 update) fused {e_on:.3e} torch lines {e_off:.3e}; |update| {w.norm().item():.4f}")
        assert torch.isfinite(on["embs"][i]).all()
        assert e_on <= max(2 * e_off, 1e-6)
    assert cos(on["x_T"], ref["x_T"]) >= 0.9999


def test_backward_bindings_run_only_with_the_path_on(runs):
    on, off, ref = runs.single("bf16"), runs.single("bf16", fused=False), runs.single("f32")
    print(f"backward binding calls with the path on: {on['counts']}")
    assert all(on["counts"][name] > 0 for name in BWD)
    assert not any(off["counts"].values()) and not any(ref["counts"].values())


def test_one_step_graphed_and_eager_same_bits(runs, cuda):
    """The gradient of the null embedding through the fused U-Net: a replayed capture against the
    eager call, bit for bit (no host synchronisation, no value read back, fixed-order reductions)."""
    model = runs.model
    x = runs.x0[0].clone()
    t = torch.full((1,), 501, dtype=torch.int64, device=cuda)
    param = (0.1 * torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(3))).to(cuda).requires_grad_(True)
    param.grad = torch.zeros_like(param)
    dy = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(4)).to(cuda, torch.bfloat16)

    def body():
        param.grad.zero_()
        model.unet(x, t, encoder_hidden_states=param)["sample"].backward(dy)

    def fn():
        from p2p_amd import ptp_utils
        ptp_utils.register_attention_control(model, None)
        body()
        eager = param.grad.clone()
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(cuda).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        param.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        return eager, param.grad.clone()

    (eager, replayed), counts = runs._run(True, fn)
    assert all(counts[name] > 0 for name in BWD)
    assert eager.abs().max().item() > 0 and torch.isfinite(eager).all()
    assert torch.equal(bits(eager), bits(replayed))


def test_invert_batch_graphed_and_eager_same_bits(runs):
    """Epsilons (1e9, -1, -1): the first image stops after one Adam step per DDIM step, the others run
    all of theirs, and the graphed and eager runs agree bit for bit."""
    g, e = runs.batch(True), runs.batch(False)
    assert g["steps"] == [STEPS, STEPS * INNER, STEPS * INNER] and e["steps"] == g["steps"]
    assert all(g["counts"][name] > 0 for name in BWD) and all(e["counts"][name] > 0 for name in BWD)
    for (xg, eg), (xe, ee) in zip(g["images"], e["images"]):
        assert torch.equal(bits(xg), bits(xe))
        for a, b in zip(eg, ee):
            assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b))
