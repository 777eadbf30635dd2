"""Batched null-text inversion on the GPU: p2p_null_loss and p2p_null_adam against float64
restatements of their formulas, their gating and determinism bit for bit, and
NullInversion.invert_batch against the oracle and against the single-image ``invert``.

Every bar is measured in the test, not fixed: the kernels may err at most twice as much as the f32
torch lines they replace (``_GraphedNullStep.body``'s expression, ``torch.optim.Adam``) err against
the same float64 reference, with a floor of 4 f32 ulp of the value, below which f32 results cannot
be told apart.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import forward as ofw
from oracle import nulltext as ont
from p2p_amd import _hip, config, controllers, ddim, null_text
from p2p_amd import pipeline as pl
from p2p_amd import ptp_utils

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5


def ulp32(v):
    """One f32 unit in the last place of |v| (v a float64 tensor)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 24)


def half_ulp_bf16(v):
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 9)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------ loss kernel
@functools.lru_cache(maxsize=None)
def loss_case(n, dtype):
    """Three images of n elements (inputs on the GPU), the float64 loss and gradient of the formula
    on the widened inputs, and the error of the project's f32 torch lines against them."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n)
    shape = (3, 4, n // 4)
    eps_u = torch.randn(shape, generator=g).to(dev, dtype)
    eps_c = torch.randn(shape, generator=g).to(dev, dtype)
    x = torch.randn(shape, generator=g).to(dev)
    target = torch.randn(shape, generator=g).to(dev)
    sched = ddim.DDIMScheduler()
    sched.set_timesteps(50)
    coef = torch.tensor(sched.prev_coeffs(501), dtype=torch.float32, device=dev)
    # float64 reference
    c = coef.double()
    eu, ec = eps_u.double(), eps_c.double()
    eps = eu + GUIDANCE * (ec - eu)
    r = c[2] * (x.double() - c[0] * eps) / c[1] + c[3] * eps - target.double()
    loss64 = (r * r).reshape(3, -1).mean(1)
    grad64 = (2.0 / n) * (1.0 - GUIDANCE) * (c[3] - c[2] * c[0] / c[1]) * r
    # the project's f32 lines (_GraphedNullStep.body), one image at a time as invert runs them
    leaf = eps_u.float().requires_grad_(True)
    losses = []
    for b in range(3):
        e32 = leaf[b:b + 1] + GUIDANCE * (eps_c[b:b + 1] - leaf[b:b + 1])
        x0 = (x[b:b + 1] - coef[0] * e32) / coef[1]
        prev = coef[2] * x0 + coef[3] * e32
        losses.append(F.mse_loss(prev, target[b:b + 1]))
    torch.stack(losses).sum().backward()
    torch_loss_err = (torch.stack(losses).detach().double() - loss64).abs()
    torch_grad_err = (leaf.grad.double() - grad64).abs().max().item()
    return dict(eps_u=eps_u, eps_c=eps_c, x=x, target=target, coef=coef, loss64=loss64, grad64=grad64,
                torch_loss_err=torch_loss_err, torch_grad_err=torch_grad_err)


def run_loss(case, sel, active=None):
    """The kernel on images ``sel`` of the case."""
    dev = case["x"].device
    idx = torch.tensor(sel, device=dev)
    eu, ec = case["eps_u"][idx].contiguous(), case["eps_c"][idx].contiguous()
    x, tg = case["x"][idx].contiguous(), case["target"][idx].contiguous()
    act = torch.tensor(active if active is not None else [1] * len(sel), dtype=torch.uint8, device=dev)
    loss = torch.full((len(sel),), float("nan"), device=dev)
    grad = torch.full_like(eu, float("nan"))
    _hip.null_loss(eu, ec, x, tg, case["coef"], GUIDANCE, act, loss, grad)
    torch.cuda.synchronize()
    return loss, grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [256, 2304, 16384])
@pytest.mark.parametrize("B", [1, 3])
def test_null_loss_against_float64(cuda, B, n, dtype):
    """Loss and gradient within twice the f32 torch lines' error against float64 (floor: 4 f32 ulp
    of the value; a bf16 gradient additionally half a bf16 ulp for its one rounding).

    Measured on an MI355X (max abs error, kernel / torch f32 lines; losses ~2.4-2.6):
      loss, f32 eps:  n=256 6.4e-8..1.7e-7 / 1.7e-7..2.3e-7;  n=2304 1.3e-7 / 1.1e-7;  n=16384 6.4e-8..1.1e-7 / 1.7e-7
      loss, bf16 eps: n=256 8.8e-8..2.3e-7 / 3.3e-7;  n=2304 4.2e-8 / 4.2e-8;  n=16384 1.5e-8..1.0e-7 / 1.5e-8..1.3e-7
      grad, f32 eps:  n=256 6.4e-9 / 1.7e-8 (|grad| <= 1.4e-2);  n=2304 8.9e-10 / 3.4e-9 (2.2e-3);
                      n=16384 1.3e-10 / 5.8e-10 (3.2e-4) -- the kernel forms the scalar in f64
      grad, bf16 eps: n=256 3.0e-5;  n=2304 5.8e-6;  n=16384 9.0e-7 -- each within half a bf16 ulp of
                      the largest gradient, the one rounding to bf16; torch (f32 leaf) as above."""
    case = loss_case(n, dtype)
    sel = list(range(B))
    loss, grad = run_loss(case, sel)
    loss64, grad64 = case["loss64"][:B], case["grad64"][:B]
    loss_err = (loss.double() - loss64).abs()
    grad_err = (grad.double() - grad64).abs()
    loss_bar = torch.maximum(2 * case["torch_loss_err"][:B], 4 * ulp32(loss64))
    grad_bar = torch.maximum(torch.full_like(grad64, 2 * case["torch_grad_err"]), 4 * ulp32(grad64))
    if dtype == torch.bfloat16:
        grad_bar = grad_bar + half_ulp_bf16(grad64)
    print(f"null_loss B={B} n={n} {dtype}: loss err kernel {loss_err.max().item():.3e} torch "
          f"{case['torch_loss_err'][:B].max().item():.3e} (loss {loss64.max().item():.4f}); grad err kernel "
          f"{grad_err.max().item():.3e} torch {case['torch_grad_err']:.3e} (|grad| max {grad64.abs().max().item():.3e})")
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    assert (loss_err <= loss_bar).all(), (loss_err, loss_bar)
    assert (grad_err <= grad_bar).all(), ((grad_err - grad_bar).max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [256, 2304, 16384])
def test_null_loss_gating_and_determinism(cuda, n, dtype):
    case = loss_case(n, dtype)
    loss3, grad3 = run_loss(case, [0, 1, 2])
    # two launches, identical bits
    loss3b, grad3b = run_loss(case, [0, 1, 2])
    assert torch.equal(bits(loss3), bits(loss3b)) and torch.equal(bits(grad3), bits(grad3b))
    # an inactive image: gradient bitwise zero, loss written all the same, the others untouched
    loss_g, grad_g = run_loss(case, [0, 1, 2], active=[1, 0, 1])
    assert (bits(grad_g[1]) == 0).all()
    assert torch.equal(bits(loss_g), bits(loss3))
    assert torch.equal(bits(grad_g[0]), bits(grad3[0])) and torch.equal(bits(grad_g[2]), bits(grad3[2]))
    # image 2 alone (B = 1) has the bits it has in the last place of B = 3; so has image 0 moved there
    loss1, grad1 = run_loss(case, [2])
    assert torch.equal(bits(loss1[0]), bits(loss3[2])) and torch.equal(bits(grad1[0]), bits(grad3[2]))
    loss_p, grad_p = run_loss(case, [1, 2, 0])
    assert torch.equal(bits(loss_p[2]), bits(loss3[0])) and torch.equal(bits(grad_p[2]), bits(grad3[0]))


# ------------------------------------------------------------------------------------ Adam kernel
LR = float(torch.tensor(1e-2 * (1.0 - 3 / 100.0), dtype=torch.float32))    # the f32 the device holds
ADAM_STEPS = 10


class AdamState:
    def __init__(self, param, lr=LR):
        dev = param.device
        B = param.shape[0]
        self.param = param.clone()
        self.m, self.v = torch.zeros_like(param), torch.zeros_like(param)
        self.lr = torch.tensor(lr, dtype=torch.float32, device=dev)
        self.step = torch.zeros(B, dtype=torch.int32, device=dev)
        self.steps_run = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active = torch.ones(B, dtype=torch.uint8, device=dev)
        self.loss = torch.ones(B, dtype=torch.float32, device=dev)
        self.threshold = torch.full((B,), -1.0, dtype=torch.float32, device=dev)

    def run(self, grad):
        _hip.null_adam(self.param, grad, self.m, self.v, self.lr, self.step, self.active, self.loss, self.threshold,
                       self.steps_run)

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.param, self.m, self.v, self.step, self.steps_run, self.active)]


def adam_inputs(m, dev, B=3):
    g = torch.Generator().manual_seed(m)
    param = torch.randn(B, 77, m // 77, generator=g).to(dev)
    grads = [(1e-3 * torch.randn(B, 77, m // 77, generator=g)).to(dev) for _ in range(ADAM_STEPS)]
    return param, grads


def torch_adam(param, grads, dtype):
    p = param.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR)
    for gr in grads:
        p.grad = gr.to(dtype).clone()
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("m", [77 * 128, 77 * 768])
def test_null_adam_against_float64(cuda, m):
    """Ten steps, B = 3, gradients ~1e-3: parameter and both moments within twice
    torch.optim.Adam's f32 error against torch.optim.Adam in float64 (floor 4 f32 ulp of the value).
    Measured on an MI355X (max abs error, kernel / torch.optim.Adam f32): param 6.4e-7 / 6.4e-7
    (m = 9856) and 9.0e-7 / 9.0e-7 (m = 59136); exp_avg 1.4e-10 / 8.1e-11 and 1.5e-10 / 9.5e-11 (torch
    updates it with one lerp, the kernel as two products); exp_avg_sq 7.6e-15 / 8.9e-15 and
    7.8e-15 / 1.1e-14."""
    param, grads = adam_inputs(m, cuda)
    want = torch_adam(param, grads, torch.float64)
    t32 = torch_adam(param, grads, torch.float32)
    st = AdamState(param)
    for gr in grads:
        st.run(gr)
    torch.cuda.synchronize()
    assert st.step.tolist() == [ADAM_STEPS] * 3 and st.steps_run.tolist() == [ADAM_STEPS] * 3
    assert st.active.tolist() == [1, 1, 1]
    for name, got, w, t in zip(("param", "exp_avg", "exp_avg_sq"), (st.param, st.m, st.v), want, t32):
        err = (got.double() - w).abs()
        terr = (t.double() - w).abs().max().item()
        print(f"null_adam m={m} {name}: max err kernel {err.max().item():.3e} torch f32 {terr:.3e}")
        bar = torch.maximum(torch.full_like(w, 2 * terr), 4 * ulp32(w))
        assert (err <= bar).all(), (name, (err - bar).max().item())


def test_null_adam_gate(cuda):
    """Loss 0 against threshold 1e-5 stops, loss 1 does not, loss == threshold does not (strict <);
    the stopping step's update is applied; afterwards the stopped image keeps every bit and is no
    longer counted; the others match a run in which they were alone."""
    m = 77 * 128
    param, grads = adam_inputs(m, cuda)
    thr = torch.tensor(1e-5, dtype=torch.float32).item()
    st = AdamState(param)
    st.threshold.fill_(thr)
    st.loss.copy_(torch.tensor([0.0, 1.0, thr]))
    st.run(grads[0])
    p1, m1, v1, step1, run1, act1 = st.snapshot()
    assert act1.tolist() == [0, 1, 1]
    assert step1.tolist() == [1, 1, 1] and run1.tolist() == [1, 1, 1]
    # each image alone, same inputs: bit-identical, image 0's stopping update included
    alone = []
    for b in range(3):
        sb = AdamState(param[b:b + 1])
        sb.threshold.fill_(thr)
        sb.loss.copy_(st.loss[b:b + 1])
        sb.run(grads[0][b:b + 1].contiguous())
        alone.append(sb)
        torch.cuda.synchronize()
        assert torch.equal(bits(sb.param[0]), bits(p1[b])) and not torch.equal(bits(p1[b]), bits(param[b]))
        assert torch.equal(bits(sb.m[0]), bits(m1[b])) and torch.equal(bits(sb.v[0]), bits(v1[b]))
    assert alone[0].active.tolist() == [0]
    # further launches: image 0 frozen, the others go on as if alone
    for k in (1, 2):
        st.run(grads[k])
        for b in (1, 2):
            alone[b].run(grads[k][b:b + 1].contiguous())
    p3, m3, v3, step3, run3, act3 = st.snapshot()
    assert torch.equal(bits(p3[0]), bits(p1[0])) and torch.equal(bits(m3[0]), bits(m1[0]))
    assert torch.equal(bits(v3[0]), bits(v1[0]))
    assert step3.tolist() == [1, 3, 3] and run3.tolist() == [1, 3, 3] and act3.tolist() == [0, 1, 1]
    for b in (1, 2):
        assert torch.equal(bits(alone[b].param[0]), bits(p3[b])) and torch.equal(bits(alone[b].m[0]), bits(m3[b]))
        assert torch.equal(bits(alone[b].v[0]), bits(v3[b]))
        assert not torch.equal(bits(p3[b]), bits(p1[b]))


# ------------------------------------------------------------------------------------- end to end
# a narrow U-Net whose head dims (40, 80, 80, 80) all have a compiled attention backward
NARROW = dict(block_out_channels=(160, 320, 320, 320), heads=4)
STEPS, INNER = 4, 3
PROMPTS = ["a painting of a squirrel eating a burger", "a photo of a cat on a sofa", "a lion in the snow"]
STOP, NEVER = 1e9, -1.0


def cos(a, b):
    return F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()


@pytest.fixture(scope="module")
def e2e(cuda):
    """The model, three latents, and per (image, epsilon) the oracle's run and the single-image
    ``invert`` (the code path this feature leaves unchanged) -- computed once for the module."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.float32, unet_config=NARROW)
    x0 = [torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(11 + b)).to(cuda) for b in range(3)]
    sched = model.scheduler
    ref = {}
    for b, eps in ((0, STOP), (0, NEVER), (1, NEVER), (2, NEVER)):
        with config.compute_mode("bf16"):
            inv = null_text.NullInversion(model, num_ddim_steps=STEPS)
            _, x_T, embs = inv.invert(x0[b], PROMPTS[b], num_inner_steps=INNER, early_stop_epsilon=eps)
            assert inv.inner_steps_run == (STEPS if eps == STOP else STEPS * INNER)
        uncond, cond = inv.context.chunk(2)
        ofw.install(model, None)
        sched.set_timesteps(STEPS)
        ac, fa = sched.alphas_cumprod.to(cuda), sched.final_alpha_cumprod.to(cuda)
        traj = ont.ddim_loop(model.unet, ac, fa, sched.timesteps, cond, x0[b], STEPS)
        want, _ = ont.null_optimization(model.unet, ac, fa, sched.timesteps, uncond, cond, traj, STEPS, INNER, eps)
        ref[(b, eps)] = dict(single=[e.clone() for e in embs], single_xT=x_T.clone(), oracle=want, traj=traj,
                             u0=uncond[:1].clone())
    return model, x0, ref


@pytest.mark.parametrize("epsilons", [(STOP, NEVER, NEVER), (NEVER, NEVER, NEVER)], ids=["first-stops", "none-stops"])
@pytest.mark.parametrize("use_graphs", [True, False], ids=["graphed", "eager"])
def test_invert_batch_matches_oracle_and_single(e2e, cuda, use_graphs, epsilons):
    """Per image and DDIM step: the batched run is as close to the oracle as the single-image run
    is (1 - cosine of the embeddings and of the updates at most twice the single run's, floor 1e-6),
    its updates agree with the single run's at least as well as those agree with the oracle's
    (same floor: the cosines are of the same f32 data), and the DDIM trajectories keep the existing
    test's cosine >= 0.9999.  An image whose epsilon is 1e9 stops after one Adam step of every DDIM
    step while the others, in the same batch, run all of theirs.

    Measured on an MI355X, worst over images and steps (graphed and eager give the same figures):
    1 - cos(embedding, oracle) batch 3.5e-7 / single 3.2e-7; 1 - cos(update, oracle) batch 4.2e-4 /
    single 3.3e-4 (largest ratio 1.36); 1 - cos(update batch, update single) <= 5.7e-5, against
    5.4e-5..2.4e-4 single-to-oracle at the same steps."""
    model, x0, ref = e2e
    with config.compute_mode("bf16"):
        inv = null_text.NullInversion(model, num_ddim_steps=STEPS, use_graphs=use_graphs)
        out = inv.invert_batch(x0, PROMPTS, num_inner_steps=INNER, early_stop_epsilon=epsilons)
        traj = inv.ddim_loop(torch.cat(x0))
    assert inv.inner_steps_run_per_image == [STEPS if e == STOP else STEPS * INNER for e in epsilons]
    assert len(out) == 3
    for b, ((gt, rec), x_T, embs) in enumerate(out):
        r = ref[(b, epsilons[b])]
        assert gt is x0[b] and rec is None
        assert x_T.shape == (1, 4, 32, 32) and len(embs) == STEPS and all(e.shape == (1, 77, 768) for e in embs)
        for a, w in zip(traj, r["traj"]):
            assert cos(a[b], w) >= 0.9999
        assert cos(x_T, r["traj"][-1]) >= 0.9999
        u0 = r["u0"]
        for i, (e, s, w) in enumerate(zip(embs, r["single"], r["oracle"])):
            e_b, e_s = 1 - cos(e, w), 1 - cos(s, w)
            u_b, u_s = 1 - cos(e - u0, w - u0), 1 - cos(s - u0, w - u0)
            u_bs = 1 - cos(e - u0, s - u0)
            print(f"image {b} step {i}: 1-cos(emb, oracle) batch {e_b:.3e} single {e_s:.3e}; 1-cos(update, oracle) "
                  f"batch {u_b:.3e} single {u_s:.3e}; 1-cos(update batch, update single) {u_bs:.3e}; "
                  f"|update| {(w - u0).norm().item():.4f}")
            assert e_b <= max(2 * e_s, 1e-6)
            assert u_b <= max(2 * u_s, 1e-6)
            assert u_bs <= max(u_s, 1e-6)


def test_edit_with_batched_embeddings(e2e, cuda):
    """One image's (x_T, embeddings) of a batched inversion feeds text2image_ldm_stable unchanged.
    (That function samples at 512 x 512 only, so this inversion runs on 64 x 64 latents, given as one
    [B, 4, h, w] tensor.)"""
    model, _, _ = e2e
    x0 = torch.randn(3, 4, 64, 64, generator=torch.Generator().manual_seed(21)).to(cuda)
    with config.compute_mode("bf16"):
        inv = null_text.NullInversion(model, num_ddim_steps=STEPS)
        out = inv.invert_batch(x0, PROMPTS, num_inner_steps=1)
        assert inv.inner_steps_run_per_image == [STEPS] * 3
        (gt, _), x_T, embs = out[1]
        assert torch.equal(gt, x0[1:2]) and x_T.shape == (1, 4, 64, 64) and len(embs) == STEPS
        lat, _ = ptp_utils.text2image_ldm_stable(model, [PROMPTS[1]], controllers.EmptyControl(),
                                                 num_inference_steps=STEPS, latent=x_T, uncond_embeddings=embs)
    assert lat.shape == (1, 4, 64, 64) and torch.isfinite(lat).all()
