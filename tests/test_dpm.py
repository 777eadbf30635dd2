"""DPMSolverMultistepScheduler (p2p_amd/dpm.py: DPM-Solver++ 2M) and the argument checks of
p2p_dpm_step -- CPU.

diffusers is not available offline, so the scheduler is checked against the mathematics, by
statements that do not share its code: the timestep grid written out, the DDIM step its first-order
update is, a constant data prediction (the second-order term vanishes), its order of accuracy on a
model with a closed-form solution, and the rule for the last call.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from p2p_amd import _hip
from p2p_amd.dpm import DPMSolverMultistepScheduler, StepPlan


def _double(s):
    s.alphas_cumprod = s.alphas_cumprod.double()
    return s


def _targets(s):
    """The timestep each call steps to."""
    ts = s.timesteps.tolist()
    return ts[1:] + [0]


# ------------------------------------------------------------------ 1. the grid
GRID_20 = [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50]


@pytest.mark.parametrize("n,want", [
    (4, [999, 749, 500, 250]),
    (10, [999, 899, 799, 699, 599, 500, 400, 300, 200, 100]),
    (20, GRID_20),
])
def test_timestep_grid(n, want):
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(n)
    assert s.timesteps.tolist() == want and s.timesteps.dtype == torch.int64
    assert len(want) == n                       # n calls for n steps: no corrector call
    assert s.config.num_train_timesteps == 1000


def test_alphas_are_ddims_and_last_step_goes_to_timestep_0():
    from p2p_amd.ddim import DDIMScheduler
    s = DPMSolverMultistepScheduler()
    assert torch.equal(s.alphas_cumprod, DDIMScheduler().alphas_cumprod) and s.alphas_cumprod.dtype == torch.float32
    s.set_timesteps(4)
    x = torch.zeros(1)
    plans = []
    for t in s.timesteps.tolist():
        plans.append(s.plan_step(t))
        s.step(torch.zeros(1), t, x)
    assert [(p.t_from, p.t_to) for p in plans] == [(999, 749), (749, 500), (500, 250), (250, 0)]
    a0 = float(s.alphas_cumprod[0]) ** 0.5      # alphas_cumprod[0], not a "final alpha" of 1
    a250 = float(s.alphas_cumprod[250])
    assert plans[-1].x_coeff == pytest.approx(((1 - a0 * a0) / (1 - a250)) ** 0.5, rel=1e-12)


def test_set_timesteps_resets():
    s = DPMSolverMultistepScheduler()
    g = torch.Generator().manual_seed(2)
    x_T = torch.randn(1, 4, 8, 8, generator=g)
    eps = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(10)]

    def run(calls=10):
        s.set_timesteps(10)
        assert s.counter == 0 and s.m_prev is None and s._ring is None
        x = x_T
        for e, t in list(zip(eps, s.timesteps.tolist()))[:calls]:
            x = s.step(e, t, x)["prev_sample"]
        return x

    first = run()
    assert s.counter == 10 and s.m_prev is None         # the last call stores nothing
    run(calls=5)                                        # abandoned half-way: history and counter in place
    assert s.counter == 5 and s.m_prev is not None
    assert torch.equal(run(), first)


# ------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("kw", [
    dict(beta_schedule="linear"), dict(solver_order=3), dict(solver_order=0), dict(algorithm_type="dpmsolver"),
    dict(solver_type="heun"), dict(thresholding=True), dict(prediction_type="v_prediction"),
], ids=lambda kw: next(iter(kw)))
def test_unsupported_arguments_raise(kw):
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        DPMSolverMultistepScheduler(**kw)


def test_call_out_of_sequence_raises():
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError):
        DPMSolverMultistepScheduler().step(x, 999, x)            # no set_timesteps
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(4)
    with pytest.raises(RuntimeError):
        s.step(x, 749, x)                                        # the second call's timestep first
    s.step(x, 999, x)
    with pytest.raises(RuntimeError):
        s.step(x, 999, x)                                        # the first call's timestep twice
    for t in (749, 500, 250):
        s.step(x, t, x)
    with pytest.raises(RuntimeError):
        s.step(x, 250, x)                                        # a fifth call of four
    assert s.counter == 4


# ------------------------------------------------------------------ 3. first order is the DDIM step
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("dtype,bar", [(torch.float64, 1e-12), (torch.float32, 1e-6)], ids=["f64", "f32"])
def test_first_order_is_the_ddim_step(order, dtype, bar):
    """abar_t^1/2 x0 + (1 - abar_t)^1/2 e for the same pair of timesteps: every call of solver_order
    1, the first call of order 2."""
    s = DPMSolverMultistepScheduler(solver_order=order)
    if dtype == torch.float64:
        _double(s)
    s.set_timesteps(20)
    ac = s.alphas_cumprod.to(dtype)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 16, 16, generator=g, dtype=dtype)
    worst, compared = 0.0, 0
    for c, (t, t_to) in enumerate(zip(s.timesteps.tolist(), _targets(s))):
        e = torch.randn(2, 4, 16, 16, generator=g, dtype=dtype)
        plan = s.plan_step(t)
        got = s.step(e, t, x)["prev_sample"]
        assert got.dtype == dtype
        if order == 1 or c == 0:
            assert plan.n_hist == 0 and plan.diff_coeff == 0.0
            x0 = (x - (1 - ac[t]).sqrt() * e) / ac[t].sqrt()
            want = ac[t_to].sqrt() * x0 + (1 - ac[t_to]).sqrt() * e
            worst = max(worst, ((got - want).abs().max() / want.abs().max()).item())
            compared += 1
        else:
            assert plan.n_hist == 1
        x = got
    assert compared == (20 if order == 1 else 1)
    print(f"first-order DPM-Solver++ vs the DDIM step (order {order}, {dtype}): {worst:.2e} of max|out| (bar {bar:g})")
    assert worst <= bar, worst


# ------------------------------------------------------------------ 4. constant data prediction
def test_constant_data_prediction_is_first_order():
    """Model outputs chosen so that x0 is the same c at every call, e = (x - a_s c) / sg_s: m0 - m1
    is then 0 up to the rounding of m0 = (x - sg_s e) / a_s, and every second-order call must equal
    the first-order update of the same state.  Bar: m0 is c to a few ulp of |x| / a_s (a_s >= 0.068,
    |x| <= 5: 2e-14), times |diff_coeff| < 4 -- 1e-12 of max|c|; a history entry that is not the
    previous call's x0 moves the result by diff_coeff * |c|, ten orders more.  (The exactly
    representable case is the next test.)"""
    n = 20
    s2, s1 = _double(DPMSolverMultistepScheduler()), _double(DPMSolverMultistepScheduler(solver_order=1))
    ac = s2.alphas_cumprod
    g = torch.Generator().manual_seed(3)
    c = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    s2.set_timesteps(n)
    second, worst = 0, 0.0
    for i, t in enumerate(s2.timesteps.tolist()):
        e = (x - ac[t].sqrt() * c) / (1 - ac[t]).sqrt()
        plan = s2.plan_step(t)
        second += plan.n_hist
        m1 = s2.m_prev
        got = s2.step(e, t, x)["prev_sample"]
        # the same call by the first-order scheduler, its state set to this call
        s1.set_timesteps(n)
        s1.counter, s1.m_prev = i, m1
        first = s1.step(e, t, x)["prev_sample"]
        assert abs(plan.diff_coeff) < 4 and x.abs().max().item() <= 5
        if plan.n_hist:
            worst = max(worst, (got - first).abs().max().item() / c.abs().max().item())
        else:
            assert torch.equal(got, first)
        x = got
    assert second == n - 1                      # n = 20: every call but the first is second-order
    print(f"second-order vs first-order update on a constant data prediction: {worst:.2e} of max|c| (bar 1e-12)")
    assert worst <= 1e-12, worst


def test_constant_data_prediction_exact_zero_difference():
    """The same with a data prediction that is reproduced bit for bit: x = c = 0 gives e = 0 and
    m0 = m1 = 0 exactly at every call, so every second-order call equals the first-order update
    exactly; and with a stored history that differs (m1 = 1) it must not."""
    n = 20
    s = _double(DPMSolverMultistepScheduler())
    s.set_timesteps(n)
    z = torch.zeros(1, 4, 8, 8, dtype=torch.float64)
    for t in s.timesteps.tolist():
        assert torch.equal(s.step(z, t, z)["prev_sample"], z)
    s.set_timesteps(n)
    s.step(z, 999, z)
    s.m_prev = torch.ones_like(z)
    plan = s.plan_step(949)
    got = s.step(z, 949, z)["prev_sample"]
    assert plan.n_hist == 1 and torch.equal(got, torch.full_like(z, plan.diff_coeff))   # 0 - d (0 - 1)
    assert plan.diff_coeff != 0.0


# ------------------------------------------------------------------ 5. order of accuracy on a closed form
def _landing_error(n, var, order, stop=200):
    """Relative error, against the exact probability-flow solution, of the state at the call that
    lands on timestep ``stop``: data N(0, var), x_T = 1, the exact noise prediction as the model."""
    s = _double(DPMSolverMultistepScheduler(solver_order=order))
    s.set_timesteps(n)
    ac = s.alphas_cumprod
    x = torch.ones((), dtype=torch.float64)
    T = int(s.timesteps[0])
    for t, t_to in zip(s.timesteps.tolist(), _targets(s)):
        e = (1 - ac[t]).sqrt() * x / (ac[t] * var + 1 - ac[t])
        x = s.step(e, t, x)["prev_sample"]
        if t_to == stop:
            exact = ((ac[stop] * var + 1 - ac[stop]) / (ac[T] * var + 1 - ac[T])).sqrt()
            return ((x - exact).abs() / exact).item()
    raise AssertionError(f"the grid of n = {n} does not contain {stop}")


# (b)'s bar: half the smallest ratio measured when the method was written (10.6, 26.8, 39.3)
@pytest.mark.parametrize("var", [0.25, 1.0, 4.0])
def test_order_of_accuracy(var):
    """(a) each doubling of n from 10 to 160 divides the error at timestep 200 by at least 3 (second
    order: 4; first order, for comparison, measures 1.96-1.99); (b) at n = 20 the error is at least
    5 times smaller than with solver_order=1.  A wrong r0, a missing 1/2 or h with the wrong sign
    fails one of them.  Measured: (a) 4.0-4.3 / 4.2-5.4 / 4.2-5.3 and (b) 10.6 / 26.8 / 39.3 for
    var 0.25 / 1 / 4.  The trajectory is stopped at timestep 200: the stiff last steps toward t = 0
    (and, below n = 15, the first-order last call) are not part of the figure."""
    ns = (10, 20, 40, 80, 160)
    err2 = [_landing_error(n, var, 2) for n in ns]
    err1 = [_landing_error(n, var, 1) for n in ns]
    r2 = [a / b for a, b in zip(err2, err2[1:])]
    r1 = [a / b for a, b in zip(err1, err1[1:])]
    b = err1[1] / err2[1]
    print(f"var {var}: second-order errors {['%.3e' % e for e in err2]}, ratios per doubling "
          f"{['%.2f' % r for r in r2]} (bar 3); first order {['%.2f' % r for r in r1]}; "
          f"first / second at n = 20: {b:.1f} (bar 5)")
    assert all(r >= 3 for r in r2), r2
    assert b >= 5, b


# ------------------------------------------------------------------ 6. lower_order_final
@pytest.mark.parametrize("lof,n,want", [(True, 10, 0), (True, 20, 1), (True, 14, 0), (True, 15, 1),
                                        (False, 10, 1), (False, 20, 1)])
def test_lower_order_final(lof, n, want):
    s = DPMSolverMultistepScheduler(lower_order_final=lof)
    s.set_timesteps(n)
    x = torch.zeros(1, 1, 2, 2)
    plans = []
    for t in s.timesteps.tolist():
        plans.append(s.plan_step(t))
        s.step(x, t, x)
    assert isinstance(plans[-1], StepPlan)
    assert plans[0].n_hist == 0 and all(p.n_hist == 1 for p in plans[1:-1])
    assert plans[-1].n_hist == want
    assert [p.store for p in plans] == [True] * (n - 1) + [False]


# ------------------------------------------------------------------ 7. C ABI
def test_dpm_step_is_declared():
    text = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    assert re.search(r"^int\s+p2p_dpm_step\s*\(const p2p_dpm_step_args\*", text, flags=re.M)
    assert "p2p_dpm_step" in _hip.EXPORTED_SYMBOLS
    assert _hip.lib().p2p_abi_version() == 16


def test_dpm_args_lead_with_the_plms_fields():
    """The leading fields of p2p_plms_step_args, unchanged in name, type and offset."""
    lead = _hip.PlmsArgs._fields_[:[f[0] for f in _hip.PlmsArgs._fields_].index("hist")]
    assert _hip.DpmArgs._fields_[:len(lead)] == lead
    for name, _ in lead:
        assert getattr(_hip.DpmArgs, name).offset == getattr(_hip.PlmsArgs, name).offset
    assert [f[0] for f in _hip.DpmArgs._fields_[len(lead):len(lead) + 3]] == ["hist", "n_hist", "hist_out"]


def _args(kw):
    a = _hip.DpmArgs()
    a.eps, a.x, a.out = 1024, 2048, 4096
    a.eps_dtype, a.cfg, a.guidance = 1, 1, 7.5
    a.n_prompts, a.channels, a.height, a.width = 4, 4, 64, 64
    a.n_hist = 1
    a.hist[0] = 8192
    a.hist_out = 65536
    a.sigma_s, a.alpha_s, a.x_coeff, a.m0_coeff, a.diff_coeff = 0.9, 0.4, 0.95, -0.1, -0.05
    for k, v in kw.items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


_FOLD = {("blend_sums", 0): 1 << 20, "blend_lh": 40, "blend_res": 16}


@pytest.mark.parametrize("kw,code", [
    (dict(eps=None), -1),
    (dict(x=None), -1),
    (dict(out=None), -1),
    (dict(n_prompts=0), -1),                         # the geometry cases p2p_latent_step rejects
    (dict(channels=0), -1),
    (dict(height=0), -1),
    (dict(width=0), -1),
    (dict(group_size=-1), -1),
    (dict(group_size=3), -1),
    (dict(n_hist=-1), -1),
    (dict(n_hist=2), -1),
    ({("hist", 0): None}, -1),                       # a missing entry with n_hist = 1
    (dict(hist_out=8192), -1),                       # hist_out is the history entry in use
    (dict(hist_out=2048), -1),                       # ... or x
    (dict(hist_out=4096), -1),                       # ... or out
    (dict(alpha_s=0.0), -1),
    (dict(eps_dtype=7), -3),
    # the one-launch LocalBlend form: its own conditions, and 16-byte aligned history pointers (the
    # three step forms answer a misaligned pointer of this form with P2P_E_ARG)
    ({**_FOLD, "mask": 512}, -1),
    ({**_FOLD, "out": 2048}, -1),
    ({**_FOLD, "height": 63, "width": 63}, -1),      # H * W % 4
    ({**_FOLD, "x": 2052}, -1),
    ({**_FOLD, ("hist", 0): 8196}, -1),
    ({**_FOLD, "hist_out": 65540}, -1),
    ({**_FOLD, "blend_res": 17}, -1),                # res^2 > 256
    ({("blend_sums", 3): 1 << 20, "blend_lh": 40, "blend_res": 16}, -1),     # a group past the batch
    (dict(n_hist=2, eps_dtype=7), -3),               # two faults: the dtype is answered before the history
])
def test_dpm_step_rejects(kw, code):
    """Every case returns before any launch (the pointers are not memory: a launch would fault)."""
    assert _hip.lib().p2p_dpm_step(ctypes.byref(_args(kw)), None) == code


def test_dpm_step_rejects_null_args():
    assert _hip.lib().p2p_dpm_step(None, None) == -1
