"""PNDMScheduler in its PLMS form (p2p_amd/pndm.py) and the argument checks of p2p_plms_step -- CPU.

The scheduler is checked against statements that do not share its code: the timestep grid written
out, a float64 restatement of the method with true divisions, the DDIM step it reduces to for a
constant model output, and its order of accuracy on a model with a known solution.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from p2p_amd import _hip
from p2p_amd.ddim import DDIMScheduler
from p2p_amd.pndm import PNDMScheduler
from p2p_amd.ptp_words import get_time_words_attention_alpha


# ------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("n,offset,want", [
    (50, 1, [981, 961] + list(range(961, 0, -20))),
    (50, 0, [980, 960] + list(range(960, -1, -20))),
    (100, 1, [991, 981] + list(range(981, 0, -10))),
])
def test_timestep_grid(tok, n, offset, want):
    s = PNDMScheduler(steps_offset=offset)
    s.set_timesteps(n)
    assert s.timesteps.tolist() == want
    assert len(want) == n + 1 and want[1] == want[2] and want[-1] == offset
    prompts = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger"]
    assert len(s.timesteps) == get_time_words_attention_alpha(prompts, n, 0.8, tok).shape[0]


def test_grid_head_written_out():
    s = PNDMScheduler()
    s.set_timesteps(50)
    assert s.timesteps.tolist()[:6] == [981, 961, 961, 941, 921, 901]
    assert s.timesteps.tolist()[-3:] == [41, 21, 1]
    assert s.config.num_train_timesteps == 1000
    d = DDIMScheduler()
    assert torch.equal(s.alphas_cumprod, d.alphas_cumprod) and s.alphas_cumprod.dtype == torch.float32
    assert torch.equal(s.final_alpha_cumprod, d.final_alpha_cumprod)


def test_unsupported_configurations_raise():
    with pytest.raises(NotImplementedError):
        PNDMScheduler(skip_prk_steps=False)
    with pytest.raises(NotImplementedError):
        PNDMScheduler(beta_schedule="linear")


# ------------------------------------------------------------------ 2. closed form
def closed_form(ac, final, c, t, r, e_new, stored, x, kept):
    """Call c of the method in float64, true divisions.  ac: alphas_cumprod (float64); stored: the
    model outputs stored before this call, oldest first; e_new: this call's; x: this call's sample;
    kept: call 0's sample.  Returns (prev, the error scale of its f32 evaluation)."""
    E = [e.double() for e in stored]
    e = e_new.double()
    if c == 0:
        terms, t_from, t_to, src = [(1.0, e)], t, t - r, x
    elif c == 1:
        terms, t_from, t_to, src = [(1 / 2, e), (1 / 2, E[-1])], t + r, t, kept
    elif len(E) == 1:
        terms, t_from, t_to, src = [(3 / 2, e), (-1 / 2, E[-1])], t, t - r, x
    elif len(E) == 2:
        terms, t_from, t_to, src = [(23 / 12, e), (-16 / 12, E[-1]), (5 / 12, E[-2])], t, t - r, x
    else:
        terms = [(55 / 24, e), (-59 / 24, E[-1]), (37 / 24, E[-2]), (-9 / 24, E[-3])]
        t_from, t_to, src = t, t - r, x
    m = sum(w * v for w, v in terms)
    a_t = ac[t_from]
    a_p = ac[t_to] if t_to >= 0 else final
    coeff = (a_p / a_t).sqrt()
    num, den = a_p - a_t, a_t * (1 - a_p).sqrt() + (a_t * (1 - a_t) * a_p).sqrt()
    src = src.double()
    prev = coeff * src - num * m / den
    scale = (coeff * src).abs() + (num / den).abs() * sum(abs(w) * v.abs() for w, v in terms)
    return prev, scale


def test_closed_form_51_calls():
    s = PNDMScheduler()
    s.set_timesteps(50)
    ac, final = s.alphas_cumprod.double(), s.final_alpha_cumprod.double()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 64, 64, generator=g)
    stored, kept, worst, worst_of_max = [], None, 0.0, 0.0
    for c, t in enumerate(s.timesteps.tolist()):
        e = torch.randn(2, 4, 64, 64, generator=g)
        want, scale = closed_form(ac, final, c, t, 20, e, stored, x, kept)
        got = s.step(e, t, x)["prev_sample"]
        assert got.dtype == torch.float32
        # both sides hold the same f32 history
        if c == 0:
            kept = x
        if c != 1:
            stored = (stored + [e])[-4:]
        assert len(s.ets) == len(stored) and all(torch.equal(a, b) for a, b in zip(s.ets, stored))
        err = (got.double() - want).abs()
        ratio = (err / (scale * 2.0 ** -24)).max().item()
        worst, worst_of_max = max(worst, ratio), max(worst_of_max, (err.max() / want.abs().max()).item())
        assert ratio <= 16, (c, t, ratio)
        x = got
    assert s.counter == 51
    print(f"PLMS f32 vs float64 closed form: worst {worst:.2f} x 2^-24 of the term magnitudes (bar 16), "
          f"{worst_of_max:.2e} of max|out|")


# ------------------------------------------------------------------ 3. DDIM identity
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dtype,bar", [(torch.float64, 1e-12), (torch.float32, 1e-6)], ids=["f64", "f32"])
def test_constant_eps_is_the_ddim_step(offset, dtype, bar):
    """The multistep weights sum to 1: with one constant model output every non-corrector call is
    the DDIM step of the same timestep (from the same fixed sample; nothing is chained)."""
    p, d = PNDMScheduler(steps_offset=offset), DDIMScheduler(steps_offset=offset)
    if dtype == torch.float64:
        for sch in (p, d):
            sch.alphas_cumprod = sch.alphas_cumprod.double()
            sch.final_alpha_cumprod = sch.final_alpha_cumprod.double()
    p.set_timesteps(50)
    d.set_timesteps(50)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 16, 16, generator=g, dtype=dtype)
    e = torch.randn(2, 4, 16, 16, generator=g, dtype=dtype)
    worst, compared = 0.0, 0
    for c, t in enumerate(p.timesteps.tolist()):
        got = p.step(e, t, x)["prev_sample"]
        assert got.dtype == dtype
        if c == 1:
            continue
        want = d.prev_step(e, t, x)
        worst = max(worst, ((got - want).abs().max() / want.abs().max()).item())
        compared += 1
    assert compared == 50
    print(f"PLMS with a constant eps vs DDIM prev_step ({dtype}): {worst:.2e} of max|out| (bar {bar:g})")
    assert worst <= bar, worst


# ------------------------------------------------------------------ 4. order of accuracy
def _toy_eps(ac, x, t, var=0.25):
    """The exact noise prediction for data N(0, var I)."""
    a = ac[int(t)]
    return x * (1 - a).sqrt() / (a * var + 1 - a)


def _double(s):
    s.alphas_cumprod = s.alphas_cumprod.double()
    s.final_alpha_cumprod = s.final_alpha_cumprod.double()
    return s


def _sample(s, n, x):
    s.set_timesteps(n)
    for t in s.timesteps.tolist():
        x = s.step(_toy_eps(s.alphas_cumprod, x, t), t, x)["prev_sample"]
    return x


def test_order_of_accuracy():
    """PLMS lands several times closer to the 1000-step DDIM solution than DDIM with the same number
    of steps (float64, seeded: reproducible).  A wrong weight, a stored E1 or a wrong corrector
    timestep lands below 1.  The bars are half the ratios measured when the method was written
    (9.16 at n = 50, 5.05 at n = 20)."""
    g = torch.Generator().manual_seed(0)
    x_T = torch.randn(4, 4, 8, 8, generator=g, dtype=torch.float64)
    ref = _sample(_double(DDIMScheduler(steps_offset=0)), 1000, x_T)
    ratios = {}
    for n in (50, 20, 10):
        ddim = (_sample(_double(DDIMScheduler(steps_offset=0)), n, x_T) - ref).abs().max().item()
        plms = (_sample(_double(PNDMScheduler(steps_offset=0)), n, x_T) - ref).abs().max().item()
        ratios[n] = ddim / plms
        print(f"n = {n}: DDIM {ddim:.4g}, PLMS {plms:.4g}, ratio {ratios[n]:.2f}")
    assert ratios[50] >= 4, ratios
    assert ratios[20] >= 2.5, ratios


# ------------------------------------------------------------------ 5. reset
def test_set_timesteps_resets():
    s = PNDMScheduler()
    g = torch.Generator().manual_seed(2)
    x_T = torch.randn(1, 4, 8, 8, generator=g)
    eps = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(11)]

    def run(calls=11):
        s.set_timesteps(10)
        assert s.counter == 0 and s.ets == [] and s.cur_sample is None
        x = x_T
        for e, t in list(zip(eps, s.timesteps.tolist()))[:calls]:
            x = s.step(e, t, x)["prev_sample"]
        return x

    first = run()
    run(calls=5)                    # abandoned half-way: history, counter and kept sample in place
    assert s.counter == 5 and len(s.ets) == 4
    run(calls=1)
    assert s.cur_sample is not None
    assert torch.equal(run(), first)
    with pytest.raises(RuntimeError):
        PNDMScheduler().step(eps[0], 981, x_T)      # no set_timesteps


# ------------------------------------------------------------------ 6. C ABI
def test_plms_step_is_declared():
    text = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    assert re.search(r"^int\s+p2p_plms_step\s*\(const p2p_plms_step_args\*", text, flags=re.M)
    assert "p2p_plms_step" in _hip.EXPORTED_SYMBOLS
    assert _hip.lib().p2p_abi_version() == 16


def _args(kw):
    a = _hip.PlmsArgs()
    a.eps, a.x, a.out = 1024, 2048, 4096
    a.eps_dtype, a.cfg, a.guidance = 1, 1, 7.5
    a.n_prompts, a.channels, a.height, a.width = 4, 4, 64, 64
    a.n_hist = 3
    a.hist[0], a.hist[1], a.hist[2] = 8192, 16384, 32768
    a.hist_out = 65536
    for i, w in enumerate((55 / 24, -59 / 24, 37 / 24, -9 / 24)):
        a.w[i] = w
    a.sample_coeff, a.eps_num, a.eps_den = 1.01, 0.02, 0.5
    for k, v in kw.items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(eps=None), -1),
    (dict(x=None), -1),
    (dict(out=None), -1),
    (dict(n_prompts=0), -1),
    (dict(group_size=3), -1),
    (dict(n_hist=-1), -1),
    (dict(n_hist=5), -1),
    ({("hist", 1): None}, -1),                       # a missing entry below n_hist
    (dict(hist_out=16384), -1),                      # hist_out is a history entry in use
    (dict(hist_out=2048), -1),                       # ... or x
    (dict(hist_out=4096), -1),                       # ... or out
    (dict(eps_den=0.0), -1),
    (dict(eps_dtype=7), -3),
    # the one-launch LocalBlend form: its own conditions, and 16-byte aligned history pointers
    ({("blend_sums", 0): 1 << 20, "blend_lh": 40, "blend_res": 16, "mask": 512}, -1),
    ({("blend_sums", 0): 1 << 20, "blend_lh": 40, "blend_res": 16, "out": 2048}, -1),
    ({("blend_sums", 0): 1 << 20, "blend_lh": 40, "blend_res": 16, "height": 63, "width": 63}, -1),   # H * W % 4
    ({("blend_sums", 0): 1 << 20, "blend_lh": 40, "blend_res": 16, ("hist", 2): 32772}, -1),
    ({("blend_sums", 0): 1 << 20, "blend_lh": 40, "blend_res": 16, "hist_out": 65540}, -1),
    ({("blend_sums", 3): 1 << 20, "blend_lh": 40, "blend_res": 16}, -1),     # a group past the batch
    (dict(n_hist=5, eps_dtype=7), -3),               # two faults: the dtype is answered before the history
])
def test_plms_step_rejects(kw, code):
    assert _hip.lib().p2p_plms_step(ctypes.byref(_args(kw)), None) == code


def test_plms_step_rejects_null_args():
    assert _hip.lib().p2p_plms_step(None, None) == -1
