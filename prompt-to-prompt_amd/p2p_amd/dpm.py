"""DPM-Solver++ (2M): the second-order multistep solver in its data-prediction form.

diffusers 0.8.1 (the version the reference's requirements.txt pins) ships it as
DPMSolverMultistepScheduler, and the reference's diffusion_step only calls
``model.scheduler.step(noise_pred, t, latents)["prev_sample"]`` (ptp_utils.py:74), so users swap it
in and sample in 20-25 U-Net calls instead of 50.  diffusers is external to the reference and not
available offline, so this module restates the method from the paper (Lu et al., "DPM-Solver++:
Fast Solver for Guided Sampling of Diffusion Probabilistic Models", 2022, Algorithm 2: multistep,
data prediction) with diffusers' documented defaults (``algorithm_type="dpmsolver++"``,
``solver_type="midpoint"``, ``solver_order=2``, ``lower_order_final=True``); the beta schedule and
``alphas_cumprod`` are ddim.py's.  Agreement with diffusers' implementation is NOT verified; the
module is tested against the mathematics (tests/test_dpm.py: the DDIM step its first-order update
is, a constant data prediction, its order of accuracy on a closed form).

Grid: ``linspace(0, T - 1, n + 1).round()[::-1][:-1]`` -- n calls for n steps, no corrector call; the
call at the last timestep steps to timestep 0 (``alphas_cumprod[0]``, not a "final alpha" of 1).

A call at timestep s stepping to t, with a = sqrt(alphas_cumprod), sg = sqrt(1 - alphas_cumprod),
lambda = log a - log sg, h = lambda_t - lambda_s and e the (CFG-combined) model output:

    m0  = (x - sg_s e) / a_s                            the data prediction, stored (history)
    out = (sg_t / sg_s) x - a_t (exp(-h) - 1) m0        first order: the first call, every call of
                                                        solver_order 1, and the last call when
                                                        lower_order_final and n < 15
    out = ... - 1/2 a_t (exp(-h) - 1) (m0 - m1) / r0    second order (2M, midpoint): m1 the previous
                                                        call's m0, r0 = (lambda_s - lambda_s') / h,
                                                        s' the previous call's timestep

Arithmetic (the same on the CPU and the GPU, and what p2p_dpm_step reproduces bit for bit): the
model output is cast to float32 on entry and the history is float32 (float64 inputs stay float64,
for analysis on the CPU).  Every scalar is computed on the host in float64 (Python floats, ``math``)
from the ``alphas_cumprod`` entries -- exp(-h) - 1 as ``expm1(-h)`` -- and rounded once to the work
dtype, as a 0-dim tensor moved to the sample's device:

    sigma_s = sg_s      alpha_s = a_s      x_coeff = sg_t / sg_s      m0_coeff = a_t expm1(-h)
    diff_coeff = 1/2 a_t expm1(-h) / r0    (one host scalar)

and the tensor operations are, in this order, each rounded on its own,

    m0  = (x - sigma_s * e) / alpha_s                   the only division of tensors: one IEEE division
    out = x_coeff * x - m0_coeff * m0
    out = out - diff_coeff * (m0 - m1)                  second order only

``tensor / python_scalar`` never appears (pndm.py's docstring says why).  ``plan_step`` makes every
host decision of a call; the eager ``step`` and the fused latent step (ptp_utils._fused_latent_step)
both execute its plan.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .ddim import _Config

RING = 2    # history buffers of the fused path: one read and one written per call


class StepPlan(NamedTuple):
    """One call's host decisions (the scalars as Python floats, float64)."""
    n_hist: int          # 0: first-order update; 1: second-order, reads the previous call's m0
    sigma_s: float       # m0 = (x - sigma_s * e) / alpha_s
    alpha_s: float
    x_coeff: float       # sg_t / sg_s
    m0_coeff: float      # a_t expm1(-h)
    diff_coeff: float    # 1/2 a_t expm1(-h) / r0 (0.0 when n_hist == 0)
    store: bool          # this call's m0 is kept for the next call (False on the last call)
    t_from: int          # s
    t_to: int            # t


class DPMSolverMultistepScheduler:
    def __init__(self, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                 solver_order=2, lower_order_final=True, algorithm_type="dpmsolver++", solver_type="midpoint",
                 thresholding=False, prediction_type="epsilon"):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError(f"beta_schedule={beta_schedule!r}")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order!r}")
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}")
        if solver_type != "midpoint":
            raise NotImplementedError(f"solver_type={solver_type!r}")
        if thresholding:
            raise NotImplementedError("thresholding=True")
        if prediction_type != "epsilon":
            raise NotImplementedError(f"prediction_type={prediction_type!r}")
        self.config = _Config(num_train_timesteps)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.solver_order = solver_order
        self.lower_order_final = lower_order_final
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self._reset()

    def _reset(self):
        self.counter = 0
        self.m_prev = None       # the previous call's data prediction (f32)
        self._ring = None        # the fused path's history buffers [RING, B, C, H, W]

    def set_timesteps(self, num_inference_steps: int):
        self.num_inference_steps = num_inference_steps
        T = self.config.num_train_timesteps
        ts = np.linspace(0, T - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts)
        self._reset()

    # ------------------------------------------------------------------ the plan of one call
    def _alpha_sigma_lambda(self, t: int):
        ac = float(self.alphas_cumprod[t])
        a, sg = math.sqrt(ac), math.sqrt(1.0 - ac)
        return a, sg, math.log(a) - math.log(sg)

    def plan_step(self, timestep) -> StepPlan:
        """Every host decision of the next ``step`` call at ``timestep`` (no state changes)."""
        if self.num_inference_steps is None:
            raise RuntimeError("DPMSolverMultistepScheduler: call set_timesteps first")
        c, s, n = self.counter, int(timestep), self.num_inference_steps
        if c >= n or s != int(self.timesteps[c]) or (self.m_prev is None) != (c == 0):
            raise RuntimeError(f"DPMSolverMultistepScheduler: call {c} of {n} at timestep {s} is out of sequence "
                               f"(set_timesteps resets)")
        last = c == n - 1
        t = 0 if last else int(self.timesteps[c + 1])
        a_s, sg_s, lam_s = self._alpha_sigma_lambda(s)
        a_t, sg_t, lam_t = self._alpha_sigma_lambda(t)
        h = lam_t - lam_s
        m0_coeff = a_t * math.expm1(-h)
        first_order = c == 0 or self.solver_order == 1 or (last and self.lower_order_final and n < 15)
        diff_coeff = 0.0
        if not first_order:
            h0 = lam_s - self._alpha_sigma_lambda(int(self.timesteps[c - 1]))[2]
            diff_coeff = 0.5 * m0_coeff / (h0 / h)
        return StepPlan(0 if first_order else 1, sg_s, a_s, sg_t / sg_s, m0_coeff, diff_coeff, store=not last,
                        t_from=s, t_to=t)

    def history(self, plan: StepPlan):
        """The stored data predictions ``plan`` reads (none, or the previous call's)."""
        return (self.m_prev,) if plan.n_hist else ()

    def history_slot(self, plan: StepPlan, like: torch.Tensor) -> Optional[torch.Tensor]:
        """Where the fused path writes this call's data prediction (None on the last call): the
        buffer of the scheduler's ring of two that the previous call's does not occupy.  The ring is
        allocated at the first call after set_timesteps (under capture: from the graph's pool)."""
        if not plan.store:
            return None
        if self._ring is None or self._ring.shape[1:] != like.shape or self._ring.device != like.device:
            self._ring = torch.empty((RING,) + tuple(like.shape), dtype=torch.float32, device=like.device)
        busy = self.m_prev.data_ptr() if self.m_prev is not None else None
        return next(buf for buf in self._ring if buf.data_ptr() != busy)

    def commit(self, plan: StepPlan, m0):
        """The state change of a call: ``m0`` is this call's data prediction (eager: the tensor
        ``step`` computed; fused: the history_slot buffer the kernel filled; None on the last call)."""
        self.m_prev = m0 if plan.store else None
        self.counter += 1

    # ------------------------------------------------------------------ the eager step
    def step(self, model_output, timestep, sample, **kw):
        plan = self.plan_step(timestep)
        work = torch.float64 if model_output.dtype == torch.float64 else torch.float32
        e = model_output.to(work)
        x = sample
        sigma_s, alpha_s, x_coeff, m0_coeff, diff_coeff = (
            torch.tensor(v, dtype=work).to(x.device)
            for v in (plan.sigma_s, plan.alpha_s, plan.x_coeff, plan.m0_coeff, plan.diff_coeff))
        m0 = (x - sigma_s * e) / alpha_s
        prev = x_coeff * x - m0_coeff * m0
        for m1 in self.history(plan):
            prev = prev - diff_coeff * (m0 - m1)
        self.commit(plan, m0)
        return {"prev_sample": prev}
