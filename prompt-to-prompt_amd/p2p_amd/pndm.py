"""PNDM scheduler in its PLMS form, the sampler main.py runs.

main.py:29 takes the Stable Diffusion v1.4 pipeline's own scheduler: diffusers' PNDMScheduler with
``skip_prk_steps`` (no Runge-Kutta warm-up: pseudo linear multistep from the first call) and
``steps_offset = 1``.  For n inference steps it makes n + 1 U-Net calls -- the second call is a
corrector at the timestep the first one stepped to -- which is why
``get_time_words_attention_alpha`` builds n + 1 rows (ptp_utils.py:280-297).

diffusers is external to the reference, so this module restates the method (Liu et al., "Pseudo
Numerical Methods for Diffusion Models on Manifolds", 2022, eq. 12 and the transfer of eq. 11); the
beta schedule and ``alphas_cumprod`` are ddim.py's.  Call c with the new model output E:

    c = 0     m = E0                                    sample kept, E0 stored
    c = 1     m = (E1 + E0) / 2                         stepped from the kept sample, t + r -> t,
                                                        E1 not stored
    c = 2     m = (3 E2 - E0) / 2
    c = 3     m = (23 E3 - 16 E2 + 5 E0) / 12
    c >= 4    m = (55 E_c - 59 E_{c-1} + 37 E_{c-2} - 9 E_{c-3}) / 24

    prev = sqrt(a_p / a_t) x - (a_p - a_t) m / (a_t sqrt(1 - a_p) + sqrt(a_t (1 - a_t) a_p))

which is the DDIM step (ddim.py prev_step) with m as the noise.

Arithmetic (the same on the CPU and the GPU, and what p2p_plms_step reproduces bit for bit): the
model output is cast to float32 on entry and the history is float32 (diffusers keeps both in the
U-Net's dtype; float64 inputs stay float64, for analysis on the CPU); the combination multiplies
by Python-float weights and sums the products left to right, newest first -- never
``tensor / python_scalar``, which torch computes as a multiplication by the reciprocal on the GPU
and as a division on the CPU; the three transfer scalars are 0-dim tensors computed on the CPU
from ``alphas_cumprod`` and moved to the sample's device, and the transfer is
``sample_coeff * x - (num * m) / den``.  ``plan_step`` makes every host decision of a call; the
eager ``step`` and the fused latent step (ptp_utils._fused_latent_step) both execute its plan.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .ddim import _Config

# w[0] for the new model output, then the stored ones, newest first
_WEIGHTS = {0: (1.0,), 1: (3 / 2, -1 / 2), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
_CORRECTOR = (1 / 2, 1 / 2)
RING = 4    # history buffers of the fused path: three read and one written per call


class StepPlan(NamedTuple):
    """One call's host decisions."""
    weights: Tuple[float, ...]   # w[0] for the new model output, w[1:] for the history entries used
    n_hist: int                  # stored outputs read, newest first (len(weights) - 1)
    sample_coeff: float          # the transfer's three scalars (f32 values)
    eps_num: float
    eps_den: float
    append: bool                 # the new model output is stored
    from_kept: bool              # stepped from the sample kept at call 0 (the corrector call)
    keep_sample: bool            # call 0: this call's sample is kept by reference


class PNDMScheduler:
    def __init__(self, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000,
                 set_alpha_to_one=False, skip_prk_steps=True, steps_offset=1):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError(beta_schedule)
        if not skip_prk_steps:
            raise NotImplementedError("skip_prk_steps=False (the Runge-Kutta warm-up)")
        self.config = _Config(num_train_timesteps)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.steps_offset = steps_offset
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self._reset()

    def _reset(self):
        self.ets = []            # stored model outputs (f32), oldest first, at most four
        self.counter = 0
        self.cur_sample = None
        self._ring = None        # the fused path's history buffers [RING, B, C, H, W]

    def set_timesteps(self, num_inference_steps: int):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round().astype(np.int64) + self.steps_offset
        # the second-to-last timestep twice: the corrector call (n + 1 U-Net calls for n steps)
        ts = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()
        self.timesteps = torch.from_numpy(ts)
        self._reset()

    # ------------------------------------------------------------------ the plan of one call
    def _transfer(self, t_from: int, t_to: int):
        """(sample_coeff, a_p - a_t, denominator) of the step a_t -> a_p as 0-dim CPU tensors in
        ``alphas_cumprod``'s dtype."""
        a_t = self.alphas_cumprod[t_from]
        a_p = self.alphas_cumprod[t_to] if t_to >= 0 else self.final_alpha_cumprod
        sample_coeff = (a_p / a_t) ** 0.5
        den = a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5
        return sample_coeff, a_p - a_t, den

    def plan_step(self, timestep) -> StepPlan:
        """Every host decision of the next ``step`` call at ``timestep`` (no state changes)."""
        if self.num_inference_steps is None:
            raise RuntimeError("PNDMScheduler: call set_timesteps first")
        c, t = self.counter, int(timestep)
        r = self.config.num_train_timesteps // self.num_inference_steps
        stored = min(len(self.ets), 3)
        # E0 after call 0, nothing from the corrector, then one per call, the last four kept
        if len(self.ets) != (c if c < 2 else min(c - 1, 4)):
            raise RuntimeError(f"PNDMScheduler: call {c} with {len(self.ets)} stored outputs (set_timesteps resets)")
        if c == 1:      # the corrector repeats call 0's step with the averaged output
            weights, t_from, t_to = _CORRECTOR, t + r, t
        else:
            weights, t_from, t_to = _WEIGHTS[stored], t, t - r
        sc, num, den = (float(v) for v in self._transfer(t_from, t_to))
        return StepPlan(weights, len(weights) - 1, sc, num, den, append=c != 1, from_kept=c == 1, keep_sample=c == 0)

    def history(self, plan: StepPlan):
        """The stored outputs ``plan`` reads, newest first."""
        return tuple(self.ets[-1 - i] for i in range(plan.n_hist))

    def step_source(self, plan: StepPlan, sample):
        """The sample ``plan`` steps from."""
        return self.cur_sample if plan.from_kept else sample

    def history_slot(self, plan: StepPlan, like: torch.Tensor) -> Optional[torch.Tensor]:
        """Where the fused path writes the new model output (None on the corrector call): a buffer
        of the scheduler's ring that none of the outputs ``plan`` reads occupies.  The ring is
        allocated at the first call after set_timesteps (under capture: from the graph's pool)."""
        if not plan.append:
            return None
        if self._ring is None or self._ring.shape[1:] != like.shape or self._ring.device != like.device:
            self._ring = torch.empty((RING,) + tuple(like.shape), dtype=torch.float32, device=like.device)
        busy = {h.data_ptr() for h in self.ets[-3:]}
        return next(buf for buf in self._ring if buf.data_ptr() not in busy)

    def commit(self, plan: StepPlan, model_output_f32, sample):
        """The state change of a call: ``model_output_f32`` is the stored output (eager: the cast
        model output; fused: the history_slot buffer the kernel filled)."""
        if plan.append:
            self.ets = self.ets[-3:] + [model_output_f32]
        if plan.keep_sample:
            self.cur_sample = sample
        elif plan.from_kept:
            self.cur_sample = None
        self.counter += 1

    # ------------------------------------------------------------------ the eager step
    def step(self, model_output, timestep, sample, **kw):
        plan = self.plan_step(timestep)
        work = torch.float64 if model_output.dtype == torch.float64 else torch.float32
        e = model_output.to(work)
        x = self.step_source(plan, sample)
        m = plan.weights[0] * e
        for w, h in zip(plan.weights[1:], self.history(plan)):
            m = m + w * h
        sc, num, den = (torch.tensor(v, dtype=work).to(x.device)
                        for v in (plan.sample_coeff, plan.eps_num, plan.eps_den))
        prev = sc * x - (num * m) / den
        self.commit(plan, e, sample)
        return {"prev_sample": prev}
