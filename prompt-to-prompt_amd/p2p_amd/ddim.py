"""DDIM scheduler (eta = 0) with the configuration null_text.py:16-20 builds.

diffusers' DDIMScheduler is external to the reference; its deterministic step is restated
in the reference itself as ``NullInversion.prev_step`` (null_text.py:471-479) and the inverse
``next_step`` (:481-489), which this module follows (pinned by tests/golden/ddim.npz).
The beta schedule (``scaled_linear``: linspace(sqrt(b0), sqrt(b1), 1000) ** 2) and the
timestep grid (``arange(n) * (1000 // n)`` reversed, steps_offset 0) are diffusers
conventions -- parity unpinned beyond the reference's own restatement.

``step`` stays the deterministic one whatever ``eta`` it is handed.  The stochastic step (diffusers'
``step(eta=..., variance_noise=...)``) is ``ddpm_step`` with its factors in ``ddpm_coeffs``, restated
from the DDIM paper's sigma for the edit-friendly DDPM inversion (ddpm_inversion.py); parity with
diffusers is unpinned.
"""
from __future__ import annotations

import numpy as np
import torch


class _Config:
    def __init__(self, num_train_timesteps):
        self.num_train_timesteps = num_train_timesteps


class DDIMScheduler:
    def __init__(self, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                 set_alpha_to_one=False, num_train_timesteps=1000, steps_offset=0):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError(beta_schedule)
        if clip_sample:
            raise NotImplementedError("clip_sample")
        self.config = _Config(num_train_timesteps)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.steps_offset = steps_offset
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())

    def set_timesteps(self, num_inference_steps: int):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts + self.steps_offset)

    def _coeffs(self, t, t_other, device):
        a_t = self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod
        a_o = self.alphas_cumprod[t_other] if t_other >= 0 else self.final_alpha_cumprod
        return a_t.to(device), a_o.to(device)

    def prev_step(self, model_output, timestep, sample):
        """x_{t-Δ} from x_t (null_text.py:471-479)."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t, a_prev = self._coeffs(t, prev_t, sample.device)
        beta_t = 1 - a_t
        x0 = (sample - beta_t ** 0.5 * model_output) / a_t ** 0.5
        direction = (1 - a_prev) ** 0.5 * model_output
        return a_prev ** 0.5 * x0 + direction

    def next_step(self, model_output, timestep, sample):
        """x_{t} from x_{t-Δ} (DDIM inversion, null_text.py:481-489)."""
        t_next = int(timestep)
        t = min(t_next - self.config.num_train_timesteps // self.num_inference_steps, 999)
        a_t, a_next = self._coeffs(t, t_next, sample.device)
        beta_t = 1 - a_t
        x0 = (sample - beta_t ** 0.5 * model_output) / a_t ** 0.5
        direction = (1 - a_next) ** 0.5 * model_output
        return a_next ** 0.5 * x0 + direction

    def prev_coeffs(self, timestep):
        """The four 0-dim factors prev_step multiplies by, as host floats (for p2p_latent_step):
        (beta_t ** 0.5, a_t ** 0.5, a_prev ** 0.5, (1 - a_prev) ** 0.5), computed by the same
        f32 tensor ops as prev_step."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t, a_prev = self._coeffs(t, prev_t, torch.device("cpu"))
        return (float((1 - a_t) ** 0.5), float(a_t ** 0.5), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5))

    def next_coeffs(self, timestep):
        """The same factors for next_step (DDIM inversion)."""
        t_next = int(timestep)
        t = min(t_next - self.config.num_train_timesteps // self.num_inference_steps, 999)
        a_t, a_next = self._coeffs(t, t_next, torch.device("cpu"))
        return (float((1 - a_t) ** 0.5), float(a_t ** 0.5), float(a_next ** 0.5), float((1 - a_next) ** 0.5))

    def ddpm_coeffs(self, timestep, eta=1.0):
        """The five factors of the stochastic step (diffusers' DDIMScheduler.step with eta > 0) as host
        floats, for p2p_ddpm_step / p2p_ddpm_noise and ``ddpm_step``:
        (sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma) with
        sigma^2 = eta^2 (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev) -- computed in double from the
        f32 alphas_cumprod and rounded once each (as dpm.plan_step computes its factors), the
        direction term clamped at 0 before the root.  Where a_prev == a_t (the last step of this
        grid: t = 0 steps to final_alpha_cumprod = alphas_cumprod[0]) sigma is exactly 0."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t, a_prev = (float(a) for a in self._coeffs(t, prev_t, torch.device("cpu")))
        var = float(eta) ** 2 * (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
        five = ((1 - a_t) ** 0.5, a_t ** 0.5, a_prev ** 0.5, max(1 - a_prev - var, 0.0) ** 0.5, max(var, 0.0) ** 0.5)
        return tuple(float(np.float32(c)) for c in five)

    def ddpm_step(self, model_output, timestep, sample, variance_noise, eta=1.0):
        """x_{t-Δ} = mu(x_t, eps) + sigma * variance_noise: prev_step's lines with the five factors of
        ``ddpm_coeffs`` as 0-dim f32 tensors, the product first, then the sum -- the eager sequence
        p2p_ddpm_step equals bit for bit."""
        sigma = torch.tensor(self.ddpm_coeffs(timestep, eta)[4], dtype=torch.float32, device=sample.device)
        return self.ddpm_mean(model_output, timestep, sample, eta) + sigma * variance_noise.to(sample.device)

    def ddpm_mean(self, model_output, timestep, sample, eta=1.0):
        """mu of ``ddpm_step``: prev_step's lines with sqrt(1 - a_prev - sigma^2) as the direction factor."""
        c0, c1, c2, c3 = (torch.tensor(c, dtype=torch.float32, device=sample.device)
                          for c in self.ddpm_coeffs(timestep, eta)[:4])
        return c2 * ((sample - c0 * model_output) / c1) + c3 * model_output

    def step(self, model_output, timestep, sample, **kw):
        return {"prev_sample": self.prev_step(model_output, timestep, sample)}
