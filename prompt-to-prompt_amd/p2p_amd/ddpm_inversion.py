"""The edit-friendly DDPM noise space (Huberman-Spiegelglas, Kulikov, Michaeli, CVPR 2024, "An Edit
Friendly DDPM Noise Space: Inversion and Manipulations"; the inversion behind LEDITS and LEDITS++):
real-image edits through the stochastic (eta > 0) sampler, with the noise of every step extracted
from the image.

With the scheduler's grid t_0 > ... > t_{T-1}, a_i = alphas_cumprod[t_i], the five factors of
``DDIMScheduler.ddpm_coeffs`` at step i (c0 = sqrt(1 - a_t), c1 = sqrt(a_t), c2 = sqrt(a_prev),
c3' = sqrt(1 - a_prev - sigma_i^2), c4 = sigma_i) and

    mu_i(x, e) = c2 ((x - c0 e) / c1) + c3' e            e = eps_u + g (eps_c - eps_u)

the noisy levels are drawn independently from the image latent z0, from the clean end:

    level[T] = z0
    level[i] = sqrt(a_i) z0 + sqrt(1 - a_i) eps~_i       i = T-1 ... 0, eps~ ~ N(0, I) independent
    level[i] = level[i+1]                                where sigma_i == 0

and the noise maps are what the sampler would have had to draw to walk from level to level:

    z_i = (level[i+1] - mu_i(level[i], e_i)) / sigma_i   e_i = unet([level[i]] * 2, t_i, [null, source])
    z_i = 0                                              where sigma_i == 0

The edit starts every row from level[skip] and runs x <- mu_i(x, e) + sigma_i z_i for i = skip ...
T-1 (``ptp_utils.text2image_ldm_stable(latent_noise=..., first_step=skip)``): the source row then
reproduces z0 up to rounding, and every edited row shares its noise realisation, which is what keeps
the structure; attention injection and LocalBlend act on top (the noise goes in before the blend).
On this scheduler's grid the last step runs at t = 0 with a_prev == a_t, so sigma_{T-1} is exactly
0 at every T: the rule above makes that step the deterministic one, from level[T-1] = z0's level.

Every level comes from z0 alone, so there is no serial loop and no backward pass: the steps are
independent, ``steps_per_call`` of them share one U-Net call, and any U-Net dtype works.

The method is restated from the paper; agreement with its published code and image quality on real
weights are not verified.  The published code reassigns level[i+1] := mu + sigma z
after each step -- an identity in exact arithmetic -- which is left out here so that the steps stay
independent.  Not built: per-prompt guidance scales (the paper's 3.5 for the source and 15 for the
edit; one ``guidance_scale`` serves both here), and fresh-noise stochastic sampling without an
inversion.
"""
from __future__ import annotations

import torch

from .ddim import DDIMScheduler
from .null_text import GUIDANCE_SCALE, NUM_DDIM_STEPS, NullInversion, _rows_call, load_512


class DDPMInversion(NullInversion):
    """``invert`` / ``invert_batch`` in num_ddim_steps - skip pairs of forward U-Net rows per image,
    ``steps_per_call`` timesteps (times the images of a batch) per U-Net call; the default of 4 keeps
    a single image's call at 8 rows, the most the U-Net's fused time path takes.

    On the GPU with this library's DDIM scheduler and f32 latents a call's noise maps are one
    p2p_ddpm_noise launch, each row with its own five factors; with ``use_graphs`` the U-Net call
    and the kernel replay one captured graph per call size.  On the CPU, or with a scheduler object
    of the caller's own (it needs ``ddpm_coeffs`` / ``ddpm_mean``), the torch lines run.  Nothing
    here touches autograd."""

    def __init__(self, model, num_ddim_steps: int = NUM_DDIM_STEPS, guidance_scale: float = GUIDANCE_SCALE,
                 eta: float = 1.0, skip: int = 0, steps_per_call: int = 4, use_graphs: bool = True):
        super().__init__(model, num_ddim_steps, guidance_scale, use_graphs)    # (TypeError without prev_step / next_step)
        if not hasattr(model.scheduler, "ddpm_coeffs"):
            raise TypeError(f"DDPMInversion needs a DDIM scheduler with ddpm_coeffs / prev_step: "
                            f"{type(model.scheduler).__name__} has none")
        if not float(eta) > 0:
            raise ValueError(f"eta must be positive (the noise maps divide by sigma), got {eta}")
        if not 0 <= int(skip) < num_ddim_steps:
            raise ValueError(f"skip must be in 0 .. {num_ddim_steps - 1}, got {skip}")
        if int(steps_per_call) < 1:
            raise ValueError(f"steps_per_call must be at least 1, got {steps_per_call}")
        self.eta, self.skip, self.steps_per_call = float(eta), int(skip), int(steps_per_call)

    # ------------------------------------------------------------------ public
    def invert(self, image, prompt: str, offsets=(0, 0, 0, 0), generator=None):
        """``image``: a path, a uint8 array or a [1, 4, h, w] latent, as NullInversion.invert takes.
        Returns ((image_gt, image_rec), x_start, noise_maps): x_start [1, 4, h, w] is level[skip],
        the ``latent`` of the edit; noise_maps [num_ddim_steps, 1, 4, h, w] in the latent's dtype
        (f32), index i belonging to scheduler.timesteps[i], zeros below ``skip`` -- the
        ``latent_noise`` argument of ptp_utils.text2image_ldm_stable, with ``first_step=skip``."""
        return self.invert_batch([image], [prompt], offsets, generator)[0]

    def invert_batch(self, images, prompts, offsets=(0, 0, 0, 0), generator=None):
        """``invert`` for B images per U-Net call.  ``images``: B paths, uint8 arrays or [1, 4, h, w]
        latents, or one [B, 4, h, w] latent tensor; ``prompts``: B strings.  ``generator`` draws
        the levels' noise, [num_ddim_steps, B, 4, h, w] at once on the CPU (as init_latent draws
        x_T).  Returns B tuples as ``invert``'s."""
        if torch.is_tensor(images) and images.dim() == 4:
            images = [images[b:b + 1] for b in range(images.shape[0])]
        images, prompts = list(images), list(prompts)
        B = len(images)
        if B == 0 or len(prompts) != B:
            raise ValueError(f"invert_batch: {B} images for {len(prompts)} prompts")
        images_gt = [load_512(im, *offsets) if isinstance(im, str) else im for im in images]
        latents = [self.image2latent(im) for im in images_gt]
        if any(x.shape != latents[0].shape or x.shape[0] != 1 for x in latents):
            raise ValueError(f"invert_batch: the latents must share one size, got {[tuple(x.shape) for x in latents]}")
        from . import ptp_utils
        self._init_prompts(prompts)
        ptp_utils.register_attention_control(self.model, None)
        images_rec = [self.latent2image(x) for x in latents]
        levels = self.noisy_levels(torch.cat(latents), generator)
        maps = self.noise_maps(levels)
        return [((images_gt[b], images_rec[b]), levels[self.skip][b:b + 1].contiguous(), maps[:, b:b + 1].contiguous())
                for b in range(B)]

    # ------------------------------------------------------------------ the two halves
    def _coeffs(self, i):
        return self.scheduler.ddpm_coeffs(int(self.scheduler.timesteps[i]), self.eta)

    @torch.no_grad()
    def noisy_levels(self, z0, generator=None):
        """[level[0], ..., level[T]] for the image latents z0 [B, 4, h, w] (entries below ``skip``:
        None, not computed; the noise of all T steps is drawn whatever ``skip`` is, so a level does
        not depend on it)."""
        T = self.num_ddim_steps
        noise = torch.randn((T, *z0.shape), generator=generator, dtype=z0.dtype).to(z0.device)
        levels = [None] * T + [z0]
        for i in range(T - 1, self.skip - 1, -1):
            c0, c1, _, _, sigma = self._coeffs(i)
            if sigma == 0:
                levels[i] = levels[i + 1]
                continue
            c0, c1 = (torch.tensor(c, dtype=torch.float32, device=z0.device) for c in (c0, c1))
            levels[i] = c1 * z0 + c0 * noise[i]
        return levels

    def _fused(self, latent) -> bool:
        dtype = getattr(self.model.unet, "dtype", None)
        return (latent.is_cuda and latent.dtype == torch.float32 and isinstance(self.scheduler, DDIMScheduler)
                and dtype in (torch.float32, torch.bfloat16, torch.float16))

    @torch.no_grad()
    def noise_maps(self, levels):
        """The maps of ``noisy_levels``' output (the context of ``init_prompt`` / ``_init_prompts`` in
        place): [num_ddim_steps, B, 4, h, w], zeros below ``skip``.  Steps i0 .. i0 + steps_per_call
        - 1 share one U-Net call of 2 x steps x B rows -- the null block first, row s * B + b of a
        block being step i0 + s of image b, with its own timestep -- and, on the GPU, one
        p2p_ddpm_noise launch with each row's ddpm_coeffs.  The last call may be short."""
        T, S = self.num_ddim_steps, self.steps_per_call
        if len(levels) != T + 1:
            raise ValueError(f"{len(levels)} levels for {T} steps")
        z0 = levels[T]
        B = z0.shape[0]
        dev = z0.device
        ts = [int(t) for t in self.scheduler.timesteps]
        null, cond = self.context.chunk(2)
        if null.shape[0] != B:
            raise ValueError(f"the context holds {null.shape[0]} prompts for {B} latents")
        fused = self._fused(z0)
        out = torch.zeros((T, B, *z0.shape[1:]), dtype=z0.dtype, device=dev)
        calls = {}          # rows per call -> the call (a graph, or the eager lines) and its context
        for i0 in range(self.skip, T, S):
            steps = range(i0, min(i0 + S, T))
            n = len(steps)
            x = torch.cat([levels[i] for i in steps])
            target = torch.cat([levels[i + 1] for i in steps])
            t_rows = torch.tensor([ts[i] for i in steps], dtype=torch.int64).repeat_interleave(B)
            t2 = torch.cat([t_rows, t_rows]).to(dev)
            if n not in calls:
                ctx = torch.cat([null.repeat(n, 1, 1), cond.repeat(n, 1, 1)])
                calls[n] = ctx
                if fused:
                    from . import _hip
                    calls[n] = _rows_call(self.model.unet, self.guidance_scale, self.use_graphs, _hip.ddpm_noise,
                                          5, x, ctx, t2)
            if fused:
                coef = torch.tensor([self._coeffs(i) for i in steps], dtype=torch.float32)
                z = calls[n](x, target, t2, coef.repeat_interleave(B, 0).to(dev))
                out[i0:i0 + n] = z.reshape(n, B, *z0.shape[1:])
                continue
            eps = self.model.unet(torch.cat([x, x]), t2, encoder_hidden_states=calls[n])["sample"]
            eps_u, eps_c = eps.chunk(2)
            for k, i in enumerate(steps):
                sigma = self._coeffs(i)[4]
                if sigma == 0:
                    continue                                    # (out is zeros)
                rows = slice(k * B, (k + 1) * B)
                e = eps_u[rows] + self.guidance_scale * (eps_c[rows] - eps_u[rows])
                mu = self.scheduler.ddpm_mean(e, ts[i], x[rows], self.eta)
                out[i] = (target[rows] - mu) / torch.tensor(sigma, dtype=torch.float32, device=dev)
        return out
