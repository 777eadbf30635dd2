"""Direct Inversion (Ju et al. 2023, "Direct Inversion: Boosting Diffusion-based Editing with 3
Lines of Code", also known as PnP Inversion): real-image edits without null-text optimisation.

The DDIM inversion trajectory z*_0 ... z*_T is inverted with the source prompt at guidance 1, as
``NullInversion.ddim_loop`` does.  Then, for step i at timestep t_i, with z*_cur the trajectory
latent at t_i and z*_prev the next cleaner one,

    offset[i] = z*_prev - prev_step(eps_u + g (eps_c - eps_u), t_i, z*_cur)
    eps       = unet([z*_cur, z*_cur], t_i, [null, source])

and the edit loop adds offset[i] to the source row after step i (``ptp_utils.diffusion_step``'s
``latent_offset``): the source branch then reproduces z*_0 up to rounding, and the edited branches
see it through attention injection and LocalBlend as usual.  There is no optimisation and no
backward pass, so any U-Net dtype works (float16 too, which the attention backward of null-text
inversion refuses), and every offset's input comes from the stored trajectory: the steps do not
depend on each other, so ``steps_per_call`` timesteps share one U-Net call, each row with its own
timestep.

The method is restated from the paper; agreement with its published code (a fork of the
reference's ``null_text.py``) and image quality on real weights are not verified.
The paper's "add_target" ablation (offsets on the edited rows too) is not built.
"""
from __future__ import annotations

import torch

from .ddim import DDIMScheduler
from .null_text import GUIDANCE_SCALE, NUM_DDIM_STEPS, NullInversion, _GraphedForward, _rows_call, load_512


class DirectInversion(NullInversion):
    """``invert`` / ``invert_batch`` in about 2 x num_ddim_steps forward U-Net rows per image: the
    serial inversion loop, then the offsets pass, ``steps_per_call`` timesteps (times the images of
    a batch) per U-Net call.  The default of 4 keeps a single image's call at 8 rows, the most the
    U-Net's fused time path takes (unet.TIME_FUSED_MAX_ROWS).

    On the GPU with this library's DDIM scheduler and f32 latents, the inversion's next_step is
    p2p_latent_step with the inversion coefficients and a call's offsets are one p2p_direct_offset
    launch; with ``use_graphs`` the U-Net call of the loop and the whole offsets call (U-Net and
    kernel) replay captured graphs.  On the CPU, or with a scheduler object of the caller's own,
    the torch lines run.  Nothing here touches autograd."""

    def __init__(self, model, num_ddim_steps: int = NUM_DDIM_STEPS, guidance_scale: float = GUIDANCE_SCALE,
                 steps_per_call: int = 4, use_graphs: bool = True):
        super().__init__(model, num_ddim_steps, guidance_scale, use_graphs)    # (TypeError without prev_step / next_step)
        if int(steps_per_call) < 1:
            raise ValueError(f"steps_per_call must be at least 1, got {steps_per_call}")
        self.steps_per_call = int(steps_per_call)

    # ------------------------------------------------------------------ public
    def invert(self, image, prompt: str, offsets=(0, 0, 0, 0)):
        """``image``: a path, a uint8 array or a [1, 4, h, w] latent, as NullInversion.invert takes.
        Returns ((image_gt, image_rec), x_T, latent_offsets): latent_offsets f32
        [num_ddim_steps, 1, 4, h, w], index i belonging to scheduler.timesteps[i] -- the
        ``latent_offsets`` argument of ptp_utils.text2image_ldm_stable."""
        return self.invert_batch([image], [prompt], offsets)[0]

    def invert_batch(self, images, prompts, offsets=(0, 0, 0, 0)):
        """``invert`` for B images per U-Net call (there is no per-image state: the same code, with
        B times the rows).  ``images``: B paths, uint8 arrays or [1, 4, h, w] latents, or one
        [B, 4, h, w] latent tensor; ``prompts``: B strings.  Returns B tuples as ``invert``'s."""
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
        trajectory = self.ddim_loop(torch.cat(latents))
        offs = self.latent_offsets(trajectory)
        return [((images_gt[b], images_rec[b]), trajectory[-1][b:b + 1], offs[:, b:b + 1].contiguous())
                for b in range(B)]

    # ------------------------------------------------------------------ the two passes
    def _fused(self, latent) -> bool:
        dtype = getattr(self.model.unet, "dtype", None)
        return (latent.is_cuda and latent.dtype == torch.float32 and isinstance(self.scheduler, DDIMScheduler)
                and dtype in (torch.float32, torch.bfloat16, torch.float16))

    @torch.no_grad()
    def ddim_loop(self, latent):
        """NullInversion.ddim_loop (the trajectory [z*_0, ..., z*_T], inverted with the conditional
        rows of the context); on the GPU the U-Net call replays one graph and next_step is
        p2p_latent_step with DDIMScheduler.next_coeffs -- next_step's lines with the four factors
        computed on the host, bit for bit."""
        if not self._fused(latent):
            return super().ddim_loop(latent)
        from . import _hip
        unet, sched = self.model.unet, self.scheduler
        cond = self.context.chunk(2)[1]
        ts = sched.timesteps
        x = latent.clone().detach().contiguous()
        fwd = _GraphedForward(unet, x, cond, ts[len(ts) - 1]) if self.use_graphs else None
        trajectory = [latent]
        for i in range(self.num_ddim_steps):
            t = ts[len(ts) - i - 1]
            eps = fwd(x, t, cond) if fwd is not None else unet(x, t, encoder_hidden_states=cond)["sample"]
            x = _hip.latent_step(eps.contiguous(), x, torch.empty_like(x), sched.next_coeffs(t))
            trajectory.append(x)
        return trajectory

    @torch.no_grad()
    def latent_offsets(self, trajectory):
        """The offsets of a trajectory of ``ddim_loop`` ([B, 4, h, w] latents; the context of
        ``init_prompt`` / ``_init_prompts`` in place): f32 [num_ddim_steps, B, 4, h, w].  Steps
        i0 .. i0 + steps_per_call - 1 share one U-Net call of 2 x steps x B rows -- the null block
        first, row s * B + b of a block being step i0 + s of image b, with its own timestep -- and,
        on the GPU, one p2p_direct_offset launch with each row's prev_coeffs.  The last call may
        be short."""
        T, S = self.num_ddim_steps, self.steps_per_call
        if len(trajectory) != T + 1:
            raise ValueError(f"a trajectory of {len(trajectory)} latents for {T} steps")
        z0 = trajectory[0]
        B = z0.shape[0]
        dev = z0.device
        ts = [int(t) for t in self.scheduler.timesteps]
        null, cond = self.context.chunk(2)
        if null.shape[0] != B:
            raise ValueError(f"the context holds {null.shape[0]} prompts for {B} latents")
        fused = self._fused(z0)
        out = torch.empty((T, B, *z0.shape[1:]), dtype=torch.float32, device=dev)
        calls = {}          # rows per call -> the call (a graph, or the eager lines) and its context
        for i0 in range(0, T, S):
            steps = range(i0, min(i0 + S, T))
            n = len(steps)
            x = torch.cat([trajectory[T - i] for i in steps])
            target = torch.cat([trajectory[T - i - 1] for i in steps])
            t_rows = torch.tensor([ts[i] for i in steps], dtype=torch.int64).repeat_interleave(B)
            t2 = torch.cat([t_rows, t_rows]).to(dev)
            if n not in calls:
                ctx = torch.cat([null.repeat(n, 1, 1), cond.repeat(n, 1, 1)])
                calls[n] = ctx
                if fused:
                    from . import _hip
                    calls[n] = _rows_call(self.model.unet, self.guidance_scale, self.use_graphs, _hip.direct_offset,
                                          4, x, ctx, t2)
            if fused:
                coef = torch.tensor([self.scheduler.prev_coeffs(ts[i]) for i in steps], dtype=torch.float32)
                off = calls[n](x, target, t2, coef.repeat_interleave(B, 0).to(dev))
                out[i0:i0 + n] = off.reshape(n, B, *z0.shape[1:])
                continue
            eps = self.model.unet(torch.cat([x, x]), t2, encoder_hidden_states=calls[n])["sample"]
            eps_u, eps_c = eps.chunk(2)
            for k, i in enumerate(steps):
                rows = slice(k * B, (k + 1) * B)
                noise = eps_u[rows] + self.guidance_scale * (eps_c[rows] - eps_u[rows])
                out[i] = target[rows] - self.prev_step(noise, ts[i], x[rows])
        return out
