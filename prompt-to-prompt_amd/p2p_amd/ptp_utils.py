"""Drop-in for the reference ``ptp_utils.py``: the attention hook, the sampling loop and the
word/time tables.

``register_attention_control(model, controller)`` keeps the reference's patching rule
(every module whose class is named ``CrossAttention`` under ``unet.{down,mid,up}*``,
ptp_utils.py:223-240) and its forward signature (``:183``), and sets
``controller.num_att_layers`` (``:242``).  The replacement forward keeps the projections as
they are and hands ``q, k, v`` to the controller's fused kernel (controllers.py) -- or, for a
reference-style controller, to the materialised protocol (attention.py).
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from .attention import materialized_attention, plain_attention
from .ptp_words import get_time_words_attention_alpha, get_word_inds, update_alpha_time_word  # noqa: F401


# ------------------------------------------------------------------ figures
def text_under_image(image: np.ndarray, text: str, text_color: Tuple[int, int, int] = (0, 0, 0)):
    """ptp_utils.py:24-34: ``image`` [h, w, c] on a white canvas with a band of int(0.2 h) rows under
    it that carries ``text``.  With cv2 the text is drawn as the reference draws it (Hershey simplex,
    scale 1, thickness 2); without it, centred in the band in PIL's default font."""
    h, w, c = image.shape
    offset = int(h * .2)
    img = np.ones((h + offset, w, c), dtype=np.uint8) * 255
    img[:h] = image
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        font = cv2.FONT_HERSHEY_SIMPLEX
        textsize = cv2.getTextSize(text, font, 1, 2)[0]
        text_x, text_y = (w - textsize[0]) // 2, h + offset - textsize[1] // 2
        cv2.putText(img, text, (text_x, text_y), font, 1, text_color, 2)
        return img
    from PIL import Image, ImageDraw, ImageFont
    band = Image.fromarray(np.ascontiguousarray(img[h:]))
    draw = ImageDraw.Draw(band)
    font = ImageFont.load_default()
    left, top, right, bottom = draw.textbbox((0, 0), text, font=font)
    pos = ((w - (right - left)) // 2 - left, (offset - (bottom - top)) // 2 - top)
    draw.text(pos, text, fill=tuple(text_color)[:c] if c > 1 else text_color[0], font=font)
    img[h:] = np.asarray(band).reshape(offset, w, c)
    return img


def view_images(images, num_rows=1, offset_ratio=0.02):
    """ptp_utils.py:37-62: the images (a list, an array [n, h, w, 3] or one image) as one white grid
    of ``num_rows`` rows, int(h * offset_ratio) pixels apart, with the reference's padding rule
    (len % num_rows white cells are appended).  Returns the PIL image; it is displayed only where
    IPython is installed (a notebook), and never through ``Image.show()``."""
    from PIL import Image
    if type(images) is list:
        num_empty = len(images) % num_rows
    elif images.ndim == 4:
        num_empty = images.shape[0] % num_rows
    else:
        images = [images]
        num_empty = 0

    empty_images = np.ones(images[0].shape, dtype=np.uint8) * 255
    images = [image.astype(np.uint8) for image in images] + [empty_images] * num_empty
    num_items = len(images)

    h, w, c = images[0].shape
    offset = int(h * offset_ratio)
    num_cols = num_items // num_rows
    image_ = np.ones((h * num_rows + offset * (num_rows - 1),
                      w * num_cols + offset * (num_cols - 1), 3), dtype=np.uint8) * 255
    for i in range(num_rows):
        for j in range(num_cols):
            image_[i * (h + offset): i * (h + offset) + h:, j * (w + offset): j * (w + offset) + w] = images[
                i * num_cols + j]

    pil_img = Image.fromarray(image_)
    try:
        from IPython.display import display
    except ImportError:
        display = None
    if display is not None:
        display(pil_img)
    return pil_img


# ------------------------------------------------------------------ sampling loop
def diffusion_step(model, controller, latents, context, t, guidance_scale, low_resource=False, t_unet=None,
                   latent_offset=None, latent_noise=None, eta=1.0):
    """One CFG denoising step (ptp_utils.py:65-76).  With this library's DDIM, PNDM or DPM-Solver++
    scheduler and a controller whose step_callback is its own, the CFG combine, the scheduler's step and
    LocalBlend's latent blend run as one HIP kernel (p2p_latent_step / p2p_plms_step / p2p_dpm_step) --
    same result, bit for bit.
    ``t_unet``: the same timestep as a device tensor for the U-Net (a captured step must not copy
    a host timestep to the device); the scheduler keeps reading the host ``t``.
    ``latent_offset``: Direct Inversion's offset of this step (direct_inversion.py), [G, 4, h, w] for
    the G prompt groups of the batch (G = 1: one source prompt), added to each group's source row
    after step_callback -- in the same launch (p2p_direct_step) where the fused DDIM step applies,
    by add_latent_offset otherwise (low_resource, a controller with its own step_callback).
    ``latent_noise``: the DDPM inversion's noise map of this step (ddpm_inversion.py), [G, 4, h, w]:
    the step becomes the stochastic one at ``eta`` (DDIMScheduler.ddpm_step) with group g's map as the
    variance noise of every row of the group, added BEFORE step_callback -- in the same launch
    (p2p_ddpm_step) where the fused DDIM step applies, by scheduler.ddpm_step otherwise.  DDIM
    only; not together with ``latent_offset``."""
    if latent_noise is not None:
        if latent_offset is not None:
            raise ValueError("latent_noise (DDPM inversion) and latent_offset (Direct Inversion) are two methods: "
                             "pass one of them")
        if not (float(eta) > 0):
            raise ValueError(f"eta must be positive with latent_noise, got {eta}")
        if not hasattr(model.scheduler, "ddpm_step"):
            raise TypeError(f"latent_noise needs the DDIM scheduler: {type(model.scheduler).__name__} has no "
                            f"prev_step / ddpm_step (build the model with scheduler='ddim')")
        if latent_noise.dim() != 4 or latents.shape[0] % latent_noise.shape[0] or \
                latent_noise.shape[1:] != latents.shape[1:]:
            raise ValueError(f"latent_noise {tuple(latent_noise.shape)} for latents {tuple(latents.shape)}: "
                             f"[groups, C, H, W] with a batch of whole groups")
    tu = t if t_unet is None else t_unet
    if low_resource:
        eps_u = model.unet(latents, tu, encoder_hidden_states=context[0])["sample"]
        eps_c = model.unet(latents, tu, encoder_hidden_states=context[1])["sample"]
        eps = None
    else:
        eps = model.unet(torch.cat([latents] * 2), tu, encoder_hidden_states=context)["sample"]
        eps_u, eps_c = eps.chunk(2)
    if latent_noise is not None:
        fused = None if low_resource else _fused_latent_step(model, controller, eps, eps_u, eps_c, latents, t,
                                                             guidance_scale, None, latent_noise, eta)
        if fused is not None:
            return fused
        noise_pred = eps_u + guidance_scale * (eps_c - eps_u)
        G = latent_noise.shape[0]
        z = latent_noise.to(latents.device).repeat_interleave(latents.shape[0] // G, 0)
        return controller.step_callback(model.scheduler.ddpm_step(noise_pred, t, latents, z, eta))
    if latent_offset is None:
        fused = _fused_latent_step(model, controller, eps, eps_u, eps_c, latents, t, guidance_scale)
    else:
        if latent_offset.dim() != 4 or latents.shape[0] % latent_offset.shape[0] or \
                latent_offset.shape[1:] != latents.shape[1:]:
            raise ValueError(f"latent_offset {tuple(latent_offset.shape)} for latents {tuple(latents.shape)}: "
                             f"[groups, C, H, W] with a batch of whole groups")
        fused = None if low_resource else _fused_latent_step(model, controller, eps, eps_u, eps_c, latents, t,
                                                             guidance_scale, latent_offset)
    if fused is not None:
        return fused
    noise_pred = eps_u + guidance_scale * (eps_c - eps_u)
    latents = model.scheduler.step(noise_pred, t, latents)["prev_sample"]
    if latent_offset is None:
        return controller.step_callback(latents)
    return add_latent_offset(controller.step_callback(latents), latent_offset)


def add_latent_offset(latents, latent_offset):
    """Direct Inversion's three lines for G prompt groups: ``latent_offset`` [G, 4, h, w] added to the
    first (source) row of each group of latents.shape[0] / G rows, the other rows as they are.  With
    G = 1: torch.cat([latents[:1] + latent_offset, latents[1:]])."""
    G = latent_offset.shape[0]
    x = latents.reshape(G, latents.shape[0] // G, *latents.shape[1:])
    off = latent_offset.to(latents.device)
    return torch.cat([x[:, :1] + off[:, None], x[:, 1:]], dim=1).reshape(latents.shape)


def _fused_latent_step(model, controller, eps, eps_u, eps_c, latents, t, guidance_scale, latent_offset=None,
                       latent_noise=None, eta=1.0):
    from .ddim import DDIMScheduler
    from .dpm import DPMSolverMultistepScheduler
    from .pndm import PNDMScheduler
    sched = model.scheduler
    if not (isinstance(sched, (DDIMScheduler, PNDMScheduler, DPMSolverMultistepScheduler)) and latents.is_cuda
            and latents.dtype == torch.float32 and eps_u.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and hasattr(controller, "fused_step_mask")):
        return None
    if latent_offset is not None and not (isinstance(sched, DDIMScheduler) and latent_offset.is_cuda
                                          and latent_offset.dtype == torch.float32):
        return None         # (Direct Inversion is a DDIM method; other operands take the eager add)
    if latent_noise is not None and not (isinstance(sched, DDIMScheduler) and latent_noise.is_cuda
                                         and latent_noise.dtype == torch.float32):
        return None         # (a scheduler object of the caller's own, other operands: scheduler.ddpm_step)
    ok, mask_fn = controller.fused_step_mask()
    if not ok:
        return None
    if eps is None or not eps.is_contiguous():
        eps = torch.cat([eps_u, eps_c]).contiguous()
    x = latents.contiguous()
    out = torch.empty_like(x)
    plms, dpm = isinstance(sched, PNDMScheduler), isinstance(sched, DPMSolverMultistepScheduler)
    if plms:
        # the call's plan (pndm.plan_step, which the eager step executes too): the sample it steps
        # from -- call 0's on the corrector call, kept by reference, hence the fresh ``out`` -- the
        # stored model outputs it reads and the ring buffer that receives this call's
        plan = sched.plan_step(t)
        src = sched.step_source(plan, x).contiguous()
        hist, hist_out = sched.history(plan), sched.history_slot(plan, x)
    elif dpm:
        # dpm.plan_step likewise: the previous call's data prediction, if the plan reads it, and the
        # ring buffer that receives this call's
        plan = sched.plan_step(t)
        src, hist, hist_out = x, sched.history(plan), sched.history_slot(plan, x)
    else:
        plan, src, hist, hist_out = None, x, (), None
    _launch_latent_step(sched, mask_fn, eps, x, src, out, t, guidance_scale, plan, hist, hist_out, latent_offset,
                        latent_noise, eta)
    if plms:
        sched.commit(plan, hist_out, x)
    elif dpm:
        sched.commit(plan, hist_out)
    return out


def _launch_latent_step(sched, mask_fn, eps, x, src, out, t, guidance_scale, plan, hist, hist_out, offset=None,
                        noise=None, eta=1.0):
    """The step's mask (mask_fn's side effects included) and the one p2p_latent_step / p2p_plms_step /
    p2p_dpm_step launch (``plan``: the PLMS or DPM-Solver++ call's plan, None for DDIM) that reads it.
    ``offset`` (DDIM only): Direct Inversion's [groups, C, H, W] rows, added by p2p_direct_step;
    ``noise`` (DDIM only, instead of it): the DDPM inversion's rows, added by p2p_ddpm_step at ``eta``."""
    from . import _hip
    from . import dpm as dpm_mod
    from .controllers import FoldedBlendMask, StepMask, as_mask, group_mask_tensor
    size = tuple(x.shape[2:])
    step = mask_fn(size) if mask_fn is not None else StepMask([None], 0)
    if not isinstance(step, StepMask):     # a controller of the caller's own may return its one entry bare
        step = StepMask([step], 0)
    entries, group_size = step
    mask, group_blend, blend = None, None, None
    blending = [e for e in entries if e is not None]
    kept = hist + ((hist_out,) if hist_out is not None else ())
    rows = offset if offset is not None else noise     # the per-group operand of the step, if any
    if rows is not None:
        rows = rows.contiguous()
        kept = kept + (rows,)
    if not blending:
        # (the offsets alone still go to each group's first prompt, the noise to each group's rows)
        group_size = 0 if rows is None or rows.shape[0] == 1 else x.shape[0] // rows.shape[0]
    elif (all(isinstance(e, FoldedBlendMask) for e in blending) and len({e.latent_entry()[1:] for e in blending}) == 1
          and _blend_launch_ok(src, out, eps, blending[0], kept)):
        # every blending group folded, one threshold set: the masks are built inside the latent-step
        # launch (one launch per step for the whole batch)
        blend = [e.latent_entry() if e is not None else None for e in entries]
    elif group_size == 0:
        # a mask, or shapes the one-launch LocalBlend does not take: the mask is built by
        # p2p_localblend and the latent step reads it (the same mask, two launches)
        mask = as_mask(entries[0])
    else:
        mask, group_size, group_blend = group_mask_tensor(entries, group_size, size)
    if rows is not None:
        if rows.shape[0] != (x.shape[0] // group_size if group_size > 0 else 1):
            raise ValueError(f"{'latent_offset' if offset is not None else 'latent_noise'} has {rows.shape[0]} rows "
                             f"for a batch of {x.shape[0]} prompts in groups of {group_size or x.shape[0]}")
        if offset is None:
            return _hip.ddpm_step(eps, x, out, sched.ddpm_coeffs(t, eta), rows, guidance_scale, mask, group_size,
                                  group_blend, blend)
        return _hip.direct_step(eps, x, out, sched.prev_coeffs(t), rows, guidance_scale, mask, group_size,
                                group_blend, blend)
    if plan is None:
        return _hip.latent_step(eps, x, out, sched.prev_coeffs(t), guidance_scale, mask, group_size, group_blend, blend)
    launch = _hip.dpm_step if isinstance(plan, dpm_mod.StepPlan) else _hip.plms_step
    return launch(eps, src, out, plan, guidance_scale, mask, group_size, group_blend, blend, hist, hist_out)


def _blend_launch_ok(x, out, eps, folded, more=()) -> bool:
    """The one-launch LocalBlend's preconditions (p2p_latent.hip check_latent_args, include/p2p_hip.h):
    whole 4-pixel vectors (H*W % 4 == 0), 16-byte aligned x / out / eps (and ``more``: the PLMS
    or DPM-Solver++ history tensors), and a latent at least as large as the map resolution (the
    3x3-pooled map is nearest-upsampled onto it)."""
    H, W = x.shape[2], x.shape[3]
    res = int(round(folded.sums.shape[-1] ** 0.5))
    ptrs = x.data_ptr() | out.data_ptr() | eps.data_ptr()
    for t in more:
        ptrs |= t.data_ptr()
    return (H * W) % 4 == 0 and res <= H and res <= W and res * res <= 256 and ptrs % 16 == 0


def image_to_uint8(image: torch.Tensor) -> np.ndarray:
    """A decoder output [N, 3, H, W] (any float dtype) as the reference's uint8 ndarray [N, H, W, 3]
    (ptp_utils.py:82-85).  On the GPU one kernel (p2p_image_u8, the same bytes); the torch lines
    serve the CPU and the sizes the kernel does not take."""
    if image.is_cuda:
        from . import _hip
        out = _hip.image_u8(image.contiguous())
        if out is not None:
            return out.cpu().numpy()
    image = (image.float() / 2 + 0.5).clamp(0, 1)   # (.float(): numpy has no bfloat16)
    image = image.cpu().permute(0, 2, 3, 1).numpy()
    return (image * 255).astype(np.uint8)


def image_to_model(image, device, dtype) -> torch.Tensor:
    """uint8 pixels [H, W, 3] (or [N, H, W, 3]) as the VAE encoder's input [N, 3, H, W] in ``dtype``:
    x / 127.5 - 1 (null_text.py:523-525), on the GPU by p2p_image_to_model."""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(image)))
    if x.dim() == 3:
        x = x[None]
    device = torch.device(device)
    if device.type == "cuda" and x.dtype == torch.uint8:
        from . import _hip
        out = _hip.image_to_model(x.to(device), dtype)
        if out is not None:
            return out
    x = x.float() / 127.5 - 1
    return x.permute(0, 3, 1, 2).contiguous().to(device, dtype)   # dense NCHW, as the kernel writes it


def latent2image(vae, latents):
    """ptp_utils.py:79-85: decode, then uint8 [N, H, W, 3]."""
    latents = 1 / 0.18215 * latents
    image = vae.decode(latents)["sample"]
    return image_to_uint8(image)


def init_latent(latent, model, height, width, generator, batch_size):
    """ptp_utils.py:88-95: one x_T shared by every prompt of the group."""
    if latent is None:
        latent = torch.randn((1, model.unet.in_channels, height // 8, width // 8), generator=generator)
    latents = latent.expand(batch_size, model.unet.in_channels, height // 8, width // 8).to(model.device)
    return latent, latents


def _encode(model, prompts, encoder):
    ids = model.tokenizer(prompts, padding="max_length", max_length=model.tokenizer.model_max_length,
                          truncation=True, return_tensors="pt").input_ids
    return encoder(ids.to(model.device))[0]


def unet_context(model, context):
    """The context in the U-Net's own dtype, cast once before the sampling loop: a U-Net that
    casts ``encoder_hidden_states`` itself then gets back this same tensor at every step (a cast
    to its own dtype is a no-op), which keeps the cross-attention K / V cache of _cross_kv valid
    across steps."""
    dtype = getattr(model.unet, "dtype", None)
    if not isinstance(dtype, torch.dtype):
        return context
    if isinstance(context, (list, tuple)):
        return type(context)(c.to(dtype) for c in context)
    return context.to(dtype)


@torch.no_grad()
def text2image_ldm(model, prompt: List[str], controller, num_inference_steps: int = 50,
                   guidance_scale: Optional[float] = 7., generator: Optional[torch.Generator] = None,
                   latent: Optional[torch.FloatTensor] = None):
    """ptp_utils.py:98-126 (LDM-256: 32x32 latent, LDMBert context)."""
    register_attention_control(model, controller)
    height = width = 256
    batch_size = len(prompt)
    uncond = _encode(model, [""] * batch_size, model.bert)
    text = _encode(model, prompt, model.bert)
    latent, latents = init_latent(latent, model, height, width, generator, batch_size)
    context = unet_context(model, torch.cat([uncond, text]))
    model.scheduler.set_timesteps(num_inference_steps)
    for t in model.scheduler.timesteps:
        latents = diffusion_step(model, controller, latents, context, t, guidance_scale)
    image = latent2image(model.vqvae, latents) if getattr(model, "vqvae", None) is not None else latents
    return image, latent


@torch.no_grad()
def text2image_ldm_stable(model, prompt: List[str], controller, num_inference_steps: int = 50,
                          guidance_scale: float = 7.5, generator: Optional[torch.Generator] = None,
                          latent: Optional[torch.FloatTensor] = None, low_resource: bool = False,
                          uncond_embeddings=None, latent_offsets=None, latent_noise=None, eta: float = 1.0,
                          first_step: int = 0):
    """ptp_utils.py:129-172.  ``uncond_embeddings`` (per-step list or one tensor) is the
    argument the missing null-text notebook passes for the edit after inversion.
    ``latent_offsets`` (a tensor [steps, G, 4, h, w] or a per-step list of [G, 4, h, w]; G = 1 for
    one source prompt) is what DirectInversion.invert returns: step i's entry is added to the source
    row after that step (diffusion_step's ``latent_offset``).
    ``latent_noise`` (a tensor [steps, G, 4, h, w] or a per-step list of [G, 4, h, w]) is what
    DDPMInversion.invert returns: step i runs the stochastic step at ``eta`` with entry i as the
    variance noise of every row of its group (diffusion_step's ``latent_noise``).  ``first_step``: the
    loop runs timesteps[first_step:] (``latent`` is then the level the inversion returned for that
    ``skip``); latent_noise / latent_offsets / uncond_embeddings stay indexed by the absolute step,
    and the controller is the caller's, built for num_inference_steps - first_step steps.  With a VAE on
    the model (SyntheticStableDiffusion(vae=True)) the images come back as the reference returns
    them, uint8 [N, 512, 512, 3]; without one, the final latents in their place."""
    register_attention_control(model, controller)
    height = width = 512
    batch_size = len(prompt)
    text = _encode(model, prompt, model.text_encoder)
    if uncond_embeddings is None:
        uncond = _encode(model, [""] * batch_size, model.text_encoder)
    else:
        uncond = None
    latent, latents = init_latent(latent, model, height, width, generator, batch_size)
    model.scheduler.set_timesteps(num_inference_steps)
    # one context for the whole loop, as ptp_utils.py:158-160 builds it: the cross-attention K / V
    # projections of an unchanged context are then computed once (_project's cache); per-step null
    # embeddings make a new context every step
    context = None if uncond_embeddings is not None else unet_context(
        model, [uncond, text] if low_resource else torch.cat([uncond, text]))
    if latent_noise is not None and latent_offsets is not None:
        raise ValueError("latent_noise (DDPM inversion) and latent_offsets (Direct Inversion) are two methods: "
                         "pass one of them")
    if not 0 <= int(first_step) < num_inference_steps:
        raise ValueError(f"first_step must be in 0 .. {num_inference_steps - 1}, got {first_step}")
    for i, t in enumerate(model.scheduler.timesteps):
        if i < first_step:
            continue
        if uncond_embeddings is not None:
            u = uncond_embeddings[i] if isinstance(uncond_embeddings, (list, tuple)) else uncond_embeddings
            uncond = u.expand(*text.shape)
            context = [uncond, text] if low_resource else torch.cat([uncond, text])
        if latent_noise is not None:
            latents = diffusion_step(model, controller, latents, context, t, guidance_scale, low_resource,
                                     latent_noise=latent_noise[i].to(model.device), eta=eta)
        elif latent_offsets is None:
            latents = diffusion_step(model, controller, latents, context, t, guidance_scale, low_resource)
        else:
            latents = diffusion_step(model, controller, latents, context, t, guidance_scale, low_resource,
                                     latent_offset=latent_offsets[i].to(model.device))
    image = latent2image(model.vae, latents) if getattr(model, "vae", None) is not None else latents
    return image, latent


# ------------------------------------------------------------------ the hook
class DummyController:
    """ptp_utils.py:212-218: identity controller (used by null-text inversion)."""

    def __call__(self, *args):
        return args[0]

    def attention(self, q, k, v, heads, scale, is_cross, place_in_unet, mask=None):
        if mask is not None:
            return materialized_attention(self, q, k, v, heads, scale, is_cross, place_in_unet, mask)
        return plain_attention(q, k, v, heads, scale)

    def __init__(self):
        self.num_att_layers = 0


FUSE_PROJECTIONS = os.environ.get("P2P_FUSE_QKV", "1") != "0"


def _stacked_weight(module, names):
    """One [sum(out), in] weight for the bias-free projections ``names`` of ``module``
    (diffusers-0.8.1 CrossAttention's to_q/to_k/to_v carry no bias), rebuilt whenever a
    source weight is replaced or modified in place; None when they cannot be stacked."""
    mods = [getattr(module, n, None) for n in names]
    if not all(type(m) is torch.nn.Linear and m.bias is None for m in mods):
        return None
    key = tuple((m.weight.data_ptr(), m.weight._version, m.weight.dtype) for m in mods)
    cache = module.__dict__.setdefault("_p2p_stacked", {})
    hit = cache.get(names)
    if hit is None or hit[0] != key:
        hit = (key, torch.cat([m.weight.detach() for m in mods]))
        cache[names] = hit
    return hit[1]


CACHE_CROSS_KV = os.environ.get("P2P_CACHE_CROSS_KV", "1") != "0"


def _cross_kv(module, context, w):
    """linear(context, [to_k; to_v]) of a cross-attention, computed once per (context, weights):
    the sampling loop hands every U-Net call of an edit group the same context tensor
    (ptp_utils.py:158-168), so its K / V are the same at all 50 steps.  The cache holds the
    context by identity (a weak reference: a new tensor, even at a recycled address, misses) and
    its version counter (an in-place change misses), and the stacked weight object (rebuilt by
    _stacked_weight whenever a projection weight changes).  Not cached: inference-mode tensors (no
    version counter).
    Under stream capture an entry is made and hit only among captures: the first captured call
    records its GEMM in its graph (which recomputes K / V from the static context a replay has
    refilled, e.g. pipeline.GraphedEditRunner's step 0 or null-text's per-step uncond embeddings)
    and the later captured steps read that GEMM's output; an entry made eagerly is never hit by a
    capture (its K / V are of the context's content at that time, not at replay), and a captured
    entry never by an eager call (its K / V exist only once a replay ran).  The SHARED_KV row
    classes need a device read, so captured entries carry none."""
    import weakref
    if not CACHE_CROSS_KV or context.is_inference() or context.requires_grad:
        return torch.nn.functional.linear(context, w), None
    capturing = _capturing(context)
    hit = module.__dict__.get("_p2p_kv")
    if (hit is not None and hit[0]() is context and hit[1] == context._version and hit[2] is w
            and hit[5] == capturing):
        return hit[3], hit[4]
    kv = torch.nn.functional.linear(context, w)
    rows = None if capturing else kv_row_classes(kv)
    module.__dict__["_p2p_kv"] = (weakref.ref(context), context._version, w, kv, rows, capturing)
    return kv, rows


def _capturing(t) -> bool:
    """True while ``t``'s device stream is being captured into a HIP graph."""
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def kv_row_classes(kv):
    """For each batch row of a cross-attention's K / V projection, the first row of its run of
    bit-identical rows (rows n and n + 1 compared exactly) -- e.g. the uncond prompts "" of a group
    (ptp_utils.py:150-156) give equal context rows, hence equal K and V.  Computed once per cached
    projection (one device -> host read); the controllers turn it into p2p_group's SHARED_KV."""
    flat = kv.reshape(kv.shape[0], -1)
    same = (flat[1:] == flat[:-1]).all(dim=1).tolist()
    rows = [0]
    for i, eq in enumerate(same):
        rows.append(rows[-1] if eq else i + 1)
    return tuple(rows)


def _project(module, x, context, is_cross):
    """q, k, v of ptp_utils.py:186-193.  Outside autograd one GEMM produces them (x read once
    for self-attention, the context once for k and v) and the kernels read q/k/v as strided
    views of its output -- no head split copies (``[b,n,h*d] -> [b*h,n,d]``, :191-193).  A
    cross-attention's k / v of an unchanged context come from the previous call (_cross_kv)."""
    src = context if is_cross else x
    grad = torch.is_grad_enabled() and (x.requires_grad or src.requires_grad)
    if FUSE_PROJECTIONS and not grad and x.is_cuda:
        if is_cross:
            w = _stacked_weight(module, ("to_k", "to_v"))
            if w is not None:
                kv, rows = _cross_kv(module, src, w)
                C = kv.shape[-1] // 2
                k, v = kv[..., :C], kv[..., C:]
                if rows is not None:
                    k._p2p_rows = v._p2p_rows = rows   # (read by the controllers' group hints)
                return module.to_q(x), k, v
        else:
            w = _stacked_weight(module, ("to_q", "to_k", "to_v"))
            if w is not None:
                qkv = torch.nn.functional.linear(x, w)
                C = qkv.shape[-1] // 3
                return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    return module.to_q(x), module.to_k(src), module.to_v(src)


def _make_forward(module, place_in_unet, controller):
    to_out = module.to_out[0] if type(module.to_out) is torch.nn.modules.container.ModuleList else module.to_out
    attend = getattr(controller, "attention", None)

    def forward(x, context=None, mask=None, encoder_hidden_states=None, attention_mask=None):
        is_cross = context is not None          # only the ``context=`` kwarg counts (:187)
        q, k, v = _project(module, x, context, is_cross)
        if attend is not None:
            out = attend(q, k, v, module.heads, module.scale, is_cross, place_in_unet, mask)
        else:
            out = materialized_attention(controller, q, k, v, module.heads, module.scale, is_cross,
                                         place_in_unet, mask)
        return to_out(out)

    return forward


def register_attention_control(model, controller):
    if controller is None:
        controller = DummyController()

    def walk(net, count, place):
        if net.__class__.__name__ == "CrossAttention":
            net.forward = _make_forward(net, place, controller)
            return count + 1
        if hasattr(net, "children"):
            for child in net.children():
                count = walk(child, count, place)
        return count

    total = 0
    for name, net in model.unet.named_children():
        if "down" in name:
            total += walk(net, 0, "down")
        elif "up" in name:
            total += walk(net, 0, "up")
        elif "mid" in name:
            total += walk(net, 0, "mid")
    controller.num_att_layers = total
