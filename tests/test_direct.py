"""Direct Inversion (p2p_amd/direct_inversion.py, ptp_utils' latent_offset) and the argument checks of
p2p_direct_step / p2p_direct_offset -- CPU.

The reference of every test is the eager torch restatement of the two formulas, written here:

    offset[i] = z*_prev - prev_step(eps_u + g (eps_c - eps_u), t_i, z*_cur)
    latents   = cat(latents[:1] + offset[i], latents[1:])         after diffusion_step

The U-Net's attention runs on the GPU only, so the model here is a stub whose U-Net is elementwise
in the latent: eps = tanh(x s(t)) + c(ctx).  It is batch-invariant bit for bit and 1-Lipschitz in
x, and c("") and c(prompt) are far apart, so a guided step without offsets leaves the trajectory
at once.  (The same ordering check on a real tiny U-Net with null_text.LocalBlend is in
tests/test_gpu_direct.py.)
"""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

from p2p_amd import _hip, null_text, ptp_utils
from p2p_amd import pipeline as pl
from p2p_amd.direct_inversion import DirectInversion
from p2p_amd.tokenizer import default_tokenizer

E_ARG, E_DTYPE, E_BATCH, E_ALIGN = -1, -3, -5, -6
GUIDANCE = 7.5
STEPS = 10
SOURCE = "a painting of a squirrel eating a burger"
EDIT = "a painting of a lion eating a burger"


# ------------------------------------------------------------------ 1. header, binding, ABI, rejections
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "p2p_hip.h")).read()
    assert re.search(r"^int\s+p2p_direct_step\s*\(const p2p_direct_step_args\*", text, flags=re.M)
    assert re.search(r"^int\s+p2p_direct_offset\s*\(const p2p_direct_offset_args\*", text, flags=re.M)
    assert "#define P2P_ABI_VERSION 16" in text
    for name in ("p2p_direct_step", "p2p_direct_offset"):
        assert name in _hip.EXPORTED_SYMBOLS
        assert getattr(_hip.lib(), name) is not None
    assert _hip.lib().p2p_abi_version() == 16 == _hip.ABI_VERSION


def test_direct_step_args_are_the_latent_args_plus_offset():
    assert _hip.DirectStepArgs._fields_[:-1] == _hip.LatentArgs._fields_
    assert _hip.DirectStepArgs._fields_[-1][0] == "offset"
    for name, _ in _hip.LatentArgs._fields_:
        assert getattr(_hip.DirectStepArgs, name).offset == getattr(_hip.LatentArgs, name).offset


X, OUT, OFF = 1 << 20, 2 << 20, 3 << 20
ROW = 4 * 64 * 64 * 4            # bytes of one [4, 64, 64] f32 row


def _step(kw):
    a = _hip.DirectStepArgs()
    a.eps, a.x, a.out, a.offset = 1 << 24, X, OUT, OFF
    a.eps_dtype, a.cfg, a.guidance = 1, 1, 7.5
    a.n_prompts, a.channels, a.height, a.width = 4, 4, 64, 64
    a.sqrt_beta_t, a.sqrt_alpha_t, a.sqrt_alpha_prev, a.sqrt_one_minus_alpha_prev = 0.8, 0.6, 0.65, 0.76
    for k, v in kw.items():
        if isinstance(k, tuple):
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


_FOLD = {("blend_sums", 0): 1 << 26, "blend_lh": 40, "blend_res": 16}


@pytest.mark.parametrize("kw,code", [
    (dict(offset=None), E_ARG),
    (dict(offset=X), E_ARG),                                 # offset is x
    (dict(offset=OUT), E_ARG),                               # ... or out
    (dict(offset=X + 4 * ROW - 16), E_ARG),                  # starts in x's last bytes
    (dict(offset=OUT - 16), E_ARG),                          # its one row ends inside out
    (dict(offset=X - 2 * ROW + 16, group_size=2), E_ARG),    # two groups: the second row reaches x
    (dict(offset=X - 16, out=X), E_ARG),                     # out aliasing x is served, an offset in them is not
    (dict(group_size=3), E_ARG),                             # n_prompts no multiple of group_size
    (dict(eps=None), E_ARG), (dict(x=None), E_ARG), (dict(out=None), E_ARG),     # what p2p_latent_step rejects
    (dict(n_prompts=0), E_ARG), (dict(channels=0), E_ARG), (dict(height=0), E_ARG), (dict(width=0), E_ARG),
    (dict(group_size=-1), E_ARG),
    (dict(eps_dtype=7), E_DTYPE),
    # the one-launch LocalBlend form: its own conditions; a misaligned pointer is P2P_E_ARG, as in the
    # other three step forms
    ({**_FOLD, "mask": 512}, E_ARG),
    ({**_FOLD, "out": X}, E_ARG),
    ({**_FOLD, "height": 63, "width": 63}, E_ARG),
    ({**_FOLD, "x": X + 4}, E_ARG),
    ({**_FOLD, "offset": OFF + 4}, E_ARG),
    ({**_FOLD, "blend_res": 17}, E_ARG),
    ({("blend_sums", 3): 1 << 26, "blend_lh": 40, "blend_res": 16}, E_ARG),
    (dict(offset=None, eps_dtype=7), E_ARG),                 # two faults: a NULL offset is answered first ...
    (dict(offset=X, eps_dtype=7), E_DTYPE),                  # ... an overlapping one after the dtype
])
def test_direct_step_rejects(kw, code):
    """Every case returns before any launch (the pointers are not memory: a launch would fault)."""
    assert _hip.lib().p2p_direct_step(ctypes.byref(_step(kw)), None) == code


def _offset(**kw):
    a = _hip.DirectOffsetArgs()
    a.eps, a.x, a.target, a.coef, a.offset = 1 << 24, X, OUT, 4096, OFF
    a.eps_dtype, a.guidance, a.R, a.n = 1, 7.5, 4, 4 * 64 * 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code", [
    (dict(eps=None), E_ARG), (dict(x=None), E_ARG), (dict(target=None), E_ARG), (dict(coef=None), E_ARG),
    (dict(offset=None), E_ARG), (dict(R=0), E_ARG), (dict(R=-1), E_ARG), (dict(n=0), E_ARG),
    (dict(eps_dtype=7), E_DTYPE),
    (dict(R=65536), E_BATCH),
    (dict(n=4 * 64 * 64 + 2), E_ALIGN),
    (dict(eps=(1 << 24) + 8), E_ALIGN), (dict(x=X + 4), E_ALIGN), (dict(target=OUT + 8), E_ALIGN),
    (dict(coef=4100), E_ALIGN), (dict(offset=OFF + 4), E_ALIGN),
])
def test_direct_offset_rejects(kw, code):
    assert _hip.lib().p2p_direct_offset(ctypes.byref(_offset(**kw)), None) == code


def test_null_args_are_rejected():
    assert _hip.lib().p2p_direct_step(None, None) == E_ARG
    assert _hip.lib().p2p_direct_offset(None, None) == E_ARG


# ------------------------------------------------------------------ the stub model and the restatement
class StubTextEncoder:
    """One constant per prompt in every context element: 0 for "", 0.5 .. 1.1 from the token ids."""

    def __call__(self, ids):
        n_words = (ids != ids[:, -1:]).sum(1)            # tokens before the padding ("": 1, the start token)
        c = torch.where(n_words <= 1, torch.zeros(()), 0.5 + (ids.sum(1) % 7).float() / 10)
        return (c[:, None, None].expand(ids.shape[0], ids.shape[1], 4).contiguous(),)


class StubUNet:
    dtype = torch.float32
    in_channels = 4

    def __init__(self):
        self.calls = []

    def named_children(self):           # (no attention modules for register_attention_control to patch)
        return []

    def __call__(self, x, t, encoder_hidden_states=None):
        self.calls.append((x.clone(), torch.as_tensor(t).clone()))
        s = 0.5 + torch.as_tensor(t).reshape(-1).to(torch.float32) / 1000
        c = encoder_hidden_states[:, 0, 0]
        return {"sample": torch.tanh(x * s.reshape(-1, 1, 1, 1)) + c.reshape(-1, 1, 1, 1)}


def stub_model(scheduler="ddim"):
    return SimpleNamespace(unet=StubUNet(), tokenizer=default_tokenizer(), text_encoder=StubTextEncoder(),
                           scheduler=pl.make_scheduler(scheduler), device=torch.device("cpu"), vae=None)


def encode(model, prompts):
    return ptp_utils._encode(model, list(prompts), model.text_encoder)


def ddim_pair(sched, t, inverse):
    """(a_from, a_to) of the DDIM step at grid timestep t: t -> t - delta, or inverted t - delta -> t."""
    delta = 1000 // sched.num_inference_steps
    a_t = sched.alphas_cumprod[t]
    a_less = sched.alphas_cumprod[t - delta] if t - delta >= 0 else sched.final_alpha_cumprod
    return (a_less, a_t) if inverse else (a_t, a_less)


def ddim_move(sched, eps, t, x, inverse=False):
    """prev_step (null_text.py:471-479) and, inverted, next_step (:481-489), restated."""
    a_from, a_to = ddim_pair(sched, t, inverse)
    x0 = (x - (1 - a_from) ** 0.5 * eps) / a_from ** 0.5
    return a_to ** 0.5 * x0 + (1 - a_to) ** 0.5 * eps


def restated_inversion(model, z0, prompt, steps=STEPS, g=GUIDANCE):
    """The trajectory [z*_0 .. z*_T] and the offsets [steps, 1, 4, h, w], one U-Net row pair per step."""
    sched, unet = model.scheduler, StubUNet()
    sched.set_timesteps(steps)
    null, cond = encode(model, [""]), encode(model, [prompt])
    ts = [int(t) for t in sched.timesteps]
    traj = [z0]
    for t in reversed(ts):
        eps = unet(traj[-1], t, cond)["sample"]
        traj.append(ddim_move(sched, eps, t, traj[-1], inverse=True))
    offs = []
    for i, t in enumerate(ts):
        cur, prev = traj[steps - i], traj[steps - i - 1]
        eps_u, eps_c = unet(torch.cat([cur, cur]), t, torch.cat([null, cond]))["sample"].chunk(2)
        offs.append(prev - ddim_move(sched, eps_u + g * (eps_c - eps_u), t, cur))
    return traj, torch.stack(offs)


def restated_edit(model, prompts, x_T, offs, callback=None, steps=STEPS, g=GUIDANCE):
    """The edit loop: per step the guided DDIM step, the callback (LocalBlend's place), then the three
    lines.  Returns the latents after every step."""
    sched, unet = model.scheduler, StubUNet()
    sched.set_timesteps(steps)
    ctx = torch.cat([encode(model, [""] * len(prompts)), encode(model, prompts)])
    lat = x_T.expand(len(prompts), *x_T.shape[1:])
    seen = []
    for i, t in enumerate(int(t) for t in sched.timesteps):
        eps_u, eps_c = unet(torch.cat([lat] * 2), t, ctx)["sample"].chunk(2)
        lat = ddim_move(sched, eps_u + g * (eps_c - eps_u), t, lat)
        if callback is not None:
            lat = callback(lat)
        if offs is not None:
            lat = torch.cat([lat[:1] + offs[i], lat[1:]])
        seen.append(lat)
    return seen


def z_start(seed=0, shape=(1, 4, 8, 8)):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def library_edit(model, prompts, x_T, offs, steps=STEPS):
    """The same loop through ptp_utils.diffusion_step, latents after every step."""
    model.scheduler.set_timesteps(steps)
    ctx = torch.cat([encode(model, [""] * len(prompts)), encode(model, prompts)])
    lat = x_T.expand(len(prompts), *x_T.shape[1:])
    ctrl = null_text.EmptyControl()
    seen = []
    for i, t in enumerate(model.scheduler.timesteps):
        lat = ptp_utils.diffusion_step(model, ctrl, lat, ctx, t, GUIDANCE,
                                       latent_offset=None if offs is None else offs[i])
        seen.append(lat)
    return seen


# ------------------------------------------------------------------ 2. identity
def test_source_row_follows_the_trajectory():
    """After every edit-loop step the source row is the trajectory latent within 2^-16 max|z*|.
    Measured here (max|z*| = 3.89, bar 5.9e-5): the library loop and the eager restatement are the
    same bits and stay within 3.4e-6, a margin of 17x -- the rounding of one step's
    rec + (z*_prev - rec), carried on through a 1-Lipschitz U-Net under guidance 7.5; without offsets
    the same loop is off by 54.6, about 900,000 bars."""
    model = stub_model()
    z0 = z_start()
    (image_gt, image_rec), x_T, offs = DirectInversion(model, STEPS, GUIDANCE).invert(z0, SOURCE)
    assert image_gt is z0 and image_rec is None
    assert offs.shape == (STEPS, 1, 4, 8, 8) and offs.dtype == torch.float32 and torch.isfinite(offs).all()
    traj, want_offs = restated_inversion(model, z0, SOURCE)
    assert torch.equal(x_T, traj[-1]) and torch.equal(offs, want_offs)
    bar = 2.0 ** -16 * max(z.abs().max().item() for z in traj)

    def worst(seen):
        return max((lat[:1] - traj[STEPS - i - 1]).abs().max().item() for i, lat in enumerate(seen))

    restated = worst(restated_edit(model, [SOURCE, EDIT], x_T, offs))
    library = worst(library_edit(model, [SOURCE, EDIT], x_T, offs))
    without = worst(library_edit(model, [SOURCE, EDIT], x_T, None))
    print(f"bar {bar:.3e}  restated {restated:.3e}  library {library:.3e}  without offsets {without:.3e}")
    assert restated <= bar / 8          # the restatement alone, with margin
    assert library <= bar
    assert without >= 1000 * bar        # negative control
    # the edited row moved away from the source: the offsets went to row 0 only
    final = library_edit(model, [SOURCE, EDIT], x_T, offs)[-1]
    assert (final[1] - final[0]).abs().max().item() > 1000 * bar


# ------------------------------------------------------------------ 3. chunking
@pytest.mark.parametrize("steps_per_call", [1, 3, 4, 50])
def test_chunks_give_the_same_offsets(steps_per_call):
    """10 steps in calls of 1, 3 (tail of 1), 4 (tail of 2) and 50 (one short call): every row carries
    its own timestep and coefficients, so the offsets are the restatement's bit for bit."""
    model = stub_model()
    z0 = z_start(1)
    inv = DirectInversion(model, STEPS, GUIDANCE, steps_per_call=steps_per_call)
    _, x_T, offs = inv.invert(z0, SOURCE)
    traj, want = restated_inversion(model, z0, SOURCE)
    assert torch.equal(x_T, traj[-1])
    assert torch.equal(offs, want), (offs - want).abs().max().item()
    # the offsets pass really was chunked: U-Net calls of 2 x steps_per_call rows, then the tail
    rows = [x.shape[0] for x, t in model.unet.calls[STEPS:]]
    full, tail = divmod(STEPS, steps_per_call)
    assert rows == [2 * steps_per_call] * full + ([2 * tail] if tail else [])
    ts = torch.cat([t.reshape(-1)[:t.numel() // 2] for x, t in model.unet.calls[STEPS:]])
    assert ts.tolist() == model.scheduler.timesteps.tolist()
    assert want.abs().max().item() > 0.1            # (offsets of a guided step: not rounding noise)


def test_steps_per_call_must_be_positive():
    with pytest.raises(ValueError, match="steps_per_call"):
        DirectInversion(stub_model(), STEPS, GUIDANCE, steps_per_call=0)


# ------------------------------------------------------------------ 4. invert_batch
def test_invert_batch_is_three_inverts():
    prompts = [SOURCE, EDIT, "a photo of a cat riding a bike"]
    model = stub_model()
    assert len({encode(model, [p])[0, 0, 0].item() for p in prompts + [""]}) == 4     # four different contexts
    zs = [z_start(10 + b) for b in range(3)]
    inv = DirectInversion(model, STEPS, GUIDANCE, steps_per_call=3)
    batch = inv.invert_batch(torch.cat(zs), prompts)
    listed = inv.invert_batch(zs, prompts)
    assert len(batch) == 3
    for b in range(3):
        (gt, rec), x_T, offs = inv.invert(zs[b], prompts[b])
        assert offs.shape == (STEPS, 1, 4, 8, 8) and x_T.shape == (1, 4, 8, 8)
        for got in (batch[b], listed[b]):
            assert torch.equal(got[1], x_T) and torch.equal(got[2], offs)
            assert torch.equal(got[0][0], zs[b]) and got[0][1] is None
    assert not torch.equal(batch[0][2], batch[1][2])
    with pytest.raises(ValueError, match="prompts"):
        inv.invert_batch(zs, prompts[:2])
    with pytest.raises(ValueError, match="one size"):
        inv.invert_batch([zs[0], torch.zeros(1, 4, 16, 16)], prompts[:2])


# ------------------------------------------------------------------ 5. ordering and defaults
class MaskBlend(null_text.EmptyControl):
    """A controller with a step_callback of its own: LocalBlend's blend line (null_text.py:68-70) on a
    fixed mask, recording what it was given and what it returned."""

    def __init__(self, mask):
        self.mask, self.seen = mask, []

    def step_callback(self, x_t):
        out = x_t[:1] + self.mask * (x_t - x_t[:1])
        self.seen.append((x_t, out))
        return out


@pytest.mark.parametrize("low_resource", [False, True])
def test_offsets_are_added_after_the_blend(low_resource):
    """text2image_ldm_stable(latent_offsets=...) on 64 x 64 latents: what the next step starts from
    is, in rows >= 1, the blend against the UN-offset source row, and in row 0 that row plus the
    offset; the tensor form, the per-step list and the restatement agree bit for bit."""
    steps, prompts = 4, [SOURCE, EDIT, "a painting of a squirrel eating a lasagna"]
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(1, 4, 64, 64, generator=g)
    offs = 0.1 * torch.randn(steps, 1, 4, 64, 64, generator=g)
    mask = (torch.rand(3, 1, 64, 64, generator=g) > 0.5).float()
    model = stub_model()
    ctrl = MaskBlend(mask)
    final, _ = ptp_utils.text2image_ldm_stable(model, prompts, ctrl, num_inference_steps=steps, latent=x_T,
                                               low_resource=low_resource, latent_offsets=offs)
    assert len(ctrl.seen) == steps
    rows = 3 if low_resource else 6
    starts = [x[:3] for x, t in model.unet.calls if x.shape[0] == rows][::2 if low_resource else 1][1:] + [final]
    assert len(starts) == steps
    for i, ((given, blended), start) in enumerate(zip(ctrl.seen, starts)):
        assert torch.equal(blended, given[:1] + mask * (given - given[:1]))
        assert torch.equal(start[1:], blended[1:]), i                       # against the un-offset source
        assert torch.equal(start[:1], blended[:1] + offs[i]), i             # added after the blend
        assert not torch.equal(start[:1], blended[:1])
    want = restated_edit(model, prompts, x_T, offs, callback=lambda x: x[:1] + mask * (x - x[:1]), steps=steps)[-1]
    assert torch.equal(final, want)
    as_list, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps,
                                                 latent=x_T, low_resource=low_resource, latent_offsets=list(offs))
    assert torch.equal(as_list, final)


def test_no_offsets_is_todays_loop():
    steps, prompts = 4, [SOURCE, EDIT]
    g = torch.Generator().manual_seed(4)
    x_T = torch.randn(1, 4, 64, 64, generator=g)
    mask = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float()
    model = stub_model()
    plain, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps, latent=x_T)
    none, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps, latent=x_T,
                                              latent_offsets=None)
    want = restated_edit(model, prompts, x_T, None, callback=lambda x: x[:1] + mask * (x - x[:1]), steps=steps)[-1]
    assert torch.equal(plain, want) and torch.equal(none, want)
    zero, _ = ptp_utils.text2image_ldm_stable(model, prompts, MaskBlend(mask), num_inference_steps=steps, latent=x_T,
                                              latent_offsets=torch.zeros(steps, 1, 4, 64, 64))
    assert torch.equal(zero, want)


def test_offset_shape_is_checked():
    model = stub_model()
    model.scheduler.set_timesteps(4)
    lat = torch.zeros(3, 4, 8, 8)
    ctx = torch.cat([encode(model, [""] * 3), encode(model, [SOURCE] * 3)])
    for bad in (torch.zeros(2, 4, 8, 8), torch.zeros(1, 4, 8, 4), torch.zeros(4, 8, 8)):
        with pytest.raises(ValueError, match="latent_offset"):
            ptp_utils.diffusion_step(model, null_text.EmptyControl(), lat, ctx, 750, GUIDANCE, latent_offset=bad)


def test_add_latent_offset_per_group():
    g = torch.Generator().manual_seed(5)
    lat, off = torch.randn(6, 4, 8, 8, generator=g), torch.randn(3, 4, 8, 8, generator=g)
    got = ptp_utils.add_latent_offset(lat, off)
    want = lat.clone()
    want[0::2] += off
    assert torch.equal(got, want)
    assert torch.equal(ptp_utils.add_latent_offset(lat, off[:1]), torch.cat([lat[:1] + off[:1], lat[1:]]))


# ------------------------------------------------------------------ 6. scheduler check
@pytest.mark.parametrize("scheduler", ["dpm", "pndm"])
def test_needs_a_ddim_scheduler(scheduler):
    with pytest.raises(TypeError, match="prev_step"):
        DirectInversion(stub_model(scheduler))
    assert DirectInversion(stub_model("ddim"), 4).scheduler.num_inference_steps == 4
