"""Direct Inversion on the GPU: p2p_direct_offset and p2p_direct_step bit for bit against
p2p_latent_step plus the torch line each one fuses, the fused edit loop against the eager add, the
fp16 workflow null-text inversion refuses, the reconstruction property on a real U-Net, and the
graphed passes against the eager ones.

The reference of every test is the eager restatement of the two formulas:

    offset[i] = z*_prev - prev_step(eps_u + g (eps_c - eps_u), t_i, z*_cur)
    latents   = cat(latents[:1] + offset[i], latents[1:])         after diffusion_step
"""
import pytest
import torch

from test_gpu_blend_geometry import one_launch_inputs

from p2p_amd import _hip, config, null_text, ptp_utils
from p2p_amd import pipeline as pl
from p2p_amd.ddim import DDIMScheduler
from p2p_amd.direct_inversion import DirectInversion

pytestmark = pytest.mark.gpu

GUIDANCE = 7.5
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]


def scheduler(n=50):
    s = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                      set_alpha_to_one=False)
    s.set_timesteps(n)
    return s


def eager_move(eps, x, coeffs, guidance=None):
    """The CFG line (ptp_utils.py:73) and prev_step / next_step (null_text.py:471-489) as torch ops,
    the four factors computed on the host (DDIMScheduler.prev_coeffs / next_coeffs) -- the eager
    sequence p2p_latent_step equals bit for bit (tests/test_gpu_latent.py)."""
    sb, sa, sp, s1p = (torch.tensor(c, dtype=torch.float32, device=x.device) for c in coeffs)
    if guidance is not None:
        eu, ec = eps.chunk(2)
        eps = eu + guidance * (ec - eu)
    return sp * ((x - sb * eps) / sa) + s1p * eps


# ------------------------------------------------------------------ 1. p2p_direct_offset
@pytest.mark.parametrize("g", [1.0, 7.5])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("chw", [(4, 8, 8), (4, 6, 10), (4, 64, 64)], ids=["4x8x8", "4x6x10", "4x64x64"])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_direct_offset_bit_exact(cuda, R, chw, dtype, g):
    """Per row: p2p_latent_step without a mask with that row's coefficients, then torch's subtract.
    Rows at timesteps 981 / 501 / 1 in one launch (1 steps to the final alpha); offset pre-filled
    with NaN; 4 x 6 x 10 = 240 elements is neither a power of two nor a multiple of the 256-thread
    block."""
    s = scheduler()
    gen = torch.Generator().manual_seed(R * 1000 + chw[1] * 10 + int(g))
    eps = torch.randn(2 * R, *chw, generator=gen).to(dtype).to(cuda)
    x = torch.randn(R, *chw, generator=gen).to(cuda)
    target = torch.randn(R, *chw, generator=gen).to(cuda)
    ts = [(981, 501, 1)[r % 3] for r in range(R)]
    coef = torch.tensor([s.prev_coeffs(t) for t in ts], dtype=torch.float32, device=cuda)
    before = [t.clone() for t in (eps, x, target, coef)]
    got = _hip.direct_offset(eps, x, target, coef, g, torch.full_like(x, float("nan")))
    for r in range(R):
        pair = torch.cat([eps[r:r + 1], eps[R + r:R + r + 1]]).contiguous()
        rec = _hip.latent_step(pair, x[r:r + 1].contiguous(), torch.empty(1, *chw, device=cuda), s.prev_coeffs(ts[r]), g)
        want = target[r:r + 1] - rec
        assert torch.equal(got[r:r + 1], want), (r, (got[r:r + 1] - want).abs().max().item())
        # and that is the eager sequence, with the host-computed coefficients as 0-dim tensors
        assert torch.equal(rec, eager_move(pair, x[r:r + 1], s.prev_coeffs(ts[r]), g))
    assert torch.isfinite(got).all()
    for t, b in zip((eps, x, target, coef), before):
        assert torch.equal(t, b)
    if R > 1:       # the rows' coefficients matter: row 1 with row 0's is another result
        wrong = _hip.direct_offset(eps, x, target, coef[:1].expand(R, 4).contiguous(), g, torch.empty_like(x))
        assert not torch.equal(wrong[1], got[1])


def test_direct_offset_wrapper_refuses_shapes(cuda):
    x = torch.zeros(2, 4, 8, 8, device=cuda)
    eps = torch.zeros(4, 4, 8, 8, device=cuda)
    coef = torch.ones(2, 4, device=cuda)
    with pytest.raises(_hip.HipError):
        _hip.direct_offset(eps[:3], x, x.clone(), coef, 7.5, torch.empty_like(x))
    with pytest.raises(_hip.HipError):
        _hip.direct_offset(eps, x, x.clone(), coef[:1], 7.5, torch.empty_like(x))
    with pytest.raises(_hip.HipError):
        _hip.direct_offset(eps, x, x.clone(), coef.cpu(), 7.5, torch.empty_like(x))


# ------------------------------------------------------------------ 2. p2p_direct_step
# (n_prompts, group_size) = (2, 0), (4, 4), (6, 2) and (12, 4); the three-group cases have group 1 off
GROUPINGS = {"2_0": dict(gs=2, groups=(True,)), "4_4": dict(gs=4, groups=(True,), explicit=True),
             "6_2": dict(gs=2, groups=(True, False, True)), "12_4": dict(gs=4, groups=(True, False, True))}


def step_case(cuda, grouping, dtype, geometry, seed):
    kw = dict(GROUPINGS[grouping])
    explicit = kw.pop("explicit", False)
    eps, x, blend, mask, group_size, gb = one_launch_inputs(cuda, dict(kw, dtype=dtype, **geometry), seed)
    if explicit:
        group_size = kw["gs"]           # one group named by its size instead of 0
    n_groups = len(kw["groups"])
    gen = torch.Generator().manual_seed(seed + 1)
    offset = (0.1 * torch.randn(n_groups, *x.shape[1:], generator=gen)).to(cuda)
    first = torch.arange(n_groups, device=cuda) * kw["gs"]
    return eps, x, blend, mask, group_size, gb, offset, first


def check_direct_step(cuda, eps, x, blend, mask, group_size, gb, offset, first, form):
    coeffs = scheduler().prev_coeffs(500)
    args = {"nomask": (None, group_size, None, None), "mask": (mask, group_size, gb, None),
            "blend": (None, group_size, None, blend)}[form]
    plain = _hip.latent_step(eps, x, torch.empty_like(x), coeffs, GUIDANCE, *args)
    want = plain.clone()
    want[first] = plain[first] + offset                 # the torch add on the group-first rows
    x_before = x.clone()
    got = _hip.direct_step(eps, x, torch.full_like(x, float("nan")), coeffs, offset, GUIDANCE, *args)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), (form, (got - want).abs().max().item())
    others = torch.ones(x.shape[0], dtype=torch.bool, device=cuda)
    others[first] = False
    assert torch.equal(got[others], plain[others])      # the other rows blend towards the UN-offset source
    assert not torch.equal(got[first], plain[first]) and torch.equal(x, x_before)
    if form != "nomask":
        assert not torch.equal(plain, _hip.latent_step(eps, x, torch.empty_like(x), coeffs, GUIDANCE, None, group_size))
    if form != "blend":                                 # out aliasing x, where p2p_latent_step allows it
        buf = x.clone()
        assert _hip.direct_step(eps, buf, buf, coeffs, offset, GUIDANCE, *args) is buf
        assert torch.equal(buf, want)
    else:
        with pytest.raises(_hip.HipError):
            _hip.direct_step(eps, x, x, coeffs, offset, GUIDANCE, *args)


@pytest.mark.parametrize("form", ["nomask", "mask", "blend"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("grouping", list(GROUPINGS))
def test_direct_step_bit_exact(cuda, grouping, dtype, form):
    """4 x 16 x 16 latents with 8 x 8 maps: p2p_latent_step of the same form, then the torch add."""
    case = step_case(cuda, grouping, dtype, dict(R=8, lat=(16, 16)), 700 + list(GROUPINGS).index(grouping))
    check_direct_step(cuda, *case, form)


@pytest.mark.parametrize("form", ["nomask", "mask", "blend"])
def test_direct_step_bit_exact_product_geometry(cuda, form):
    """4 x 64 x 64 latents with 16 x 16 maps, three groups of four, bf16."""
    check_direct_step(cuda, *step_case(cuda, "12_4", torch.bfloat16, dict(R=16, lat=(64, 64)), 750), form)


def test_direct_step_wrapper_refuses_offset_shapes(cuda):
    eps, x, blend, mask, group_size, gb, offset, first = step_case(cuda, "6_2", torch.float32, dict(R=8, lat=(16, 16)), 760)
    coeffs = scheduler().prev_coeffs(500)
    for bad in (offset[:2].contiguous(), offset.double(), offset[:, :, :8], offset.cpu()):
        out = torch.full_like(x, 7.0)
        with pytest.raises(_hip.HipError):
            _hip.direct_step(eps, x, out, coeffs, bad, GUIDANCE, mask, group_size, gb)
        assert (out == 7.0).all()


# ------------------------------------------------------------------ 3. the edit loop, fused against eager
STEPS = 10
SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128))     # tests/test_gpu_pndm.py: head dims 8 and 16
SOURCE = "a painting of a squirrel eating a burger"


class HostFactorDDIM(DDIMScheduler):
    """prev_step's lines with the four factors computed on the host -- the values p2p_latent_step
    is given (prev_coeffs).  DDIMScheduler.prev_step takes a ** 0.5 of a 0-dim tensor on the device,
    where 368 of the 1000 square roots come out an ulp away from the host's, so on the GPU the
    scheduler's own lines and the fused step were never the same bits (measured; the step and its
    factors are older than this file).  What is compared below is the order of step, blend and add."""

    def prev_step(self, model_output, timestep, sample):
        return eager_move(model_output, sample, self.prev_coeffs(timestep))


class EagerReplace(null_text.AttentionReplace):
    """A step_callback of the caller's own: diffusion_step then takes scheduler.step, this callback
    (LocalBlend) and the eager add."""

    def step_callback(self, x_t):
        return super().step_callback(x_t)


def make_ctrl(cls, prompts, cuda, fold):
    lb = null_text.LocalBlend(list(prompts), pl.BLEND_WORDS, th=(.3, .3), device=cuda)
    lb.start_blend = 2                       # blends from the third call on
    ctrl = cls(list(prompts), STEPS, cross_replace_steps=.8, self_replace_steps=.4, local_blend=lb, device=cuda)
    ctrl.fold_local_blend = fold
    return ctrl


class Kinds:
    def __init__(self):
        self.kinds = []

    def before(self, *args):
        pass

    after = before

    def before_aux(self, kind, nbytes):
        self.kinds.append(kind)


def edit(model, cls, x_T, offs, cuda, fold=False):
    prompts = pl.north_star_prompts()
    ctrl = make_ctrl(cls, prompts, cuda, fold)
    obs, prev = Kinds(), _hip.LAUNCH_OBSERVER
    _hip.LAUNCH_OBSERVER = obs
    try:
        with config.compute_mode("bf16"):
            lat, _ = ptp_utils.text2image_ldm_stable(model, prompts, ctrl, num_inference_steps=STEPS, latent=x_T,
                                                     latent_offsets=offs)
    finally:
        _hip.LAUNCH_OBSERVER = prev
    assert ctrl.cur_step == STEPS and ctrl.local_blend.counter == STEPS
    return lat, [k for k in obs.kinds if k.startswith(("direct", "latent"))]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_edit_loop_fused_equals_eager(cuda, dtype):
    """AttentionReplace + LocalBlend, 10 steps, a tiny U-Net: one p2p_direct_step per step against
    scheduler.step, step_callback and the eager add -- the same final latents.  (fold_local_blend off,
    as in the other fused-against-eager loops: both then build the mask from the stored maps.)  With
    the fold on, the loop runs the one-launch form, whose source row -- which no mask touches -- is
    the same bits again."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=dtype, unet_config=SMALL_UNET)
    model.scheduler = HostFactorDDIM(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                     clip_sample=False, set_alpha_to_one=False)
    x_T = pl.seed_latent(5)
    offs = (0.05 * torch.randn(STEPS, 1, 4, 64, 64, generator=torch.Generator().manual_seed(6))).to(cuda)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        edit(model, null_text.AttentionReplace, x_T, offs, cuda)          # warm-up: library kernel selection
        fused, kinds_f = edit(model, null_text.AttentionReplace, x_T, offs, cuda)
        eager, kinds_e = edit(model, EagerReplace, x_T, offs, cuda)
        folded, kinds_o = edit(model, null_text.AttentionReplace, x_T, offs, cuda, fold=True)
        plain, kinds_p = edit(model, null_text.AttentionReplace, x_T, None, cuda)
    finally:
        torch.backends.cudnn.enabled = det
    assert kinds_f == ["direct_step"] * STEPS and kinds_e == [] and kinds_p == ["latent_step"] * STEPS
    assert kinds_o == ["direct_step"] * 2 + ["direct_blend"] * (STEPS - 2)
    assert torch.isfinite(fused).all() and (fused[1:] != fused[:1]).any()
    assert torch.equal(fused, eager), (fused - eager).abs().max().item()
    assert torch.equal(folded[:1], fused[:1])
    assert (fused[:1] - plain[:1]).abs().max().item() > 1e-2               # the offsets moved the source row


# ------------------------------------------------------------------ 4. fp16
def test_fp16_inverts_and_edits(cuda):
    """What NullInversion cannot do (the attention backward refuses float16): invert with a float16
    U-Net, then edit with the offsets."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.float16, unet_config=SMALL_UNET)
    z0 = pl.seed_latent(11).to(cuda)
    with config.compute_mode("bf16"):
        inv = DirectInversion(model, num_ddim_steps=STEPS)
        (gt, rec), x_T, offs = inv.invert(z0, SOURCE)
    assert gt is z0 and rec is None
    assert x_T.shape == (1, 4, 64, 64) and x_T.dtype == torch.float32 and torch.isfinite(x_T).all()
    assert offs.shape == (STEPS, 1, 4, 64, 64) and offs.dtype == torch.float32 and offs.is_cuda
    assert torch.isfinite(offs).all() and offs.abs().max().item() > 0
    lat, kinds = edit(model, null_text.AttentionReplace, x_T, offs, cuda)
    assert kinds == ["direct_step"] * STEPS
    assert lat.shape == (4, 4, 64, 64) and torch.isfinite(lat).all()
    with pytest.raises(NotImplementedError, match="float16"):
        null_text.NullInversion(model, num_ddim_steps=STEPS).invert_batch(z0, [SOURCE])


# ------------------------------------------------------------------ 5. the property on a real U-Net
def test_source_row_returns_to_the_image_latent(cuda):
    """f32 tiny SD-topology U-Net, 10 steps, g = 7.5: with the offsets the source row ends nearer to
    z*_0 than the same loop without them.  No ratio is fixed (how strongly the random-init U-Net
    depends on its context is not known); both errors are printed."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.float32, unet_config=SMALL_UNET)
    z0 = pl.seed_latent(12).to(cuda)
    prompts = [SOURCE, "a painting of a lion eating a burger"]
    with config.compute_mode("bf16"):
        inv = DirectInversion(model, num_ddim_steps=STEPS, guidance_scale=GUIDANCE)
        _, x_T, offs = inv.invert(z0, SOURCE)
        runs = {}
        for name, o in (("with", offs), ("without", None)):
            lat, _ = ptp_utils.text2image_ldm_stable(model, prompts, null_text.EmptyControl(), num_inference_steps=STEPS,
                                                     guidance_scale=GUIDANCE, latent=x_T, latent_offsets=o)
            runs[name] = (lat[:1] - z0).abs().max().item()
    print(f"source row, max |final - z*_0| (max |z*_0| = {z0.abs().max().item():.3f}): "
          f"with offsets {runs['with']:.3e}, without {runs['without']:.3e}")
    assert runs["with"] < runs["without"]


def test_fused_inversion_loop_is_the_eager_loop(cuda):
    """ddim_loop through p2p_latent_step with next_coeffs against the eager lines of next_step
    (NullInversion.ddim_loop's, the factors computed on the host), bf16 U-Net, 4 steps: the same
    trajectory."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=SMALL_UNET)
    z0 = pl.seed_latent(13).to(cuda)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"), torch.no_grad():
            inv = DirectInversion(model, num_ddim_steps=4, use_graphs=False)
            inv.init_prompt(SOURCE)
            ptp_utils.register_attention_control(model, None)
            inv.ddim_loop(z0)                                     # warm-up: library kernel selection
            got = inv.ddim_loop(z0)
            cond = inv.context.chunk(2)[1]
            want = [z0]
            for t in reversed(model.scheduler.timesteps.tolist()):
                eps = model.unet(want[-1], t, encoder_hidden_states=cond)["sample"]
                want.append(eager_move(eps, want[-1], model.scheduler.next_coeffs(t)))
    finally:
        torch.backends.cudnn.enabled = det
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a - b).abs().max().item()
    assert (got[-1] - z0).abs().max().item() > 0.1


# ------------------------------------------------------------------ 6. graphs
def test_graphed_passes_equal_eager(cuda):
    """SD shape, bf16, 4 steps in calls of 3 (a full call and the short tail, two graphs): the
    graphed inversion and offsets pass against use_graphs=False."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16)
    z0 = pl.seed_latent(14).to(cuda)
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        with config.compute_mode("bf16"):
            out = {}
            for graphs in (False, True):
                inv = DirectInversion(model, num_ddim_steps=4, steps_per_call=3, use_graphs=graphs)
                if not graphs:
                    inv.invert(z0, SOURCE)                        # warm-up: library kernel selection
                out[graphs] = inv.invert(z0, SOURCE)
    finally:
        torch.backends.cudnn.enabled = det
    (_, x_e, off_e), (_, x_g, off_g) = out[False], out[True]
    assert off_g.shape == (4, 1, 4, 64, 64) and torch.isfinite(off_g).all()
    assert torch.equal(x_g, x_e), (x_g - x_e).abs().max().item()
    assert torch.equal(off_g, off_e), (off_g - off_e).abs().max().item()
