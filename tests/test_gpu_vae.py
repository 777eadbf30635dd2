"""The VAE on the GPU: the d = 512 self-attention kernel (csrc/p2p_selfwide.hip), the split GroupNorm
statistics of large slabs (csrc/p2p_unet.hip), the image ends (csrc/p2p_image.hip), the module's
fused path against its own torch lines, and the pipeline returning images / inverting one."""
import copy

import numpy as np
import pytest
import torch

from p2p_amd import _hip, null_text, ptp_utils, unet, vae
from p2p_amd import pipeline as pl
from test_gpu_kernels import make_qkv, o_tol, ref_out, ref_probs
from test_gpu_unet_glue import check, gn_case, rand

pytestmark = pytest.mark.gpu

WIDE = "self_wide_kernel<512,…>"
D = 512
NARROW_VAE = dict(block_out_channels=(32, 64), layers_per_block=1, norm_num_groups=8)
SMALL_UNET = dict(block_out_channels=(64, 128, 128, 128))     # tests/test_gpu_pndm.py: head dims 8 and 16
# Softmax rows are "peaky" when one key dominates.  With q scaled by s the logits q.k d^-1/2 have
# standard deviation s; the gap between the two largest of K Gaussian logits is then about
# s / sqrt(2 ln K) (2.2 at s = 8, K = 1024: the top probability is mostly below 0.9), so the peaky
# cases use s = 64 (gap ~ 17 at K = 1024, ~ 26 at K = 20).
PEAKY = 64.0
DTYPES = [torch.bfloat16, torch.float16]

_ref_cache = {}


def wide_case(N, P, K, H, dtype, qscale):
    """Inputs and the f32 reference of one geometry, computed once and shared (never modified)."""
    key = (N, P, K, H, dtype, qscale)
    if key not in _ref_cache:
        q, k, v = make_qkv(N, P, K, H, D, dtype, qscale=qscale, seed=P + K + H)
        probs = ref_probs(q, k, H, D ** -0.5)
        _ref_cache[key] = (q, k, v, probs.amax(-1), ref_out(probs, v, H))
    return _ref_cache[key]


def run_wide(q, k, v, H, o=None):
    o = torch.empty(q.shape[0], q.shape[1], H * D, dtype=q.dtype, device=q.device) if o is None else o
    assert _hip.self_attn_kernel(_hip.make_tensors(q, k, v, o, H, D ** -0.5, "bf16")) == WIDE
    _hip.self_attn(q, k, v, o, H, D ** -0.5)
    return o


def wide_bound(v, want):
    # the project's bar for a 16-bit output (tests/test_gpu_kernels.py's bf16-output kernels)
    return o_tol(v, "bf16") + 2.0 ** -8 * want.abs().max().item()


GEOMS = [(2, 20, 20, 1), (2, 64, 64, 1), (2, 200, 200, 1), (2, 1024, 1024, 1),   # partial / full / ragged / many tiles
         (2, 200, 77, 1),                                                         # P != K
         (2, 200, 200, 2)]                                                        # two heads


# ------------------------------------------------------------------ 1. the wide kernel
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("qscale", [1.0, PEAKY], ids=["flat", "peaky"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_wide_kernel_output(cuda, geom, qscale, dtype):
    N, P, K, H = geom
    q, k, v, pmax, want = wide_case(N, P, K, H, dtype, qscale)
    if qscale == PEAKY:
        frac = (pmax > 0.9).float().mean().item()
        assert frac > 0.5, f"only {frac:.2f} of the reference rows are peaky: the rescale path is not exercised"
    o = run_wide(q, k, v, H)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - want).abs().max().item()
    bound = wide_bound(v, want)
    print(f"wide {geom} qscale={qscale} {dtype}: max |O - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------ 2. strided views, 3. determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_wide_kernel_strided_views_and_determinism(cuda, dtype):
    N, P = 2, 200
    g = torch.Generator(device=cuda).manual_seed(3)
    qkv = torch.randn(N, P, 3 * D, device=cuda, generator=g).to(dtype)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    assert q.stride(1) == 3 * D and not k.is_contiguous()
    o_views = run_wide(q, k, v, 1)
    o_dense = run_wide(q.contiguous(), k.contiguous(), v.contiguous(), 1)
    assert o_views.is_contiguous() and torch.equal(o_views, o_dense)
    assert torch.equal(run_wide(q, k, v, 1), o_views), "two launches on one input differ"
    want = ref_out(ref_probs(q, k, 1, D ** -0.5), v, 1)
    assert (o_views.float() - want).abs().max().item() <= wide_bound(v, want)


# ------------------------------------------------------------------ 9. negative control
def test_wide_kernel_negative_control(cuda):
    """The comparison of test 1 notices a wrong scale: against a reference built with d^-1/4 (one
    of diffusers' two factors alone) the same kernel output is outside the bound."""
    N, P, K, H = 2, 200, 200, 1
    q, k, v, _, want = wide_case(N, P, K, H, torch.bfloat16, 1.0)
    o = run_wide(q, k, v, H)
    wrong = ref_out(ref_probs(q, k, H, D ** -0.25), v, H)
    assert (o.float() - want).abs().max().item() <= wide_bound(v, want)
    assert (o.float() - wrong).abs().max().item() > wide_bound(v, wrong)


# ------------------------------------------------------------------ 4. GroupNorm, split statistics
GN_SPLIT = 262144    # kGnStatsSplit (csrc/p2p_kernels.h): slabs of this size or more take the split form
GN_CHUNK = 32768     # kGnStatsChunk
GN_UNET_MAX = 122880  # the U-Net's largest slab, which the threshold has to stay above


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("N,C,H,W,groups,silu,tokens,add", [
    (2, 960, 64, 64, 32, True, False, None),          # the U-Net's largest slab: the one-workgroup form
    (1, 128, 8191, 8, 32, False, True, "nc+bias"),    # 262,112: just below the threshold
    (1, 128, 256, 256, 32, True, False, "c"),         # the threshold itself (the decoder's 256 x 256 norm): 8 chunks
    (1, 128, 256, 256, 32, False, True, None),
    (2, 64, 8193, 8, 16, True, True, "nc+bias"),      # 262,176: 9 chunks of 3642 vectors, the last one 3636
    (2, 8, 512, 512, 8, False, False, None),          # cpg = 1 with a large hw: 8 chunks per slab
    (1, 32, 512, 512, 8, True, False, "nc"),          # a 1 M-element slab (the decoder's 512 x 512 norm): 32 chunks
    (2, 24, 408, 400, 4, True, True, None),           # 979,200 elements: 30 chunks, the last one shorter
], ids=lambda x: str(x))
def test_group_norm_split_statistics(cuda, dtype, N, C, H, W, groups, silu, tokens, add):
    slab = C // groups * H * W
    assert N * C * H * W * 2 <= 32 << 20
    assert GN_SPLIT > GN_UNET_MAX
    if (C, H, W) == (960, 64, 64):
        assert slab == GN_UNET_MAX
    if (C, H, W) == (128, 8191, 8):
        assert GN_SPLIT - 8 * C // groups == slab
    if (C, H, W) == (128, 256, 256):
        assert slab == GN_SPLIT
    if (C, H, W) == (64, 8193, 8):
        chunks = -(-slab // GN_CHUNK)
        assert slab > GN_SPLIT and chunks == 9 and slab % (chunks * 8) != 0
    f = _hip.lib().p2p_group_norm_stats_floats
    assert (f(N, C, H * W, groups) > 2 * N * groups) == (slab >= GN_SPLIT)
    # against the f32 formula, with test_gpu_unet_glue's bar; gn_case also launches twice and
    # requires equal bits
    gn_case(cuda, dtype, N, C, H, W, groups, silu, tokens, add, eps=1e-6)


def test_group_norm_at_the_threshold_keeps_the_one_workgroup_form(cuda):
    """A slab of exactly 122,880 elements (the U-Net's largest, below the split threshold) must run
    what it ran before the split form existed.  No equal-statistics construction gives the one-workgroup result bit for bit from
    other launches (halving the slab changes the f32 summation order), so this asserts what can be
    asserted: the workspace is the {mean, rstd} pairs only -- the split form cannot run without its
    partials -- and the result meets the tolerance (test_group_norm_split_statistics, first case)."""
    assert _hip.lib().p2p_group_norm_stats_floats(2, 960, 4096, 32) == 2 * 32 * 2
    x = rand((1, 960, 64, 64), torch.bfloat16, cuda, 1, 2.0, 0.5)
    gamma, beta = rand((960,), torch.bfloat16, cuda, 2, 0.5, 1.0), rand((960,), torch.bfloat16, cuda, 3)
    y = _hip.group_norm(x, gamma, beta, 32, 1e-5)
    ref = torch.nn.functional.group_norm(x.float(), 32, gamma.float(), beta.float(), 1e-5)
    check(y, ref, torch.bfloat16, "group_norm at the split threshold")


# ------------------------------------------------------------------ 5. the image ends
def _u8_expr(x):
    return (((x.float() / 2 + 0.5).clamp(0, 1)) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_image_u8_is_byte_exact(cuda, dtype):
    g = torch.Generator(device=cuda).manual_seed(4)
    x = torch.randn(2, 3, 64, 64, device=cuda, generator=g) * 0.8
    flat = x.view(-1)
    # below -1, above 1, exactly +-1
    flat[:8] = torch.tensor([-1.0, 1.0, -1.5, 1.5, -100.0, 100.0, -1.0000001, 1.0000001], device=cuda)
    # values landing within one ulp of an integer after x 255: y = j / 255 for every j, and its f32
    # neighbours on both sides, mapped back through x = 2 y - 1
    j = torch.arange(256, device=cuda, dtype=torch.float32)
    y = j / 255
    for i, yy in enumerate((y, torch.nextafter(y, torch.full_like(y, 2.0)), torch.nextafter(y, torch.full_like(y, -1.0)))):
        flat[16 + 256 * i: 16 + 256 * (i + 1)] = yy * 2 - 1
    x = x.to(dtype)
    want = _u8_expr(x)
    got = _hip.image_u8(x)
    assert got is not None and got.dtype == torch.uint8 and got.shape == (2, 64, 64, 3)
    assert torch.equal(got, want)
    assert want.min().item() == 0 and want.max().item() == 255
    # the pipeline's helper returns the same bytes as an ndarray
    assert np.array_equal(ptp_utils.image_to_uint8(x), want.cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_image_to_model_rounds_once(cuda, dtype):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 16, 64, 3), dtype=np.uint8)
    img.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                     # every byte value
    t = torch.from_numpy(img)
    want = (t.float() / 127.5 - 1).permute(0, 3, 1, 2).contiguous().to(dtype)   # f32 on the CPU (an IEEE division), one rounding
    got = _hip.image_to_model(t.to(cuda), dtype)
    assert got is not None and got.dtype == dtype and got.shape == (2, 3, 16, 64)
    assert torch.equal(got.cpu(), want)
    one = _hip.image_to_model(t[0].to(cuda), dtype)          # [H, W, 3]
    assert torch.equal(one.cpu(), want[:1])
    assert torch.equal(ptp_utils.image_to_model(img, cuda, dtype).cpu(), want)


def test_image_ends_odd_sizes(cuda):
    """height * width % 4 != 0: the entry points answer P2P_E_ALIGN (include/p2p_hip.h), the bindings
    return None and the helpers run their torch lines -- the same results."""
    g = torch.Generator(device=cuda).manual_seed(6)
    x = (torch.randn(1, 3, 5, 7, device=cuda, generator=g)).to(torch.bfloat16)
    assert _hip.image_u8(x) is None
    assert np.array_equal(ptp_utils.image_to_uint8(x), _u8_expr(x).cpu().numpy())
    img = np.random.default_rng(7).integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    assert _hip.image_to_model(torch.from_numpy(img).to(cuda), torch.float32) is None
    want = (torch.from_numpy(img).float() / 127.5 - 1).permute(2, 0, 1)[None]
    assert torch.equal(ptp_utils.image_to_model(img, cuda, torch.float32).cpu(), want)
    # 4 | H W without 4 | W is served by the kernel
    x2 = torch.randn(1, 3, 6, 6, device=cuda, generator=g).to(torch.float16)
    assert torch.equal(_hip.image_u8(x2), _u8_expr(x2))


# ------------------------------------------------------------------ 6. / 7. the module, fused against its torch lines
def three_ways(m16, fn, x, monkeypatch):
    """fn(module, x) on the fused path, on the 16-bit torch lines and in f32 with the same weights."""
    m32 = copy.deepcopy(m16).float()
    with torch.no_grad():
        fused = fn(m16, x)
        with monkeypatch.context() as mp:
            mp.setattr(unet, "FUSE_UNET", False)
            torch16 = fn(m16, x)
        ref = fn(m32, x.float())
    return fused, torch16, ref


def assert_fused_no_worse(fused, torch16, ref, what):
    assert fused.shape == ref.shape and fused.dtype == torch16.dtype and torch.isfinite(fused.float()).all()
    e_f = (fused.float() - ref).abs().max().item()
    e_t = (torch16.float() - ref).abs().max().item()
    print(f"{what}: fused err {e_f:.4e}, torch 16-bit err {e_t:.4e}, max|ref| {ref.abs().max().item():.4e}")
    assert e_f <= 2 * e_t + 2.0 ** -8 * ref.abs().max().item(), (what, e_f, e_t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_narrow_vae_fused_against_torch_lines(cuda, dtype, monkeypatch):
    torch.manual_seed(8)
    m = vae.AutoencoderKL(**NARROW_VAE).to(cuda, dtype).eval()
    g = torch.Generator(device=cuda).manual_seed(9)
    z = torch.randn(2, 4, 16, 16, device=cuda, generator=g).to(dtype)
    dec = three_ways(m, lambda mod, t: mod.decode(t)["sample"], z, monkeypatch)
    assert dec[0].shape == (2, 3, 32, 32)
    assert_fused_no_worse(*dec, f"narrow decode {dtype}")
    img = torch.rand(2, 3, 32, 32, device=cuda, generator=g).mul(2).sub(1).to(dtype)
    enc = three_ways(m, lambda mod, t: mod.encode(t)["latent_dist"].mean, img, monkeypatch)
    assert enc[0].shape == (2, 4, 16, 16)
    assert_fused_no_worse(*enc, f"narrow encode {dtype}")


def test_sd_shape_decode_runs_the_wide_kernel(cuda, monkeypatch):
    torch.manual_seed(10)
    m = vae.AutoencoderKL().to(cuda, torch.bfloat16).eval()
    g = torch.Generator(device=cuda).manual_seed(11)
    z = torch.randn(1, 4, 64, 64, device=cuda, generator=g).to(torch.bfloat16)
    launches = []
    real = _hip.self_attn

    def shim(q, k, v, o, heads, scale, *a, **kw):
        launches.append((_hip.self_attn_kernel(_hip.make_tensors(q, k, v, o, heads, scale, "bf16")), tuple(q.shape),
                         q.stride(1)))
        return real(q, k, v, o, heads, scale, *a, **kw)

    with torch.no_grad(), monkeypatch.context() as mp:
        mp.setattr(_hip, "self_attn", shim)
        m.decode(z)
    assert launches == [(WIDE, (1, 4096, 512), 3 * 512)]        # one head of 512 over 64 x 64 tokens, strided views
    dec = three_ways(m, lambda mod, t: mod.decode(t)["sample"], z, monkeypatch)
    assert dec[0].shape == (1, 3, 512, 512)
    assert_fused_no_worse(*dec, "SD-shape decode bf16")
    with torch.no_grad():
        img = ptp_utils.latent2image(m, z.float() * 0.18215)
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (1, 512, 512, 3)


# ------------------------------------------------------------------ 8. end to end
PROMPTS = ["a painting of a squirrel eating a burger", "a painting of a lion eating a burger"]


def test_text2image_returns_images(cuda):
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16, unet_config=SMALL_UNET, vae_config=NARROW_VAE)
    x_T = pl.seed_latent(3)

    def run():
        ctrl = pl.make_replace_controller(PROMPTS, num_steps=3, blend_words=None, device=cuda)
        return ptp_utils.text2image_ldm_stable(model, PROMPTS, ctrl, num_inference_steps=3, latent=x_T)[0]

    # MIOpen's default convolution solvers are not run-to-run reproducible (two identical
    # U-Net calls differ by up to 2e-2), so, as the other bit-identity tests of the suite
    # (tests/test_gpu_pipeline.py), both runs take PyTorch's native convolution path
    det = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        images = run()
        side = 2 * x_T.shape[-1]                    # the narrow VAE has one upsampler
        assert isinstance(images, np.ndarray) and images.dtype == np.uint8 and images.shape == (2, side, side, 3)
        assert not np.array_equal(images[0], images[1])
        vae_, model.vae = model.vae, None
        latents = run()
        assert torch.is_tensor(latents) and latents.shape == (2, 4, x_T.shape[-2], x_T.shape[-1])
        with torch.no_grad():
            assert np.array_equal(ptp_utils.latent2image(vae_, latents)[0], images[0])
    finally:
        torch.backends.cudnn.enabled = det


def test_null_inversion_takes_an_image(cuda):
    """NullInversion.invert from a uint8 array.  The U-Net here is not test_gpu_pndm's SMALL_UNET: its
    head dims (8 and 16) have no attention backward (p2p_attn_bwd serves 40 / 64 / 80 / 160), which
    the null-text optimisation needs; 64 channels in one head (d = 64) do."""
    model = pl.SyntheticStableDiffusion(device=cuda, dtype=torch.bfloat16,
                                        unet_config=dict(block_out_channels=(64, 64, 64, 64), heads=1),
                                        vae_config=NARROW_VAE)
    image = np.random.default_rng(12).integers(0, 256, size=(128, 128, 3), dtype=np.uint8)
    inv = null_text.NullInversion(model, num_ddim_steps=3)
    seen = {}
    loop = inv.ddim_loop
    inv.ddim_loop = lambda latent: seen.setdefault("trajectory", loop(latent))
    (image_gt, image_rec), x_T, embs = inv.invert(image, PROMPTS[0], num_inner_steps=1)
    assert image_gt is image and image_rec.dtype == np.uint8 and image_rec.shape == (128, 128, 3)
    assert x_T.shape == (1, 4, 64, 64) and torch.isfinite(x_T).all() and len(embs) == 3
    x = (torch.from_numpy(image).float() / 127.5 - 1).permute(2, 0, 1)[None].contiguous().to(cuda, torch.bfloat16)
    with torch.no_grad():
        want = model.vae.encode(x)["latent_dist"].mean * 0.18215
    first = seen["trajectory"][0]
    assert first.shape == (1, 4, 64, 64) and torch.equal(first.float(), want.float())
