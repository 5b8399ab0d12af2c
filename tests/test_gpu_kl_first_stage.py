"""GPU tier: the KL first stage — stedm_gauss_sample (the posterior's sampling kernel), stedm_amd.vq.AutoencoderKL against the reference's own
Encoder / Decoder outputs (tests/golden/f27_kl_first_stage.npz) and the CPU oracle, and an S_ZSS_DM built from the reference's target string:
get_input's per-sample posterior draw, scale_by_std, one training step and predict_step."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stedm_amd.utils import prng

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "f27_kl_names.json")) as _f:
    KL_CASES = json.load(_f)
LOSS = {"target": "ldm.modules.losses.LPIPSWithDiscriminator", "params": {"disc_start": 50001, "kl_weight": 1e-6, "disc_weight": 0.5}}
SCALE = 0.18215          # kl-f8's published scale_factor: not a power of two, so the kernel's last product rounds


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a = a.double().cpu(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max()) / (float(b.std()) + 1e-12)


# ------------------------------------------------------------------------------------------------ the kernel
KERNEL_SHAPES = [(3, 3, 5, 5),        # rows of 75 elements: the scalar tail form, a last group of three
                 (2, 4, 64, 64)]      # rows of 16384 elements: float4 form, 16 blocks per sample


def _moments(shape, dev):
    """mean ~ N(0, 1); log-variances over -45 .. 35, beyond both ends of the clamp, with -30 and 20 themselves among them"""
    B, C, H, W = shape
    mean = prng.normal(27, f"k.mean.{shape}", shape)
    lv = prng.uniform(27, f"k.lv.{shape}", shape, -45.0, 35.0)
    lv.view(-1)[:4] = torch.tensor([-30.0, 20.0, -44.5, 34.5])
    assert float(lv.min()) < -30 and float(lv.max()) > 20
    return torch.cat([mean, lv], 1).contiguous().to(dev), mean, lv


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_gauss_sample_given_noise_against_fp64(dev, shape):
    """|delta| <= 8 * 2^-24 * |scale| * (|mean| + std |noise|) per element: expf within 2 ulp plus at most four roundings (0.5 * logvar is
    exact; std * noise, the sum, the scale), with headroom. Mode: scale * mean is one rounding, so bit-exact."""
    from stedm_amd import ops
    m, mean, lv = _moments(shape, dev)
    noise = prng.normal(27, f"k.noise.{shape}", shape)
    s32 = float(np.float32(SCALE))
    for scale in (1.0, SCALE):
        got = ops.gauss_sample(m, noise.to(dev), scale=scale).cpu().double()
        sc = 1.0 if scale == 1.0 else s32
        std = torch.exp(0.5 * lv.double().clamp(-30.0, 20.0))
        ref = sc * (mean.double() + std * noise.double())
        bound = 8 * 2.0 ** -24 * abs(sc) * (mean.double().abs() + std * noise.double().abs())
        worst = float(((got - ref).abs() / bound).max())
        print(f"[gauss_sample {shape} scale {scale}] worst |delta| / bound {worst:.3f}")
        assert torch.isfinite(got).all() and worst <= 1.0
        mode = ops.gauss_sample(m, scale=scale, mode=True)
        assert torch.equal(mode.cpu(), torch.tensor(scale, dtype=torch.float32) * mean)
    # an operand off the 16-byte grid takes the scalar form: the same bits
    buf = torch.empty(m.numel() + 1, device=dev)
    off = buf[1:].view(m.shape)
    off.copy_(m)
    assert off.data_ptr() % 16 != 0
    assert torch.equal(ops.gauss_sample(off, noise.to(dev), scale=SCALE), ops.gauss_sample(m, noise.to(dev), scale=SCALE))


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_gauss_sample_in_kernel_draw(dev, shape):
    from stedm_amd import ops
    from stedm_amd._lib import STREAM_POSTERIOR
    B, C, H, W = shape
    m, _, _ = _moments(shape, dev)
    seed = 0x5EED0000 + B
    drawn = ops.gauss_sample(m, None, scale=SCALE, seed=seed, first_id=5)
    rows = ops.philox_normal(B, (C, H, W), seed, STREAM_POSTERIOR, dev, first_id=5)
    assert torch.equal(drawn, ops.gauss_sample(m, rows, scale=SCALE))                         # the draw is philox_normal's row, bit for bit
    assert torch.equal(drawn, ops.gauss_sample(m, None, scale=SCALE, seed=seed, first_id=5))   # two identical calls
    assert not torch.equal(drawn, ops.gauss_sample(m, None, scale=SCALE, seed=seed + 1, first_id=5))
    assert not torch.equal(drawn, ops.gauss_sample(m, None, scale=SCALE, seed=seed, first_id=6))
    # a sample's latent depends on its global id, not on its place in the call: rows [2:4] of a batch of 4 = a batch of 2 at first_id 2
    m4, _, _ = _moments((4, C, H, W), dev)
    whole = ops.gauss_sample(m4, None, scale=SCALE, seed=seed, first_id=0)
    part = ops.gauss_sample(m4[2:4].contiguous(), None, scale=SCALE, seed=seed, first_id=2)
    assert torch.equal(whole[2:4], part)
    # no sampler's stream: 1 + iteration, 0x8000 + i, 0x10000 + t (include/stedm_hip.h)
    assert STREAM_POSTERIOR >= 0x10000 + 0x10000 and STREAM_POSTERIOR & 0xFFFF == 0


def test_distribution_sample_on_the_device(dev):
    """DiagonalGaussianDistribution.sample on GPU tensors: given noise, a seed, torch's CPU generator for the seed, and the deterministic
    variant (the mode flag)"""
    from stedm_amd import ops
    from stedm_amd.distributions import DiagonalGaussianDistribution
    m, mean, _ = _moments((3, 3, 5, 5), dev)
    d = DiagonalGaussianDistribution(m)
    n = prng.normal(27, "d.noise", (3, 3, 5, 5)).to(dev)
    assert torch.equal(d.sample(noise=n), ops.gauss_sample(m, n))
    assert torch.equal(d.sample(seed=9, sample_id0=4), ops.gauss_sample(m, None, seed=9, first_id=4))
    torch.manual_seed(21)
    a = d.sample()
    torch.manual_seed(21)
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    assert torch.equal(a, ops.gauss_sample(m, None, seed=seed))
    det = DiagonalGaussianDistribution(m, deterministic=True)
    assert torch.equal(det.sample().cpu(), mean) and torch.equal(det.mode().cpu(), mean)
    assert d.kl().shape == (3,) and d.nll(a).shape == (3,) and d.kl().is_cuda


# ------------------------------------------------------------------------------------------------ encoder / decoder / interface
def build(tag, dev, precision="parity"):
    from stedm_amd.vq import AutoencoderKL
    c = KL_CASES[tag]
    m = AutoencoderKL(ddconfig=c["ddconfig"], lossconfig=LOSS, embed_dim=c["embed_dim"], precision=precision).eval()
    prng.fill_module_(m, seed=27)
    return m.to(dev)


def inputs(tag):
    c = KL_CASES[tag]
    f = 2 ** (len(c["ddconfig"]["ch_mult"]) - 1)
    return prng.uniform(27, f"kl.{tag}.x", (2, 3, 64, 64)), prng.normal(27, f"kl.{tag}.z", (2, c["embed_dim"], 64 // f, 64 // f))


@pytest.fixture(scope="module")
def stages(dev):
    return {tag: build(tag, dev) for tag in KL_CASES}


@pytest.mark.parametrize("tag", sorted(KL_CASES))
def test_encoder_decoder_vs_reference_golden(dev, golden, stages, tag):
    """the bounds tests/test_gpu_vq.py::test_encoder_decoder_vs_reference_golden holds the VQ stage to"""
    from stedm_amd import ops
    fx = golden("f27_kl_first_stage")
    m = stages[tag]
    x, z = (t.to(dev) for t in inputs(tag))
    zin = ops.conv1x1_nchw(z, m.post_quant_conv.weight, m.post_quant_conv.bias)
    m._prepare(); m._cs = {}
    e1 = rel(m._encoder(x), fx[f"{tag}.enc_out"])
    m._cs = {}
    yd = m._decoder(zin)
    e2 = rel(yd, fx[f"{tag}.dec_out"])
    print(f"[KL {tag} parity] encoder {e1:.3e}, decoder {e2:.3e} max/std vs reference golden")
    assert e1 < 1e-3 and e2 < 1e-3
    try:
        for precision in ("f16", "bf16"):
            m.set_precision(precision)
            m._prepare(); m._cs = {}
            a = rel(m._encoder(x), fx[f"{tag}.enc_out"])
            m._cs = {}
            yd2 = m._decoder(zin)
            b = float((yd2.double() - yd.double()).norm() / yd.double().norm())
            print(f"[KL {tag} {precision}] encoder max/std vs golden {a:.3e}; decoder rel-L2 vs parity mode {b:.3e}")
            assert a < 0.2 and b < 0.1
    finally:
        m.set_precision("parity")


@pytest.mark.parametrize("tag", sorted(KL_CASES))
def test_interface_vs_golden_and_oracle(dev, golden, stages, tag):
    """encode(x).parameters and decode(z) (autoencoder.py:324-333) against the reference's outputs and against oracle.vq's encoder / decoder
    run on the module's own state dict (the oracle reads the state dict by name and takes the wider conv_out as it is)"""
    from oracle import vq as ovq
    from stedm_amd.distributions import DiagonalGaussianDistribution
    fx = golden("f27_kl_first_stage")
    m = stages[tag]
    c = KL_CASES[tag]
    dd = c["ddconfig"]
    x, z = inputs(tag)
    post = m.encode(x.to(dev))
    assert isinstance(post, DiagonalGaussianDistribution) and tuple(post.parameters.shape) == tuple(fx[f"{tag}.moments"].shape)
    dec = m.decode(z.to(dev))
    assert rel(post.parameters, fx[f"{tag}.moments"]) < 1e-3 and rel(dec, fx[f"{tag}.dec_out"]) < 1e-3
    assert rel(post.mean, fx[f"{tag}.mean"]) < 1e-3 and rel(post.std, fx[f"{tag}.std"]) < 1e-3
    P = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    cfg = ovq.VQConfig(ch=dd["ch"], ch_mult=tuple(dd["ch_mult"]), num_res_blocks=dd["num_res_blocks"], z_channels=dd["z_channels"],
                       embed_dim=c["embed_dim"])
    ref_m = F.conv2d(ovq.encoder(P, cfg, x), P["quant_conv.weight"], P["quant_conv.bias"])
    ref_d = ovq.decoder(P, cfg, F.conv2d(z, P["post_quant_conv.weight"], P["post_quant_conv.bias"]))
    assert rel(post.parameters, ref_m) < 1e-3 and rel(dec, ref_d) < 1e-3
    # forward (autoencoder.py:335-342): the mode's decode, and a sampled one
    d0, p0 = m(x.to(dev), sample_posterior=False)
    assert torch.equal(p0.parameters, post.parameters) and torch.equal(d0, m.decode(post.mode()))
    torch.manual_seed(1)
    d1, _ = m(x.to(dev))
    assert d1.shape == d0.shape and bool(torch.isfinite(d1).all()) and not torch.equal(d1, d0)
    # batch_invariant, as on the VQ stage: a sample's bits do not depend on the batch of its call
    m.batch_invariant = True
    try:
        assert torch.equal(m.encode(x.to(dev)).parameters[:1], m.encode(x[:1].to(dev)).parameters)
        assert torch.equal(m.decode(z.to(dev))[1:], m.decode(z[1:].to(dev)))
    finally:
        m.batch_invariant = False


# ------------------------------------------------------------------------------------------------ through S_ZSS_DM
@pytest.fixture(scope="module")
def module(dev):
    """LDM_Diffusion over an S_ZSS_DM whose first stage is the reference's YAML dict for the KL stage (three levels, embed_dim 4 =
    the U-Net's latent channels; 64^2 images -> 16^2 latents = the U-Net's image_size)"""
    from stedm_amd.ldm_module import LDM_Diffusion
    from tests.test_gpu_train import _module_cfg
    c = KL_CASES["kl_f4e"]
    cfg = _module_cfg()
    assert cfg["diffusion"]["channels"] == c["embed_dim"] and cfg["diffusion"]["image_size"] == 16
    cfg["diffusion"]["first_stage_config"] = {"target": "ldm.models.autoencoder.AutoencoderKL",
                                              "params": dict(embed_dim=c["embed_dim"], ddconfig=c["ddconfig"], lossconfig=LOSS, monitor="val/rec_loss")}
    mod = LDM_Diffusion(cfg, accumulate_grad_batches=1)
    zm = mod._model
    assert type(zm.first_stage_model).__name__ == "AutoencoderKL"
    prng.fill_module_(zm.model.diffusion_model, seed=6); prng.fill_module_(zm.cond_stage_model, seed=9); prng.fill_module_(zm.agg_block, seed=51)
    prng.fill_module_(zm.first_stage_model, seed=27)
    return mod.to(dev).eval()


def _posterior(zm, lb):
    x = lb["image"].permute(0, 3, 1, 2).float().contiguous()
    return zm.first_stage_model.encode(x)


def test_get_input_draws_the_posterior_per_sample(dev, module):
    from stedm_amd import ops
    from stedm_amd._lib import STREAM_POSTERIOR
    from tests.test_gpu_train import _module_batches
    zm = module._model
    lb = module.prepare_batch(_module_batches(dev, 1)[0])
    zm.scale_factor = SCALE
    try:
        z, c = zm.get_input(lb, "image", posterior_seed=1234)[:2]
        assert tuple(z.shape) == (2, 4, 16, 16) and set(c) == {"c_concat", "c_crossattn"}
        post = _posterior(zm, lb)
        rows = ops.philox_normal(2, (4, 16, 16), 1234, STREAM_POSTERIOR, dev, first_id=0)
        assert torch.equal(z, ops.gauss_sample(post.parameters, rows, scale=SCALE))          # scale_factor * (mean + std * philox row)
        ref = SCALE * (post.mean.double() + post.std.double() * rows.double())
        assert float((z.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        assert torch.equal(z, zm.get_input(lb, "image", posterior_seed=1234)[0])
        shifted = zm.get_input(lb, "image", posterior_seed=1234, sample_id0=1)[0]
        assert not torch.equal(z, shifted)
        assert torch.equal(shifted[0], ops.gauss_sample(post.parameters, None, scale=SCALE, seed=1234, first_id=1)[0])
        # the tiled encode is refused on this stage, the tiled decode works
        split = {"ks": (32, 32), "stride": (16, 16), "vqf": 4, "patch_distributed_vq": True, "tie_braker": False, "clip_max_weight": 0.5,
                 "clip_min_weight": 0.01, "clip_max_tie_weight": 0.5, "clip_min_tie_weight": 0.01}
        with pytest.raises(NotImplementedError, match="tiled"):
            zm.encode_first_stage(lb["image"].permute(0, 3, 1, 2).float().contiguous(), split=split)
        tiled = zm.decode_first_stage(z, split=dict(split, ks=(16, 16), stride=(16, 16)))     # one crop: the plain decode's value
        assert rel(tiled, zm.decode_first_stage(z).cpu()) < 1e-3
    finally:
        zm.scale_factor = 1.0


def test_scale_by_std_uses_exactly_that_sample(dev, module):
    """ddpm.py:479-494 on the KL stage: scale_factor = 1 / std of the first batch's sampled latents, the seed drawn from torch's CPU generator"""
    from stedm_amd import ops
    from tests.test_gpu_train import _module_batches
    zm = module._model
    lb = module.prepare_batch(_module_batches(dev, 1)[0])
    zm.scale_by_std, zm.scale_factor = True, 1.0
    zm.__dict__.pop("_std_rescaled", None)
    try:
        torch.manual_seed(77)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        torch.manual_seed(77)
        zm.on_train_batch_start(lb, 0)
        z = ops.gauss_sample(_posterior(zm, lb).parameters, None, scale=1.0, seed=seed)
        assert torch.equal(torch.as_tensor(zm.scale_factor, device=dev), 1.0 / z.flatten().std())
        assert 0.05 < float(zm.scale_factor) < 50.0
        sf = zm.scale_factor
        zm.on_train_batch_start(lb, 0)                     # once only
        assert zm.scale_factor is sf
        # the rescaled latents: unit std, and decode_first_stage divides the scale out again
        z1 = zm.get_input(lb, "image", posterior_seed=seed)[0]
        assert abs(float(z1.flatten().std()) - 1.0) < 1e-5
        assert rel(zm.decode_first_stage(z1), zm.first_stage_model.decode(z).cpu()) < 1e-3
    finally:
        zm.scale_by_std, zm.scale_factor = False, 1.0
        zm.__dict__.pop("_std_rescaled", None)


def test_predict_step_decodes_through_the_kl_stage(dev, module):
    """predict_step: sampled latents -> decode_first_stage -> uint8; the decoded floats against oracle.vq.decoder on the same latents,
    the uint8 image within one level everywhere (truncating cast)"""
    from oracle import vq as ovq
    from stedm_amd.latent_diffusion import predict_latents
    from tests.test_gpu_train import _module_batches
    zm = module._model
    batch = _module_batches(dev, 1)[0]
    torch.manual_seed(3)
    img, seg = module.predict_step(batch, 0)
    assert img.shape == (2, 64, 64, 3) and img.dtype == np.uint8 and seg.shape == (2, 64, 64)
    torch.manual_seed(3)
    lat = predict_latents(zm, module.prepare_batch(batch), ddim_steps=4, eta=0.0, cfg_scale=1.5, style_sampling="mp")
    c = KL_CASES["kl_f4e"]
    dd = c["ddconfig"]
    cfg = ovq.VQConfig(ch=dd["ch"], ch_mult=tuple(dd["ch_mult"]), num_res_blocks=dd["num_res_blocks"], z_channels=dd["z_channels"],
                       embed_dim=c["embed_dim"])
    P = {k: v.detach().cpu() for k, v in zm.first_stage_model.state_dict().items()}
    ref = ovq.decoder(P, cfg, F.conv2d(lat.cpu(), P["post_quant_conv.weight"], P["post_quant_conv.bias"]))
    assert rel(zm.decode_first_stage(lat), ref) < 1e-3
    ref8 = ((np.clip(ref.permute(0, 2, 3, 1).numpy(), -1, 1) + 1) * 127.5).astype(np.uint8)
    assert np.abs(img.astype(np.int32) - ref8.astype(np.int32)).max() <= 1


def test_training_step_on_kl_latents(dev, module):
    """one fused training step on latents sampled from the KL posterior: a finite loss, and the U-Net's parameters move"""
    from tests.test_gpu_train import _module_batches
    zm = module._model
    lb = module.prepare_batch(_module_batches(dev, 1)[0])
    module.train()
    try:
        zm.configure_trainer(lr=1e-3, accumulate_grad_batches=1)
        torch.manual_seed(5)
        x, c = zm.get_input(lb, "image", posterior_seed=99)[:2]
        before = [p.detach().clone() for p in zm.model.diffusion_model.parameters()]
        loss = zm.training_step_hip(x, c)
        assert bool(torch.isfinite(loss).all()) and float(loss) > 0
        moved = sum(not torch.equal(a, b) for a, b in zip(before, zm.model.diffusion_model.parameters()))
        assert moved == len(before), f"{moved} of {len(before)} U-Net parameters changed"
        assert all(not p.requires_grad for p in zm.first_stage_model.parameters())
    finally:
        module.eval()
