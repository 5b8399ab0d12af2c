"""CPU tier: the KL first stage's host side — stedm_amd.vq.AutoencoderKL / IdentityFirstStage, stedm_amd.distributions and their wiring
through LatentDiffusion — against tests/golden/f27_kl_first_stage.npz and f27_kl_names.json (written by tests/golden/make_golden_kl.py from the
reference's own Encoder / Decoder / DiagonalGaussianDistribution). No device call is made: the refusals must raise before one."""
import json
import os

import numpy as np
import pytest
import torch

from stedm_amd.utils import prng

torch.set_grad_enabled(False)
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "f27_kl_names.json")) as _f:
    KL_CASES = json.load(_f)
LOSS = {"target": "ldm.modules.losses.LPIPSWithDiscriminator", "params": {"disc_start": 50001, "kl_weight": 1e-6, "disc_weight": 0.5}}


def T(a):
    return torch.from_numpy(np.asarray(a))


def _kl(tag, **kw):
    from stedm_amd.vq import AutoencoderKL
    c = KL_CASES[tag]
    return AutoencoderKL(ddconfig=c["ddconfig"], lossconfig=LOSS, embed_dim=c["embed_dim"], **kw)


def _ld(first_stage=None, **kw):
    from stedm_amd.latent_diffusion import LatentDiffusion
    return LatentDiffusion(torch.nn.Conv2d(4, 4, 1), linear_start=0.0015, linear_end=0.0205, image_size=8, channels=4, conditioning_key="hybrid",
                           loss_type="l1", first_stage_config=first_stage, **kw)


@pytest.mark.parametrize("tag", sorted(KL_CASES))
def test_state_dict_names_shapes_and_order(tag):
    """AutoencoderKL.state_dict(): the names, shapes and ORDER of the reference's encoder, decoder, quant_conv, post_quant_conv (a
    checkpoint's loss.* keys have no place in it); every parameter frozen; the surface the callers read."""
    m = _kl(tag)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == KL_CASES[tag]["params"]
    assert all(not p.requires_grad for p in m.parameters())
    dd, e = KL_CASES[tag]["ddconfig"], KL_CASES[tag]["embed_dim"]
    assert tuple(m.quant_conv.weight.shape) == (2 * e, 2 * dd["z_channels"], 1, 1) and tuple(m.post_quant_conv.weight.shape) == (dd["z_channels"], e, 1, 1)
    assert isinstance(m.loss, torch.nn.Identity) and m.encoder.num_resolutions == len(dd["ch_mult"]) and m.batch_invariant is False
    assert m.embed_dim == e and m.image_key == "image"


def test_vq_interface_still_shares_the_engine():
    from stedm_amd import vq
    assert issubclass(vq.VQModelInterface, vq.FirstStageEngine) and issubclass(vq.AutoencoderKL, vq.FirstStageEngine)
    for name in ("_prepare", "_walk", "_res", "_attn", "_down", "_up", "_encoder", "_decoder"):
        assert name not in vq.VQModelInterface.__dict__ and name not in vq.AutoencoderKL.__dict__ and hasattr(vq.FirstStageEngine, name)


def test_checkpoint_with_loss_keys_loads(tmp_path):
    """init_from_ckpt: a reference checkpoint carries loss.* (LPIPS, discriminator) beside the stage's own keys; they are dropped"""
    src = _kl("kl_tiny")
    prng.fill_module_(src, seed=3)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    sd["loss.logvar"] = torch.zeros(())
    sd["loss.discriminator.main.0.weight"] = torch.zeros(4, 3, 4, 4)
    path = str(tmp_path / "kl.ckpt")
    torch.save({"state_dict": sd}, path)
    m = _kl("kl_tiny", ckpt_path=path)
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in m.state_dict().items())
    assert all(not p.requires_grad for p in m.parameters())


def test_instantiate_first_stage_builds_the_three_targets():
    from stedm_amd import vq
    from stedm_amd.latent_diffusion import instantiate_first_stage
    c = KL_CASES["kl_f4e"]
    params = dict(ddconfig=c["ddconfig"], lossconfig=LOSS, embed_dim=c["embed_dim"], monitor="val/rec_loss")
    for target in ("ldm.models.autoencoder.AutoencoderKL", "stedm_amd.vq.AutoencoderKL"):
        m = instantiate_first_stage({"target": target, "params": params})
        assert type(m) is vq.AutoencoderKL and not m.training and m.monitor == "val/rec_loss"
    for vqi in (False, True):
        m = instantiate_first_stage({"target": "ldm.models.autoencoder.IdentityFirstStage", "params": {"vq_interface": vqi}})
        assert type(m) is vq.IdentityFirstStage and not m.training
        x = torch.arange(6.0).view(1, 1, 2, 3)
        assert m.encode(x) is x and m.decode(x) is x and m(x) is x
        q = m.quantize(x)
        assert (q[0] is x and q[1] is None and list(q[2]) == [None, None, None]) if vqi else q is x
    ld = _ld({"target": "ldm.models.autoencoder.AutoencoderKL", "params": params})
    assert type(ld.first_stage_model) is vq.AutoencoderKL


def test_construction_refusals():
    from stedm_amd.vq import AutoencoderKL
    dd = KL_CASES["kl_tiny"]["ddconfig"]
    with pytest.raises(ValueError, match="double_z"):
        AutoencoderKL(ddconfig=dict(dd, double_z=False), lossconfig=LOSS, embed_dim=4)
    with pytest.raises(NotImplementedError, match="up to 8"):
        AutoencoderKL(ddconfig=dict(dd, z_channels=5), lossconfig=LOSS, embed_dim=4)          # 2 z = 10 > 8
    AutoencoderKL(ddconfig=dict(dd, z_channels=4), lossconfig=LOSS, embed_dim=3)              # 2 z = 8: the limit itself is served


# ------------------------------------------------------------------------------------------------ the distribution
def _close(a, b):
    """fp32 rounding of a sum of a few hundred terms: a handful of ulps of the result"""
    return torch.allclose(a, b, rtol=2e-6, atol=0)


def test_distribution_against_the_reference_class(golden):
    from stedm_amd.distributions import DiagonalGaussianDistribution
    fx = golden("f27_kl_first_stage")
    g = lambda k: T(fx["dist." + k])
    lv_in = g("moments")[:, 4:]
    assert float(lv_in.min()) == -60.0 and float(lv_in.max()) == 40.0 and bool((lv_in == -30.0).any()) and bool((lv_in == 20.0).any())
    d = DiagonalGaussianDistribution(g("moments"))
    assert d.parameters is not None and d.deterministic is False
    # the expressions are the reference's, term for term: exact
    for name in ("mean", "logvar", "std", "var"):
        assert torch.equal(getattr(d, name), g(name)), name
    assert float(d.logvar.min()) == -30.0 and float(d.logvar.max()) == 20.0
    assert torch.equal(d.mode(), g("mode"))
    other = DiagonalGaussianDistribution(g("other"))
    s = g("sample")
    for got, want in ((d.kl(), g("kl")), (d.kl(other), g("kl_other")), (d.nll(s), g("nll")), (d.nll(s, dims=[1]), g("nll_dim1"))):
        assert got.shape == want.shape and _close(got, want)
    det = DiagonalGaussianDistribution(g("moments"), deterministic=True)
    assert torch.equal(det.std, g("det.std")) and torch.equal(det.var, g("det.var")) and not det.std.any()
    assert torch.equal(det.kl(), g("det.kl")) and torch.equal(det.nll(s), g("det.nll")) and torch.equal(det.mode(), g("det.mode"))
    assert torch.equal(det.sample(noise=s), det.mean)


@pytest.mark.parametrize("tag", sorted(KL_CASES))
def test_distribution_on_the_real_cases(golden, tag):
    from stedm_amd.distributions import DiagonalGaussianDistribution
    fx = golden("f27_kl_first_stage")
    g = lambda k: T(fx[f"{tag}.{k}"])
    d = DiagonalGaussianDistribution(g("moments"))
    for name in ("mean", "logvar", "std", "var"):
        assert torch.equal(getattr(d, name), g(name)), name
    e = KL_CASES[tag]["embed_dim"]
    z = prng.normal(27, f"kl.{tag}.z", tuple(d.mean.shape))
    assert d.mean.shape[1] == e and _close(d.kl(), g("kl")) and _close(d.nll(z), g("nll"))


def test_sample_on_cpu_tensors(golden):
    from stedm_amd.distributions import DiagonalGaussianDistribution
    d = DiagonalGaussianDistribution(T(golden("f27_kl_first_stage")["dist.moments"]))
    n = prng.normal(27, "cpu.noise", tuple(d.mean.shape))
    assert torch.equal(d.sample(noise=n), d.mean + d.std * n)
    torch.manual_seed(5)
    a = d.sample()
    torch.manual_seed(5)
    assert torch.equal(a, d.mean + d.std * torch.randn(d.mean.shape))
    with pytest.raises(ValueError, match="seed"):
        d.sample(seed=1)
    with pytest.raises(ValueError, match="seed"):
        d.sample(noise=n, seed=1)


# ------------------------------------------------------------------------------------------------ LatentDiffusion
def test_get_first_stage_encoding(golden):
    from stedm_amd.distributions import DiagonalGaussianDistribution
    ld = _ld(scale_factor=0.25)
    z = prng.normal(27, "gfe.z", (2, 4, 8, 8))
    assert torch.equal(ld.get_first_stage_encoding(z), 0.25 * z)                              # the tensor path, unchanged
    d = DiagonalGaussianDistribution(T(golden("f27_kl_first_stage")["kl_tiny.moments"]))
    n = prng.normal(27, "gfe.n", tuple(d.mean.shape))
    assert torch.equal(ld.get_first_stage_encoding(d, noise=n), 0.25 * (d.mean + d.std * n))
    torch.manual_seed(9)
    a = ld.get_first_stage_encoding(d)
    torch.manual_seed(9)
    assert torch.equal(a, 0.25 * (d.mean + d.std * torch.randn(d.mean.shape)))
    with pytest.raises(ValueError):
        ld.get_first_stage_encoding(d, seed=3)                                                # CPU tensors: no device bits to promise
    for bad in (object(), [z], None):
        with pytest.raises(NotImplementedError, match="not yet implemented"):
            ld.get_first_stage_encoding(bad)


class _NoDevice(torch.nn.Module):
    """a first stage whose arithmetic must not be reached"""

    def encode(self, *a, **k):
        raise AssertionError("device work before the refusal")

    decode = _encoder = _decoder = _prepare = encode


def test_refusals_come_before_any_device_work():
    from stedm_amd.ddim import DDIMSampler, first_stage_codebook
    kl = _kl("kl_tiny")
    kl.encode = kl.decode = kl._prepare = _NoDevice().encode
    ld = _ld(kl)
    ld.apply_model = _NoDevice().encode
    split = {"ks": (32, 32), "stride": (16, 16), "vqf": 8, "patch_distributed_vq": True, "tie_braker": False, "clip_max_weight": 0.5,
             "clip_min_weight": 0.01, "clip_max_tie_weight": 0.5, "clip_min_tie_weight": 0.01}
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="tiled"):
        ld.encode_first_stage(x, split=split)
    ld.split_input_params = dict(split)
    with pytest.raises(NotImplementedError, match="tiled"):
        ld.encode_first_stage(x)
    del ld.split_input_params
    for option in ("quantize_x0", "quantize_denoised"):
        with pytest.raises(NotImplementedError, match="AutoencoderKL"):
            first_stage_codebook(ld, 4, option)
    with pytest.raises(NotImplementedError, match="VQ first stage"):
        DDIMSampler(ld).sample(2, 1, (4, 8, 8), conditioning=None, quantize_x0=True, verbose=False)
    with pytest.raises(NotImplementedError, match="VQ first stage"):
        ld.sample(None, batch_size=1, shape=(1, 4, 8, 8), quantize_denoised=True, verbose=False)
    from stedm_amd.vq import IdentityFirstStage
    ld.first_stage_model = IdentityFirstStage(vq_interface=True)
    with pytest.raises(NotImplementedError, match="IdentityFirstStage"):
        first_stage_codebook(ld, 4, "quantize_x0")


def test_get_input_keywords_reach_the_posterior_and_are_ignored_by_a_tensor_stage():
    """get_input(..., posterior_seed, sample_id0): handed to the posterior's sample; a stage that returns a tensor never sees them"""
    from stedm_amd.distributions import DiagonalGaussianDistribution
    seen = {}

    class Post(DiagonalGaussianDistribution):
        def sample(self, noise=None, seed=None, sample_id0=0, scale=1.0):
            seen.update(seed=seed, sample_id0=sample_id0, scale=scale)
            return scale * self.mean

    class Stage(torch.nn.Module):
        def __init__(self, kl):
            super().__init__()
            self.kl = kl

        def encode(self, x):
            m = torch.cat([x[:, :, ::8, ::8], x[:, :1, ::8, ::8]], 1)                         # [B, 4, 8, 8]
            return Post(torch.cat([m, 0 * m], 1)) if self.kl else m

    batch = {"image": prng.uniform(27, "gi.x", (2, 64, 64, 3)), "segmentation": torch.zeros(2, 8, 8, 3)}
    for kl in (True, False):
        ld = _ld(Stage(kl), scale_factor=0.5, cond_stage_key="segmentation", cond_stage_trainable=True)
        seen.clear()
        z = ld.get_input(batch, "image", posterior_seed=77, sample_id0=6)[0]
        x = batch["image"].permute(0, 3, 1, 2)
        assert torch.equal(z, 0.5 * torch.cat([x[:, :, ::8, ::8], x[:, :1, ::8, ::8]], 1))
        assert seen == (dict(seed=77, sample_id0=6, scale=0.5) if kl else {})
        seen.clear()
        ld.get_input(batch, "image")
        assert seen == (dict(seed=None, sample_id0=0, scale=0.5) if kl else {})
