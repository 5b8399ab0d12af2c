"""CPU tier: ancestral DDPM sampling (stedm_amd/ancestral.py, LatentDiffusion.sample / sample_log(ddim=False)) against fixture F20, the
reference's own LatentDiffusion.sample / p_sample_loop / p_sample with a closed-form eps model (tests/golden/make_golden_ddpm.py).
  * the product's seven posterior buffers equal F20's (the reference's register_schedule) bit for bit;
  * `ref_ddpm_sample`, a test-local fp32 restatement of p_sample_loop over F20's buffers, reproduces every case within F20_TOL, and the
    clamp fires in `full`; it is the yardstick the GPU tier runs over the oracle U-Net;
  * the product's step table through `ddpm_update_ref` (stedm_ddpm_step's formula in torch) reproduces that loop bit for bit;
  * AncestralSampler's own loop on the CPU, the kernel replaced by `ddpm_update_ref` behind the same interface, reproduces the restated
    loop bit for bit, blends after the step and logs a list by the reference's rule;
  * the refusals raise before any device work; the state dict keeps its keys; "ddpm" is a known sampler and DDIM stays the default.
Bit-for-bit comparisons are made only between loops computed in the same process; against the stored fixture within F20_TOL (see the
generator's docstring: the toy model's tanh can round differently by an ulp on another CPU or libm build)."""
import numpy as np
import pytest
import torch

from oracle import ddim as od
from stedm_amd.utils import prng

torch.set_grad_enabled(False)

SEED, SHAPE = 20, (2, 4, 8, 8)
CASES = ("full", "short", "masked")
BUFFERS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
           "posterior_mean_coef1", "posterior_mean_coef2", "log_one_minus_alphas_cumprod")
F20_TOL = 1e-4          # max |diff| / max |ref| against the stored fixture


def toy_eps(x, t, bias):
    """F20's closed-form eps model (the one of F10 / F19)."""
    tf = t.float()[:, None, None, None] / 1000.0
    return torch.tanh(x * (0.5 + tf) + bias) * (0.8 + 0.3 * tf) + 0.1 * bias


def step_noises(name, T):
    """noise_like's draw of F20 case `name` at step k (t = T - 1 - k)."""
    return [prng.normal(SEED, f"ddpm.{name}.n{k}", SHAPE) for k in range(T)]


def q_noises(name, T):
    """q_sample's draw of the masked case at step k."""
    return [prng.normal(SEED, f"ddpm.{name}.q{k}", SHAPE) for k in range(T)]


def f20_buffers(golden):
    f = golden("f20_ddpm")
    return {b: torch.from_numpy(np.asarray(f[b])) for b in BUFFERS}


def f20_case(golden, name):
    f = golden("f20_ddpm")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    T = int(f[f"{name}_T"])
    c = {"xT": g("xT"), "cond": g("cond"), "T": T, "clip": bool(int(f[f"{name}_clip"])), "out": g(f"{name}_out"),
         "clamped": int(f[f"{name}_clamped"]), "n_inter": int(f[f"{name}_n_inter"]), "noises": step_noises(name, T),
         "mask": None, "x0": None, "q_noises": None}
    if name == "masked":
        c.update(mask=g("mask"), x0=g("x0"), q_noises=q_noises(name, T))
    if name == "full":
        c["inter"] = g("full_inter")
    return c


def rel_max(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


# ------------------------------------------------------------------------------------------------ test-local restatement
def ref_ddpm_sample(eps_fn, x_T, T, bufs, clip=True, cond=None, noises=None, mask=None, x0=None, q_noises=None, log_every_t=100,
                    stats=None):
    """p_sample_loop (ddpm.py:1169-1217) with p_sample / p_mean_variance / predict_start_from_noise / q_posterior (:219-232, 1050-1110)
    on `eps_fn(x, t, c)` in fp32 torch, from the fp32 buffers `bufs` (+ the oracle schedule's q_sample). noises[k] / q_noises[k]: the
    draws of step k (t = T - 1 - k). stats: dict receiving the clamp count. Returns (img, intermediates list)."""
    sched = od.Schedule()
    img = x_T.clone().float()
    b = img.shape[0]
    ex = lambda a, t: a[t].reshape(b, 1, 1, 1)
    inter = [img]
    clamped = 0
    for k, i in enumerate(range(T - 1, -1, -1)):
        t = torch.full((b,), i, dtype=torch.long)
        eps = eps_fn(img, t, cond)
        x_recon = ex(bufs["sqrt_recip_alphas_cumprod"], t) * img - ex(bufs["sqrt_recipm1_alphas_cumprod"], t) * eps
        if clip:
            clamped += int((x_recon.abs() > 1).sum())
            x_recon.clamp_(-1., 1.)
        mean = ex(bufs["posterior_mean_coef1"], t) * x_recon + ex(bufs["posterior_mean_coef2"], t) * img
        log_var = ex(bufs["posterior_log_variance_clipped"], t)
        nonzero_mask = (1 - (t == 0).float()).reshape(b, 1, 1, 1)
        img = mean + nonzero_mask * (0.5 * log_var).exp() * noises[k]
        if mask is not None:
            img = od.q_sample(sched, x0, t, q_noises[k]) * mask + (1. - mask) * img
        if i % log_every_t == 0 or i == T - 1:
            inter.append(img)
    if stats is not None:
        stats["clamped"] = clamped
    return img, inter


def ddpm_update_ref(x, eps, row, clip, z, mask=None, x0=None, zb=None, ca=None, cn=None):
    """stedm_ddpm_step's formula in fp32 torch, in place on x. row: {sr, srm1, c1, c2, sigma}; blend with (ca, cn) = the fp32
    sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod at t."""
    sr, srm1, c1, c2, sig = [torch.tensor(float(v), dtype=torch.float32) for v in row]
    q = sr * x - srm1 * eps
    if clip:
        q = q.clamp(-1., 1.)
    o = (c1 * q + c2 * x) + sig * z
    if mask is not None:
        o = (ca * x0 + cn * zb) * mask + (1. - mask) * o
    x.copy_(o)
    return x


def _ref(c, bufs, **kw):
    return ref_ddpm_sample(toy_eps, c["xT"], c["T"], bufs, c["clip"], c["cond"], c["noises"], c["mask"], c["x0"], c["q_noises"], **kw)


# ------------------------------------------------------------------------------------------------ schedule
def test_posterior_buffers_equal_f20_bitwise(golden):
    from stedm_amd.schedule import POSTERIOR_BUFFERS, PosteriorSchedule
    assert tuple(POSTERIOR_BUFFERS) == BUFFERS
    ps = PosteriorSchedule.make(1000, 0.0015, 0.0205)
    for b, want in f20_buffers(golden).items():
        got = getattr(ps, b)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32)), b
    ld = _cpu_ld()
    for b, want in f20_buffers(golden).items():
        assert torch.equal(getattr(ld, b), want), b


def test_step_table_rows(golden):
    from stedm_amd.schedule import ddpm_step_table
    bufs = f20_buffers(golden)
    tab = torch.from_numpy(ddpm_step_table(bufs["sqrt_recip_alphas_cumprod"], bufs["sqrt_recipm1_alphas_cumprod"],
                                           bufs["posterior_mean_coef1"], bufs["posterior_mean_coef2"], bufs["posterior_log_variance_clipped"]))
    assert tab.shape == (1000, 5) and tab.dtype == torch.float32
    assert tab[0, 4] == 0 and bool((tab[1:, 4] > 0).all())
    for t in (1, 2, 500, 999):       # the reference's expression on a [B, 1, 1, 1] tensor
        lv = bufs["posterior_log_variance_clipped"][t].reshape(1, 1, 1, 1).expand(2, 1, 1, 1).contiguous()
        assert torch.equal(tab[t, 4].expand(2, 1, 1, 1), (1 - torch.zeros(2, 1, 1, 1)) * (0.5 * lv).exp()), t


# ------------------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize("name", CASES)
def test_restated_loop_reproduces_f20(golden, name):
    c = f20_case(golden, name)
    stats = {}
    out, inter = _ref(c, f20_buffers(golden), stats=stats)
    assert rel_max(out, c["out"]) <= F20_TOL, rel_max(out, c["out"])
    assert len(inter) == c["n_inter"]
    if name == "full":
        assert len(inter) == 12
        for a, b in zip(inter, c["inter"]):
            assert rel_max(a, b) <= F20_TOL
    if c["clip"]:
        assert stats["clamped"] > 0 and abs(stats["clamped"] - c["clamped"]) <= max(4, c["clamped"] // 10000)
    if name == "full":
        assert c["clamped"] > 1000             # the clamp fires: x0 leaves [-1, 1] at high t


@pytest.mark.parametrize("name", CASES)
def test_table_and_kernel_formula_reproduce_the_loop(golden, name):
    from stedm_amd.schedule import ddpm_step_table
    c = f20_case(golden, name)
    bufs = f20_buffers(golden)
    tab = ddpm_step_table(bufs["sqrt_recip_alphas_cumprod"], bufs["sqrt_recipm1_alphas_cumprod"], bufs["posterior_mean_coef1"],
                          bufs["posterior_mean_coef2"], bufs["posterior_log_variance_clipped"])
    sched = od.Schedule()
    x = c["xT"].clone()
    for k, i in enumerate(range(c["T"] - 1, -1, -1)):
        t = torch.full((2,), i, dtype=torch.long)
        kw = {}
        if c["mask"] is not None:
            kw = dict(mask=c["mask"], x0=c["x0"], zb=c["q_noises"][k], ca=sched.sqrt_alphas_cumprod[i], cn=sched.sqrt_one_minus_alphas_cumprod[i])
        ddpm_update_ref(x, toy_eps(x, t, c["cond"]), tab[i], c["clip"], c["noises"][k], **kw)
    want, _ = _ref(c, bufs)
    assert torch.equal(x, want)
    assert rel_max(x, c["out"]) <= F20_TOL


class _CpuToy:
    """F20's model on the CPU with the surface AncestralSampler reads; records every call's t."""

    def __init__(self, log_every_t=100, clip=True):
        from stedm_amd.schedule import PosteriorSchedule
        s = od.Schedule()
        ps = PosteriorSchedule.make(1000, 0.0015, 0.0205)
        for b in BUFFERS:
            setattr(self, b, torch.from_numpy(getattr(ps, b)))
        self.sqrt_alphas_cumprod = s.sqrt_alphas_cumprod
        self.sqrt_one_minus_alphas_cumprod = s.sqrt_one_minus_alphas_cumprod
        self.num_timesteps = 1000
        self.clip_denoised = clip
        self.log_every_t = log_every_t
        self.channels, self.image_size = 4, 8
        self.device = torch.device("cpu")
        self.ts = []

    def apply_model(self, x, t, c):
        self.ts.append(t.clone())
        return toy_eps(x, t, c)


@pytest.fixture
def cpu_kernels(monkeypatch):
    """The plain step on the CPU - ops.ddpm_step_ex as the loop calls it, in place (x_out = x) and with no option set: ddpm_update_ref at
    row step_idx[0] with the given noises. Returns the list of t of every update."""
    from stedm_amd import ops
    seen = []

    def step(x, eps, table, step_idx=None, clip_denoised=True, noise=None, seed=0, first_id=0, mask=None, x0=None, mask_noise=None,
             mask_seed=0, sqrt_ac=None, sqrt_1mac=None, x_out=None):
        t = int(step_idx[0])
        seen.append(t)
        assert x_out is x and noise is not None and (mask is None or mask_noise is not None)
        kw = {} if mask is None else dict(mask=mask, x0=x0, zb=mask_noise, ca=sqrt_ac[t], cn=sqrt_1mac[t])
        return ddpm_update_ref(x, eps, table[t], clip_denoised, noise, **kw)

    monkeypatch.setattr(ops, "ddpm_step_ex", step)
    return seen


@pytest.mark.parametrize("name", CASES)
def test_sampler_loop_reproduces_the_reference_loop_and_logs_by_its_rule(golden, cpu_kernels, name):
    from stedm_amd.ancestral import AncestralSampler
    c = f20_case(golden, name)
    toy = _CpuToy(clip=c["clip"])
    kw = {} if c["mask"] is None else dict(mask=c["mask"], x0=c["x0"], mask_noises=c["q_noises"])
    timesteps = None if name == "full" else c["T"]
    x, inter = AncestralSampler(toy).sample(c["cond"], 2, return_intermediates=True, x_T=c["xT"], timesteps=timesteps,
                                            noises=c["noises"], log_every_t=5, ddim_steps=50, verbose=True, **kw)
    assert cpu_kernels == list(range(c["T"] - 1, -1, -1))
    assert [int(t[0]) for t in toy.ts] == cpu_kernels and all(bool((t == t[0]).all()) for t in toy.ts)
    want_x, want = _ref(c, toy_buffers(toy))
    assert torch.equal(x, want_x)
    # a list, x_T first, then by the MODEL's log_every_t (100): sample() swallows the log_every_t keyword as the reference does
    assert isinstance(inter, list) and len(inter) == len(want) == c["n_inter"]
    assert torch.equal(inter[0], c["xT"]) and all(torch.equal(a, b) for a, b in zip(inter, want))
    assert rel_max(x, c["out"]) <= F20_TOL
    if name == "full":
        assert all(rel_max(a, b) <= F20_TOL for a, b in zip(inter, c["inter"]))


def toy_buffers(toy):
    return {b: getattr(toy, b) for b in BUFFERS}


def test_p_sample_loop_honours_log_every_t_and_start_T(golden, cpu_kernels):
    from stedm_amd.ancestral import AncestralSampler
    c = f20_case(golden, "short")
    toy = _CpuToy(clip=False)
    seen = []
    x, inter = AncestralSampler(toy).p_sample_loop(c["cond"], SHAPE, return_intermediates=True, x_T=c["xT"], timesteps=1000, start_T=20,
                                                   noises=c["noises"], log_every_t=5, callback=seen.append)
    assert seen == list(range(19, -1, -1))
    want_x, want = _ref(c, toy_buffers(toy), log_every_t=5)
    assert torch.equal(x, want_x) and len(inter) == len(want) == 6          # x_T, t = 19, 15, 10, 5, 0
    assert all(torch.equal(a, b) for a, b in zip(inter, want))
    assert torch.equal(AncestralSampler(toy).p_sample_loop(c["cond"], SHAPE, x_T=c["xT"], timesteps=20, noises=c["noises"]), want_x)


def test_masked_blend_runs_after_the_step(golden, cpu_kernels):
    """The t = 0 step blends too: a mask of ones returns q_sample(x0, 0) with the last blend noise, not the step's result."""
    from stedm_amd.ancestral import AncestralSampler
    c = f20_case(golden, "masked")
    toy = _CpuToy()
    ones = torch.ones(1, 1, 8, 8)
    x = AncestralSampler(toy).p_sample_loop(c["cond"], SHAPE, x_T=c["xT"], timesteps=3, noises=c["noises"][:3], mask=ones, x0=c["x0"],
                                            mask_noises=c["q_noises"][:3])
    s = od.Schedule()
    want = s.sqrt_alphas_cumprod[0] * c["x0"] + s.sqrt_one_minus_alphas_cumprod[0] * c["q_noises"][2]
    assert torch.equal(x, want)


def _cpu_ld(**kw):
    from stedm_amd.latent_diffusion import LatentDiffusion
    return LatentDiffusion(torch.nn.Conv2d(4, 4, 1), linear_start=0.0015, linear_end=0.0205, image_size=8, channels=4,
                           conditioning_key="hybrid", loss_type="l1", **kw)


def test_sample_log_ddim_false_runs_the_chain(golden, cpu_kernels):
    c = f20_case(golden, "short")
    ld = _cpu_ld(log_every_t=100, clip_denoised=False)
    calls = []

    def apply_model(x, t, cond, out=None, uniform_t=False):
        calls.append(int(t[0]))
        return toy_eps(x, t, cond["c_crossattn"][0])

    ld.apply_model = apply_model
    cond = {"c_concat": [torch.zeros(3, 1, 8, 8)], "c_crossattn": [torch.cat([c["cond"], c["cond"][:1]])]}   # sliced to batch_size
    x, inter = ld.sample_log(cond, 2, False, 50, x_T=c["xT"], timesteps=20, noises=c["noises"], log_every_t=5, eta=0.)
    want_x, want = _ref(c, f20_buffers(golden))
    assert calls == list(range(19, -1, -1))
    assert torch.equal(x, want_x) and isinstance(inter, list) and len(inter) == 3
    x2, _ = ld.sample_log(cond, 2, True, 50, sampler="ddpm", x_T=c["xT"], timesteps=20, noises=c["noises"])
    assert torch.equal(x2, x)
    with pytest.raises(ValueError):
        ld.sample_log(cond, 2, False, 50, sampler="plms", x_T=c["xT"], timesteps=20, noises=c["noises"])


# ------------------------------------------------------------------------------------------------ refusals, state dict, names
class _NoDeviceModel:
    """A model whose every use fails the test: the checks must come first."""
    num_timesteps = 1000
    log_every_t = 100
    clip_denoised = True
    channels, image_size = 4, 8

    @property
    def device(self):
        raise AssertionError("device work before the argument checks")

    @property
    def sqrt_recip_alphas_cumprod(self):
        raise AssertionError("schedule work before the argument checks")

    def apply_model(self, *a, **k):
        raise AssertionError("model call before the argument checks")


@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(temperature=0.9), dict(noise_dropout=0.1), dict(score_corrector=object()),
                                dict(quantize_denoised=True),
                                dict(unconditional_guidance_scale=1.5, unconditional_conditioning=torch.zeros(2, 4, 8, 8))])
def test_refusals_raise_before_device_work(kw):
    from stedm_amd.ancestral import AncestralSampler
    s = AncestralSampler(_NoDeviceModel())
    with pytest.raises(NotImplementedError):
        s.sample(torch.zeros(2, 4, 8, 8), 2, x_T=torch.zeros(2, 4, 8, 8), **kw)


def test_ignored_and_invalid_options():
    from stedm_amd.ancestral import AncestralSampler
    s = AncestralSampler(_NoDeviceModel())
    with pytest.raises(ValueError):
        s.p_sample_loop(None, SHAPE, timesteps=1001)
    with pytest.raises(ValueError):
        s.p_sample_loop(None, SHAPE, timesteps=4, noises=[torch.zeros(SHAPE)] * 3)
    with pytest.raises(NotImplementedError):
        _cpu_ld(v_posterior=0.1)


def test_predict_latents_ddpm_refusals():
    from stedm_amd.latent_diffusion import predict_latents
    with pytest.raises(NotImplementedError):
        predict_latents(None, {}, 50, cfg_scale=1.5, style_sampling="mp", sampler="ddpm")
    with pytest.raises(NotImplementedError):
        predict_latents(None, {}, 50, eta=0.5, sampler="ddpm")


def test_state_dict_keys_unchanged():
    ld = _cpu_ld()
    keys = set(ld.state_dict())
    assert keys == {"betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "logvar",
                    "model.diffusion_model.weight", "model.diffusion_model.bias"}
    assert set(ld.reference_state_dict()) == {"_model." + k for k in keys}
    assert ld.clip_denoised is True and ld.v_posterior == 0.
    sd = dict(ld.reference_state_dict())
    missing, unexpected = _cpu_ld().load_reference_state_dict(sd)
    assert missing == [] and unexpected == []
    sd.update({"_model." + b: torch.zeros(1000) for b in BUFFERS})      # the reference's checkpoints carry them: unexpected, as before
    missing, unexpected = _cpu_ld().load_reference_state_dict(sd)
    assert missing == [] and sorted(unexpected) == sorted(BUFFERS)


def test_ddpm_is_a_known_sampler_and_the_default_stays_ddim():
    import inspect
    from stedm_amd import latent_diffusion as ld
    assert "ddpm" in ld.ALL_SAMPLERS and ld.ANCESTRAL == "ddpm"
    assert ld.SAMPLERS == ("ddim", "dpm_solver", "plms")          # the samplers driven by ddim_steps
    for fn in (ld.LatentDiffusion.sample_log, ld.predict_latents):
        assert inspect.signature(fn).parameters["sampler"].default == "ddim"
