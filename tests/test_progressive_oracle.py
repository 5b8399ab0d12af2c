"""CPU tier: `progressive_denoising`, `p_sample`, `p_mean_variance` and quantize_denoised on the ancestral sampler
(stedm_amd/ancestral.py, LatentDiffusion) against fixture F25, the reference's own functions with a closed-form eps model and recorded draws
(tests/golden/make_golden_progressive.py).
  * `ref_progressive`, a test-local fp32 restatement of progressive_denoising over F20's buffers, fed the recorded noises and keep masks,
    reproduces F25 within F20_TOL, with equal codebook indices at every step of the quantised cases;
  * AncestralSampler.progressive_denoising and LatentDiffusion.p_sample / p_mean_variance run on the CPU with ops.ddpm_step_ex replaced by
    `ddpm_step_ex_ref`, stedm_ddpm_step_ex's formula in torch behind the same interface (keep bits: the numpy restatement of the kernel's
    rule, tests.test_ddim_options_oracle.keep_mask with t for the iteration), and reproduce the restated loop bit for bit; they log the x0
    predictions by the reference's rule, blend after the step, index the temperature list by t and accept an int temperature;
  * p_sample_loop(quantize_denoised=True) equals the restated loop with the quantiser inserted;
  * the refusals raise before any device work; the state dict keeps its keys; header, ctypes table and ABI number agree.
Bit-for-bit comparisons are made only between loops computed in this process; against the stored fixture within F20_TOL (the reason is in
make_golden_ddpm.py). The GPU tier (tests/test_gpu_progressive.py) runs the kernel and the HIP loops against these restatements."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import ddim as od
from oracle import vq as ovq
from stedm_amd.utils import prng
from tests.test_ddim_options_oracle import drop_scale, keep_mask
from tests.test_ddpm_oracle import BUFFERS, F20_TOL, _CpuToy, _cpu_ld, f20_buffers, rel_max, toy_buffers, toy_eps

torch.set_grad_enabled(False)

SEED, SHAPE = 25, (2, 4, 8, 8)
N = SHAPE[1] * SHAPE[2] * SHAPE[3]
LOOPS = {"a": dict(noise_dropout=0.2, quantize=True, clip=True, log_every_t=5, ramp=True),
         "b": dict(temperature=0.7, clip=False, log_every_t=4, batch_form=True),
         "c": dict(quantize=True, clip=True, log_every_t=5, masked=True)}


def f25_case(golden, name):
    """F25 case `name`: the stored results and the draws rebuilt from their recipes (CPU tensors)."""
    f = golden("f25_progressive")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    o = LOOPS[name]
    T = int(f[f"{name}_T"])
    p = o.get("noise_dropout", 0.0)
    c = dict(o, xT=g("xT"), cond=g("cond"), T=T, p=p, out=g(f"{name}_out"), inter=g(f"{name}_inter"), clamped=int(f[f"{name}_clamped"]),
             dropout_calls=int(f[f"{name}_dropout_calls"]), noises=[prng.normal(SEED, f"prog.{name}.n{k}", SHAPE) for k in range(T)],
             temps=[float(v) for v in f["ramp"]] if o.get("ramp") else o.get("temperature", 1.0),
             codebook=g("codebook") if o.get("quantize") else None, mask=None, x0=None, q_noises=None, keeps=None)
    if p > 0:        # F.dropout's multiplier with the recorded mask
        c["keeps"] = [(prng.uniform(SEED, f"prog.{name}.d{k}", SHAPE, lo=0.0, hi=1.0) >= p).float().div_(1 - p) for k in range(T)]
    if o.get("masked"):
        c.update(mask=g("mask"), x0=g("x0"), q_noises=[prng.normal(SEED, f"prog.{name}.q{k}", SHAPE) for k in range(T)])
    if o.get("quantize"):
        c["idx"] = np.asarray(f[f"{name}_idx"]).astype(np.int64)
    return c


def kernel_keeps(seed, ids, T, p, shape=SHAPE):
    """The multiplier the kernel applies at step k (t = T - 1 - k): its keep bits times (float)(1 / (1 - p))."""
    n = int(np.prod(shape[1:]))
    return [torch.from_numpy(keep_mask(seed, ids, n, T - 1 - k, p).reshape(shape)).float() * drop_scale(p) for k in range(T)]


# ------------------------------------------------------------------------------------------------ test-local restatements
def ref_p_step(eps, img, t, bufs, clip, z, temperature, keep, codebook, stats=None):
    """p_sample with return_x0 (ddpm.py:1050-1110) from the model output: temperature [B] or a number, keep the dropout's multiplier or
    None. Returns (x_prev, x0, mean, indices or None)."""
    b = img.shape[0]
    ex = lambda a: a[t].reshape(b, 1, 1, 1)
    x_recon = ex(bufs["sqrt_recip_alphas_cumprod"]) * img - ex(bufs["sqrt_recipm1_alphas_cumprod"]) * eps
    if clip:
        if stats is not None:
            stats["clamped"] = stats.get("clamped", 0) + int((x_recon.abs() > 1).sum())
        x_recon = x_recon.clamp(-1., 1.)
    idx = None
    if codebook is not None:
        if stats is not None:            # the tie margin: winner / runner-up gap of the squared distances (f64 from the fp32 operands)
            d = torch.cdist(x_recon.permute(0, 2, 3, 1).reshape(-1, x_recon.shape[1]).double(), codebook.double()) ** 2
            two = torch.topk(d, 2, dim=1, largest=False).values
            stats["gap"] = min(stats.get("gap", float("inf")), float((two[:, 1] - two[:, 0]).min()))
        idx, x_recon = ovq.quantize(codebook, x_recon)
    mean = ex(bufs["posterior_mean_coef1"]) * x_recon + ex(bufs["posterior_mean_coef2"]) * img
    noise = z * temperature
    if keep is not None:
        noise = noise * keep
    nonzero_mask = (1 - (t == 0).float()).reshape(b, 1, 1, 1)
    return mean + nonzero_mask * (0.5 * ex(bufs["posterior_log_variance_clipped"])).exp() * noise, x_recon, mean, idx


def ref_progressive(eps_fn, x_T, T, bufs, clip, cond, noises, temps=1.0, keeps=None, codebook=None, mask=None, x0=None, q_noises=None,
                    log_every_t=100, stats=None):
    """progressive_denoising (ddpm.py:1112-1166) on `eps_fn(x, t, c)` in fp32 torch from the fp32 buffers `bufs`. noises[k] / keeps[k] /
    q_noises[k]: the draws of step k (t = T - 1 - k); temps: a number or a list indexed by t. Returns (img, the x0 log, indices per step)."""
    sched = od.Schedule()
    img = x_T.clone().float()
    b = img.shape[0]
    if not isinstance(temps, (list, tuple)):
        temps = [temps] * T
    inter, idxs = [], []
    for k, i in enumerate(range(T - 1, -1, -1)):
        t = torch.full((b,), i, dtype=torch.long)
        img, x0p, _, idx = ref_p_step(eps_fn(img, t, cond), img, t, bufs, clip, noises[k], temps[i], None if keeps is None else keeps[k],
                                      codebook, stats)
        idxs.append(idx)
        if mask is not None:
            img = od.q_sample(sched, x0, t, q_noises[k]) * mask + (1. - mask) * img
        if i % log_every_t == 0 or i == T - 1:
            inter.append(x0p)
    return img, inter, idxs


def ddpm_step_ex_ref(x, eps, table, step_idx=None, t=None, clip_denoised=True, noise=None, temperature=None, noise_dropout=0.0,
                     codebook=None, seed=0, first_id=0, mask=None, x0=None, mask_noise=None, mask_seed=0, sqrt_ac=None, sqrt_1mac=None,
                     x_out=None, x0_out=None, mean_out=None, idx_out=None):
    """stedm_ddpm_step_ex's formula in fp32 torch behind ops.ddpm_step_ex's interface (the noises must be given: the in-kernel draws are
    the GPU tier's). Every product and sum is a torch op of its own, i.e. rounded on its own."""
    assert (step_idx is None) != (t is None) and noise is not None or x_out is None
    B = x.shape[0]
    tt = torch.full((B,), int(step_idx[0]), dtype=torch.long) if t is None else t.long()
    col = lambda j: table[tt, j].reshape(B, 1, 1, 1)
    q = col(0) * x - col(1) * eps
    if clip_denoised:
        q = q.clamp(-1., 1.)
    if codebook is not None:
        assert x0_out is not None
        idx, q = ovq.quantize(codebook, q)
        if idx_out is not None:
            idx_out.copy_(idx.reshape(idx_out.shape))
    mean = col(2) * q + col(3) * x
    if x0_out is not None:
        x0_out.copy_(q)
    if mean_out is not None:
        mean_out.copy_(mean)
    if x_out is None:
        return None
    n = noise * (1.0 if temperature is None else temperature[tt].reshape(B, 1, 1, 1))
    if noise_dropout > 0:
        keep = np.stack([keep_mask(seed, [first_id + b], x[0].numel(), int(tt[b]), noise_dropout)[0] for b in range(B)])
        n = n * (torch.from_numpy(keep.reshape(x.shape)).float() * drop_scale(noise_dropout))
    o = mean + col(4) * n
    if mask is not None:
        assert mask_noise is not None
        ca, cn = sqrt_ac[tt].reshape(B, 1, 1, 1), sqrt_1mac[tt].reshape(B, 1, 1, 1)
        o = (ca * x0 + cn * mask_noise) * mask + (1. - mask) * o
    x_out.copy_(o)
    return x_out


@pytest.fixture
def cpu_kernels(monkeypatch):
    """ops.ddpm_step_ex on the CPU (ddpm_step_ex_ref); ops.ddpm_step must not be reached by a call with options. Returns the calls' t."""
    from stedm_amd import ops
    seen = []

    def step_ex(x, eps, table, step_idx=None, t=None, **kw):
        seen.append(int(step_idx[0]) if t is None else [int(v) for v in t])
        return ddpm_step_ex_ref(x, eps, table, step_idx=step_idx, t=t, **kw)

    def plain(*a, **k):
        raise AssertionError("a call with options took stedm_ddpm_step")

    monkeypatch.setattr(ops, "ddpm_step_ex", step_ex)
    monkeypatch.setattr(ops, "ddpm_step", plain)
    return seen


class _VqStage:
    """first_stage_model.quantize.embedding.weight, all that quantize_denoised reads"""

    def __init__(self, codebook):
        self.quantize = type("Q", (), {})()
        self.quantize.embedding = type("E", (), {})()
        self.quantize.embedding.weight = codebook


def _toy(c, **kw):
    toy = _CpuToy(clip=c["clip"], **kw)
    if c.get("codebook") is not None:
        toy.first_stage_model = _VqStage(c["codebook"])
    return toy


def _ref(c, bufs, keeps="recorded", **kw):
    return ref_progressive(toy_eps, c["xT"], c["T"], bufs, c["clip"], c["cond"], c["noises"], c["temps"],
                           c["keeps"] if isinstance(keeps, str) else keeps, c["codebook"], c["mask"], c["x0"], c["q_noises"],
                           c["log_every_t"], **kw)


# ------------------------------------------------------------------------------------------------ F25
@pytest.mark.parametrize("name", list(LOOPS))
def test_restated_loop_reproduces_f25(golden, name):
    from stedm_amd.ancestral import AncestralSampler
    assert hasattr(AncestralSampler, "progressive_denoising")
    c = f25_case(golden, name)
    stats = {}
    out, inter, idxs = _ref(c, f20_buffers(golden), stats=stats)
    assert rel_max(out, c["out"]) <= F20_TOL, rel_max(out, c["out"])
    want_t = [t for t in range(c["T"] - 1, -1, -1) if t % c["log_every_t"] == 0 or t == c["T"] - 1]
    assert len(inter) == len(want_t) == c["inter"].shape[0] == {"a": 5, "b": 4, "c": 4}[name]
    for a, b in zip(inter, c["inter"]):
        assert rel_max(a, b) <= F20_TOL
    assert c["dropout_calls"] == (c["T"] if c["p"] > 0 else 0)
    if c["clip"]:
        assert c["clamped"] > 100 and abs(stats["clamped"] - c["clamped"]) <= 4         # the clamp fires
    if c["codebook"] is not None:
        assert float(golden("f25_progressive")[f"{name}_gap"]) >= 1e-4                  # the tie margin the generator asserted
        for k in range(c["T"]):
            assert np.array_equal(idxs[k].reshape(-1).numpy(), c["idx"][k]), k
        px = inter[-1].permute(0, 2, 3, 1).reshape(-1, 4).double()
        assert float(torch.cdist(px, c["codebook"].double()).min(dim=1).values.max()) < 1e-6      # codebook rows, up to the straight-through rounding


def test_restated_single_steps_reproduce_f25_d(golden):
    from stedm_amd import ops
    assert hasattr(ops, "ddpm_step_ex")
    f = golden("f25_progressive")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    bufs = f20_buffers(golden)
    x, t, cond = g("d_x"), g("d_t"), g("cond")
    assert t.tolist() == [7, 0]
    z = prng.normal(SEED, "prog.d.n0", SHAPE)
    xs, x0s, _, idx = ref_p_step(toy_eps(x, t, cond), x, t, bufs, True, z, 0.8, None, g("codebook"))
    assert rel_max(xs, g("d_sample")) <= F20_TOL and rel_max(x0s, g("d_sample_x0")) <= F20_TOL
    assert np.array_equal(idx.reshape(-1).numpy(), np.asarray(f["d_idx"])[0].astype(np.int64)) and float(f["d_gap"]) >= 1e-4
    _, xr, mean, _ = ref_p_step(toy_eps(x, t, cond), x, t, bufs, True, z, 1.0, None, None)
    assert rel_max(mean, g("d_mean")) <= F20_TOL and rel_max(xr, g("d_x_recon")) <= F20_TOL
    assert torch.equal(g("d_var").reshape(2), bufs["posterior_variance"][t])
    assert torch.equal(g("d_logvar").reshape(2), bufs["posterior_log_variance_clipped"][t])


# ------------------------------------------------------------------------------------------------ the sampler on the CPU stand-in
NOISE_SEED = 0x5EED25


@pytest.mark.parametrize("name", list(LOOPS))
def test_sampler_progressive_reproduces_the_restated_loop(golden, cpu_kernels, name):
    from stedm_amd.ancestral import AncestralSampler
    c = f25_case(golden, name)
    toy = _toy(c)
    T = c["T"]
    kw = dict(mask=c["mask"], x0=c["x0"], mask_noises=c["q_noises"]) if c["mask"] is not None else {}
    cond = torch.cat([c["cond"], c["cond"][:1]])                                           # sliced to batch_size
    shape_kw = dict(shape=SHAPE[1:], batch_size=2) if c.get("batch_form") else dict(shape=SHAPE)
    seen_cb, seen_img = [], []
    x, inter = AncestralSampler(toy).progressive_denoising(cond, quantize_denoised=c["codebook"] is not None, temperature=c["temps"],
                                                           noise_dropout=c["p"], x_T=c["xT"], start_T=T, log_every_t=c["log_every_t"],
                                                           noises=c["noises"], noise_seed=NOISE_SEED, sample_id0=3, verbose=False,
                                                           callback=seen_cb.append, img_callback=lambda im, i: seen_img.append(i),
                                                           **shape_kw, **kw)
    assert cpu_kernels == seen_cb == seen_img == list(range(T - 1, -1, -1))
    assert [int(t[0]) for t in toy.ts] == cpu_kernels and all(t.shape == (2,) and bool((t == t[0]).all()) for t in toy.ts)
    keeps = kernel_keeps(NOISE_SEED, [3, 4], T, c["p"]) if c["p"] > 0 else None
    want_x, want, _ = _ref(c, toy_buffers(toy), keeps=keeps)
    assert torch.equal(x, want_x)
    assert isinstance(inter, list) and len(inter) == len(want) == c["inter"].shape[0]      # x0 predictions, no x_T
    assert all(torch.equal(a, b) for a, b in zip(inter, want))
    if c["p"] == 0:                                                                        # nothing but the recorded draws: the fixture itself
        assert rel_max(x, c["out"]) <= F20_TOL
        assert all(rel_max(a, b) <= F20_TOL for a, b in zip(inter, c["inter"]))


def test_temperature_list_is_indexed_by_t_and_an_int_is_accepted(golden, cpu_kernels):
    from stedm_amd.ancestral import AncestralSampler
    c = f25_case(golden, "b")
    toy = _toy(c)
    run = lambda temp, T=12: AncestralSampler(toy).progressive_denoising(c["cond"], SHAPE, temperature=temp, x_T=c["xT"], start_T=T,
                                                                         noises=c["noises"][:T], log_every_t=4)
    ramp = [0.25 + 0.05 * i for i in range(14)]                        # longer than timesteps: entries 12, 13 are never read
    x, inter = run(ramp)
    want_x, want, _ = ref_progressive(toy_eps, c["xT"], 12, toy_buffers(toy), False, c["cond"], c["noises"], ramp, log_every_t=4)
    assert torch.equal(x, want_x) and all(torch.equal(a, b) for a, b in zip(inter, want))
    rev, _, _ = ref_progressive(toy_eps, c["xT"], 12, toy_buffers(toy), False, c["cond"], c["noises"], ramp[:12][::-1], log_every_t=4)
    assert not torch.equal(x, rev)                                     # indexing by the step count would give this
    xi, _ = run(1)                                                     # the reference dies on an int ('int' object is not subscriptable)
    xf, _ = run(1.0)
    assert torch.equal(xi, xf)
    x2, _ = run(2)
    want2, _, _ = ref_progressive(toy_eps, c["xT"], 12, toy_buffers(toy), False, c["cond"], c["noises"], 2.0, log_every_t=4)
    assert torch.equal(x2, want2)
    with pytest.raises(ValueError):
        run(ramp[:11])


def test_progressive_blends_after_the_step(golden, cpu_kernels):
    """The t = 0 step blends too: a mask of ones returns q_sample(x0, 0) with the last blend noise; the logged x0 is the prediction."""
    from stedm_amd.ancestral import AncestralSampler
    c = f25_case(golden, "c")
    toy = _toy(c)
    ones = torch.ones(1, 1, 8, 8)
    x, inter = AncestralSampler(toy).progressive_denoising(c["cond"], SHAPE, x_T=c["xT"], start_T=3, noises=c["noises"][:3], mask=ones,
                                                           x0=c["x0"], mask_noises=c["q_noises"][:3], log_every_t=1)
    s = od.Schedule()
    assert torch.equal(x, s.sqrt_alphas_cumprod[0] * c["x0"] + s.sqrt_one_minus_alphas_cumprod[0] * c["q_noises"][2])
    assert len(inter) == 3 and not torch.equal(inter[-1], x)


def test_p_sample_loop_quantize_denoised(golden, cpu_kernels):
    from stedm_amd.ancestral import AncestralSampler
    c = f25_case(golden, "a")
    toy = _toy(c)
    T = 12
    x, inter = AncestralSampler(toy).p_sample_loop(c["cond"], SHAPE, return_intermediates=True, x_T=c["xT"], timesteps=T,
                                                   quantize_denoised=True, noises=c["noises"][:T], log_every_t=5)
    bufs = toy_buffers(toy)
    img, want = c["xT"].clone(), [c["xT"]]
    for k, i in enumerate(range(T - 1, -1, -1)):
        t = torch.full((2,), i, dtype=torch.long)
        img, x0p, _, _ = ref_p_step(toy_eps(img, t, c["cond"]), img, t, bufs, True, c["noises"][k], 1.0, None, c["codebook"])
        if i % 5 == 0 or i == T - 1:
            want.append(img)
    assert cpu_kernels == list(range(T - 1, -1, -1))
    assert torch.equal(x, img) and len(inter) == len(want) == 5 and all(torch.equal(a, b) for a, b in zip(inter, want))
    xs = AncestralSampler(toy).sample(c["cond"], 2, x_T=c["xT"], timesteps=T, quantize_denoised=True, noises=c["noises"][:T])
    assert torch.equal(xs, x)


def _ld(codebook=None, clip=True):
    ld = _cpu_ld(clip_denoised=clip)
    ld.apply_model = lambda x, t, cond, **kw: toy_eps(x, t, cond)
    if codebook is not None:
        ld.first_stage_model = _VqStage(codebook)
    return ld


def test_latent_diffusion_single_steps(golden, cpu_kernels):
    f = golden("f25_progressive")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    x, t, cond, cb = g("d_x"), g("d_t"), g("cond"), g("codebook")
    z = prng.normal(SEED, "prog.d.n0", SHAPE)
    ld = _ld(cb)
    keys = set(ld.state_dict())
    bufs = {b: getattr(ld, b) for b in BUFFERS}
    x_in = x.clone()
    xs, x0s = ld.p_sample(x_in, cond, t, clip_denoised=True, quantize_denoised=True, return_x0=True, temperature=0.8, _noise=z)
    assert cpu_kernels[-1] == [7, 0] and torch.equal(x_in, x)                              # per-sample rows; x is left alone
    wx, wx0, _, _ = ref_p_step(toy_eps(x, t, cond), x, t, bufs, True, z, 0.8, None, cb)
    assert torch.equal(xs, wx) and torch.equal(x0s, wx0)
    assert rel_max(xs, g("d_sample")) <= F20_TOL and rel_max(x0s, g("d_sample_x0")) <= F20_TOL
    only = ld.p_sample(x, cond, t, clip_denoised=True, quantize_denoised=True, temperature=0.8, _noise=z)
    assert torch.equal(only, xs)
    # noise dropout: the kernel's keep rule keyed by (noise_seed, sample_id0 + b, t[b])
    xd = ld.p_sample(x, cond, t, clip_denoised=True, temperature=0.8, noise_dropout=0.25, _noise=z, noise_seed=77, sample_id0=5)
    keep = np.stack([keep_mask(77, [5 + b], N, int(t[b]), 0.25)[0] for b in range(2)]).reshape(SHAPE)
    wd, _, _, _ = ref_p_step(toy_eps(x, t, cond), x, t, bufs, True, z, 0.8, torch.from_numpy(keep).float() * drop_scale(0.25), None)
    assert torch.equal(xd, wd)
    out = ld.p_mean_variance(x, cond, t, clip_denoised=True, return_x0=True)
    assert len(out) == 4 and len(ld.p_mean_variance(x, cond, t, clip_denoised=True)) == 3
    _, wxr, wmean, _ = ref_p_step(toy_eps(x, t, cond), x, t, bufs, True, z, 1.0, None, None)
    assert torch.equal(out[0], wmean) and torch.equal(out[3], wxr) and torch.equal(x_in, x)
    assert out[1].shape == out[2].shape == (2, 1, 1, 1)
    assert torch.equal(out[1], g("d_var")) and torch.equal(out[2], g("d_logvar"))
    assert rel_max(out[0], g("d_mean")) <= F20_TOL and rel_max(out[3], g("d_x_recon")) <= F20_TOL
    # q_posterior / predict_start_from_noise / q_mean_variance: the reference's expressions
    ex = lambda a: a[t].reshape(2, 1, 1, 1)
    pm, pv, plv = ld.q_posterior(x_start=g("x0"), x_t=x, t=t)
    assert torch.equal(pm, ex(bufs["posterior_mean_coef1"]) * g("x0") + ex(bufs["posterior_mean_coef2"]) * x)
    assert torch.equal(pv, g("d_var")) and torch.equal(plv, g("d_logvar")) and rel_max(pm, g("d_qpost_mean")) <= F20_TOL
    assert torch.equal(ld.predict_start_from_noise(x, t, z),
                       ex(bufs["sqrt_recip_alphas_cumprod"]) * x - ex(bufs["sqrt_recipm1_alphas_cumprod"]) * z)
    qm, qv, qlv = ld.q_mean_variance(x, t)
    assert torch.equal(qm, ex(ld.sqrt_alphas_cumprod) * x) and torch.equal(qv, ex(1.0 - ld.alphas_cumprod))
    assert torch.equal(qlv, ex(ld.log_one_minus_alphas_cumprod))
    assert set(ld.state_dict()) == keys == set(_cpu_ld().state_dict())                     # no new buffers
    assert keys == {"betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "logvar",
                    "model.diffusion_model.weight", "model.diffusion_model.bias"}


def test_latent_diffusion_progressive_and_sample_log_quantized(golden, cpu_kernels):
    c = f25_case(golden, "a")
    ld = _ld(c["codebook"])
    cond = {"c_concat": [torch.zeros(2, 1, 8, 8)], "c_crossattn": [c["cond"]]}
    ld.apply_model = lambda x, t, cd, **kw: toy_eps(x, t, cd["c_crossattn"][0])
    x, inter = ld.progressive_denoising(cond, SHAPE, quantize_denoised=True, temperature=c["temps"], noise_dropout=c["p"], x_T=c["xT"],
                                        start_T=c["T"], log_every_t=5, noises=c["noises"], noise_seed=NOISE_SEED)
    want_x, want, _ = _ref(c, f20_buffers(golden), keeps=kernel_keeps(NOISE_SEED, [0, 1], c["T"], c["p"]))
    assert torch.equal(x, want_x) and len(inter) == 5 and all(torch.equal(a, b) for a, b in zip(inter, want))
    xs, li = ld.sample_log(cond, 2, False, 50, x_T=c["xT"], timesteps=8, quantize_denoised=True, noises=c["noises"][:8])
    assert isinstance(li, list) and tuple(xs.shape) == SHAPE


# ------------------------------------------------------------------------------------------------ refusals, ABI
class _NoDeviceModel:
    """A model whose every use fails the test: the checks must come first."""
    num_timesteps = 1000
    log_every_t = 100
    clip_denoised = True
    channels, image_size = 4, 8
    shorten_cond_schedule = False

    @property
    def device(self):
        raise AssertionError("device work before the argument checks")

    @property
    def sqrt_recip_alphas_cumprod(self):
        raise AssertionError("schedule work before the argument checks")

    def apply_model(self, *a, **k):
        raise AssertionError("model call before the argument checks")


class _NarrowCodebook(_NoDeviceModel):
    first_stage_model = _VqStage(torch.zeros(16, 3))


class _Shortened(_NoDeviceModel):
    shorten_cond_schedule = True


Z = torch.zeros(SHAPE)


@pytest.mark.parametrize("model,kw,err", [
    (_NoDeviceModel, dict(score_corrector=object()), NotImplementedError),
    (_Shortened, dict(), NotImplementedError),
    (_NoDeviceModel, dict(temperature=[1.0] * 19, start_T=20), ValueError),
    (_NoDeviceModel, dict(noise_dropout=1.0), ValueError),
    (_NoDeviceModel, dict(noise_dropout=-0.1), ValueError),
    (_NoDeviceModel, dict(quantize_denoised=True), NotImplementedError),
    (_NarrowCodebook, dict(quantize_denoised=True), ValueError)])
def test_progressive_refusals_raise_before_device_work(model, kw, err):
    from stedm_amd.ancestral import AncestralSampler
    with pytest.raises(err):
        AncestralSampler(model()).progressive_denoising(Z, SHAPE, x_T=Z, **kw)


@pytest.mark.parametrize("model,kw,err", [
    (_NoDeviceModel, dict(score_corrector=object()), NotImplementedError),
    (_NoDeviceModel, dict(repeat_noise=True), NotImplementedError),
    (_NoDeviceModel, dict(return_codebook_ids=True), NotImplementedError),
    (_NoDeviceModel, dict(noise_dropout=1.5), ValueError),
    (_NoDeviceModel, dict(quantize_denoised=True), NotImplementedError),
    (_NarrowCodebook, dict(quantize_denoised=True), ValueError)])
def test_single_step_refusals_raise_before_device_work(model, kw, err):
    from stedm_amd.ancestral import AncestralSampler
    s = AncestralSampler(model())
    t = torch.tensor([7, 0])
    with pytest.raises(err):
        s.p_sample(Z, Z, t, **kw)
    if "repeat_noise" not in kw and "noise_dropout" not in kw:
        with pytest.raises(err):
            s.p_mean_variance(Z, Z, t, True, **kw)
    if "quantize_denoised" in kw:
        with pytest.raises(err):
            s.p_sample_loop(Z, SHAPE, x_T=Z, **kw)
        with pytest.raises(err):
            s.sample(Z, 2, x_T=Z, **kw)


def test_sample_still_refuses_what_the_reference_drops():
    from stedm_amd.ancestral import AncestralSampler
    s = AncestralSampler(_NoDeviceModel())
    assert hasattr(s, "progressive_denoising")
    for kw in (dict(temperature=0.9), dict(noise_dropout=0.1), dict(eta=0.5), dict(score_corrector=object())):
        with pytest.raises(NotImplementedError):
            s.sample(Z, 2, x_T=Z, **kw)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stedm_amd", "ancestral.py")).read()
    assert "not built" not in src                                    # the stale refusal is gone


def test_header_binding_and_abi_agree():
    from stedm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "stedm_hip.h")).read()
    assert int(re.search(r"#define STEDM_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 21
    decl = re.search(r"int stedm_ddpm_step_ex\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["stedm_ddpm_step_ex"][1]) == 30
    assert len(_lib.SIGNATURES["stedm_ddpm_step"][1]) == 21          # the plain entry keeps its form
