"""CPU tier: PLMS sampling (stedm_amd/plms.py) against fixture F19, the reference's own PLMSSampler with a closed-form eps model
(tests/golden/make_golden_plms.py).
  * `ref_plms_sample`, a test-local fp32 restatement of plms.py:115-239 over the oracle's DDIM schedule and update, reproduces every
    call's t exactly and every call's x and the final x within F19_TOL — it is the yardstick the GPU tier runs over the oracle U-Net;
  * the product's DDIM table through `plms_update_ref` (stedm_plms_step's formula in torch, same ring and phases) reproduces that loop
    bit for bit, and F19 within F19_TOL;
  * PLMSSampler's own loop on the CPU, the kernel replaced by `plms_update_ref` behind the same interface, reproduces the restated loop
    bit for bit (calls, result, intermediates), uses the reference's order at every iteration, and logs by the reference's rule;
  * the refusals raise before any device work.
Bit-for-bit comparisons are made only between loops computed in the same process. Against the stored fixture the comparison is within
F19_TOL: the toy model's tanh and the loop's fp32 arithmetic round differently across CPUs and libm builds by an ulp or so, which the
20-step loop carries to ~2e-7 of the largest value (measured: shifting every model output by one ulp moves the results by <= 4e-7)."""
import numpy as np
import pytest
import torch

from oracle import ddim as od
from stedm_amd.utils import prng

torch.set_grad_enabled(False)

CASES = ("s20c", "s4", "s1", "m10")     # F19: S = 20 CFG 1.5, S = 4, S = 1, S = 10 CFG 1.5 masked
SEED, SHAPE = 19, (2, 4, 8, 8)
F19_TOL = 1e-5          # max |diff| / max |ref| against the stored fixture (see the module docstring)


def toy_eps(x, t, bias):
    """F19's closed-form eps model (the one of F10 / F17)."""
    tf = t.float()[:, None, None, None] / 1000.0
    return torch.tanh(x * (0.5 + tf) + bias) * (0.8 + 0.3 * tf) + 0.1 * bias


def q_noise(k):
    """The noise of the k-th q_sample call of F19's masked case (make_golden_plms.q_noise)."""
    return prng.normal(SEED, f"plms.m10.q{k}", SHAPE)


# ------------------------------------------------------------------------------------------------ test-local restatement
def ref_plms_sample(eps_fn, x_T, S, scale=1.0, cond=None, uncond=None, mask=None, x0=None, q_noises=None, log_every_t=100, record=None,
                    sched=None):
    """plms.py:115-239 (ddim_use_original_steps False, eta 0) on `eps_fn(x, t, c)` in fp32 torch; CFG as get_model_output (one call on
    [x, x] with [uncond, cond], e_u + s (e_c - e_u), no rescale). record: list of (x, t) per call. Returns (x, intermediates)."""
    sched = od.Schedule() if sched is None else sched
    ds = od.DDIMSchedule(sched, S, 0.0)
    time_range = np.flip(ds.ddim_timesteps)
    n = time_range.shape[0]
    img = x_T.clone().float()
    b = img.shape[0]
    inter = {'x_inter': [img], 'pred_x0': [img]}

    def model(x, t):
        if record is not None:
            record.append((x.clone(), t.clone()))
        if scale == 1.0 or uncond is None:
            return eps_fn(x, t, cond)
        e_u, e_c = eps_fn(torch.cat([x] * 2), torch.cat([t] * 2), torch.cat([uncond, cond])).chunk(2)
        return e_u + scale * (e_c - e_u)

    old_eps = []
    for i, step in enumerate(time_range):
        index = n - i - 1
        ts = torch.full((b,), int(step), dtype=torch.long)
        ts_next = torch.full((b,), int(time_range[min(i + 1, n - 1)]), dtype=torch.long)
        if mask is not None:
            img = od.q_sample(sched, x0, ts, q_noises[i]) * mask + (1. - mask) * img
        sc = ds.scalars(index)
        e_t = model(img, ts)
        if len(old_eps) == 0:
            x_prev, _ = od.ddim_update(img, e_t, *sc)
            e_p = (e_t + model(x_prev, ts_next)) / 2
        elif len(old_eps) == 1:
            e_p = (3 * e_t - old_eps[-1]) / 2
        elif len(old_eps) == 2:
            e_p = (23 * e_t - 16 * old_eps[-1] + 5 * old_eps[-2]) / 12
        else:
            e_p = (55 * e_t - 59 * old_eps[-1] + 37 * old_eps[-2] - 9 * old_eps[-3]) / 24
        img, pred_x0 = od.ddim_update(img, e_p, *sc)
        old_eps.append(e_t)
        if len(old_eps) >= 4:
            old_eps.pop(0)
        if index % log_every_t == 0 or index == n - 1:
            inter['x_inter'].append(img)
            inter['pred_x0'].append(pred_x0)
    return img, inter


def plms_update_ref(x, e_c, e_u, ring, row, scale, phase, n_iters, index, pred_x0=None, x_tmp=None):
    """stedm_plms_step's formula in fp32 torch, with its interface: ring [4, *x.shape] updated in place, x in place (HEUN / MULTISTEP) or
    x_tmp (EULER), pred_x0 (optional) = x0. row: {a_t, a_prev, sigma, sqrt(1 - a_t)}. phase 0 EULER, 1 HEUN, 2 MULTISTEP."""
    a_t, a_prev, _, sq1m = [torch.tensor(float(v), dtype=torch.float32) for v in row]
    e = e_c if e_u is None else e_u + scale * (e_c - e_u)
    i = n_iters - 1 - index if phase == 2 else 0
    order = max(0, min(i, 3))
    r = lambda j: ring[(i - j) % 4]
    if phase == 1:
        ep = (ring[0] + e) / 2
    elif phase == 0 or order == 0:
        ep = e
    elif order == 1:
        ep = (3 * e - r(1)) / 2
    elif order == 2:
        ep = (23 * e - 16 * r(1) + 5 * r(2)) / 12
    else:
        ep = (55 * e - 59 * r(1) + 37 * r(2) - 9 * r(3)) / 24
    x0 = (x - sq1m * ep) / a_t.sqrt()
    xp = a_prev.sqrt() * x0 + (1. - a_prev).sqrt() * ep
    if phase != 1:
        ring[i % 4] = e
    if phase == 0:
        x_tmp.copy_(xp)
    else:
        x.copy_(xp)
        if pred_x0 is not None:
            pred_x0.copy_(x0)
    return x


def f19_case(golden, name):
    f = golden("f19_plms")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    c = {"xT": g("xT"), "cond": g("cond"), "uncond": g("uncond"), "S": int(f[f"{name}_S"]), "scale": float(f[f"{name}_scale"]),
         "t": g(f"{name}_t"), "call_x": g(f"{name}_call_x"), "out": g(f"{name}_out"), "mask": None, "x0": None, "q_noises": None}
    if name == "m10":
        c.update(mask=g("mask"), x0=g("x0"), q_noises=[q_noise(k) for k in range(c["S"])])
    if name == "s20c":
        c["log_iters"] = [int(v) for v in f["s20c_log_iters"]]
    return c


def rel_max(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def _ref(c, **kw):
    return ref_plms_sample(toy_eps, c["xT"], c["S"], c["scale"], c["cond"], c["uncond"], c["mask"], c["x0"], c["q_noises"], **kw)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", CASES)
def test_restated_loop_reproduces_f19(golden, name):
    c = f19_case(golden, name)
    rec = []
    out, _ = _ref(c, record=rec)
    n = od.make_ddim_timesteps(c["S"]).shape[0]
    assert len(rec) == n + 1 == c["t"].shape[0]
    for k, (x, t) in enumerate(rec):
        assert torch.equal(t, c["t"][k].expand(x.shape[0])), k
        assert rel_max(x, c["call_x"][k]) <= F19_TOL, (k, rel_max(x, c["call_x"][k]))
    assert rel_max(out, c["out"]) <= F19_TOL, rel_max(out, c["out"])
    if name == "s1":
        assert int(c["t"][0]) == int(c["t"][1])          # one iteration: t_next == t


@pytest.mark.parametrize("name", CASES)
def test_table_and_kernel_formula_reproduce_the_loop(golden, name):
    from stedm_amd.schedule import make_ddim_tables
    c = f19_case(golden, name)
    sched = od.Schedule()
    tb = make_ddim_tables(sched.alphas_cumprod.numpy(), c["S"], 0.0)
    coefs = torch.from_numpy(tb.coef_table())
    assert bool((coefs[:, 2] == 0).all())
    n = coefs.shape[0]
    x = c["xT"].clone()
    ring = torch.full((4,) + tuple(x.shape), float("nan"))
    x_tmp = torch.empty_like(x)
    cfg = c["scale"] != 1.0
    ev = lambda xx, t: (toy_eps(xx, t, c["cond"]), toy_eps(xx, t, c["uncond"]) if cfg else None)
    calls = []
    for i in range(n):
        index = n - 1 - i
        t = torch.full((2,), int(tb.timesteps[index]), dtype=torch.long)
        if c["mask"] is not None:
            x = od.q_sample(sched, c["x0"], t, c["q_noises"][i]) * c["mask"] + (1. - c["mask"]) * x
        calls.append(x.clone())
        e_c, e_u = ev(x, t)
        if i == 0:
            plms_update_ref(x, e_c, e_u, ring, coefs[index], c["scale"], 0, n, index, x_tmp=x_tmp)
            calls.append(x_tmp.clone())
            e_c, e_u = ev(x_tmp, torch.full((2,), int(tb.timesteps[max(index - 1, 0)]), dtype=torch.long))
            plms_update_ref(x, e_c, e_u, ring, coefs[index], c["scale"], 1, n, index)
        else:
            plms_update_ref(x, e_c, e_u, ring, coefs[index], c["scale"], 2, n, index)
    rec = []
    want, _ = _ref(c, record=rec)
    assert len(calls) == len(rec) and all(torch.equal(a, b[0]) for a, b in zip(calls, rec))        # same process: bit for bit
    assert torch.equal(x, want)
    assert rel_max(x, c["out"]) <= F19_TOL


class _CpuToy:
    """F19's model on the CPU with the surface PLMSSampler reads (the schedule buffers, device, apply_model); records every call."""

    def __init__(self):
        s = od.Schedule()
        self.num_timesteps = 1000
        self.alphas_cumprod = s.alphas_cumprod
        self.sqrt_alphas_cumprod = s.sqrt_alphas_cumprod
        self.sqrt_one_minus_alphas_cumprod = s.sqrt_one_minus_alphas_cumprod
        self.device = torch.device("cpu")
        self.calls = []

    def apply_model(self, x, t, c):
        self.calls.append((x.clone(), t.clone()))
        return toy_eps(x, t, c)


@pytest.fixture
def cpu_kernels(monkeypatch):
    """PLMSSampler's kernels on the CPU: stedm_plms_step by plms_update_ref, the blend by its torch form with the given noise. Returns
    the list of (phase, order) of every update, the order as the kernel derives it from the device index."""
    from stedm_amd import ops, plms
    updates = []

    def step(x, e_c, e_u, ring, coefs, step_idx, n_iters, phase, cfg_scale=1.0, pred_x0=None, x_tmp=None):
        index = int(step_idx[0])
        updates.append((phase, max(0, min(n_iters - 1 - index, 3)) if phase == ops.PLMS_MULTISTEP else None))
        return plms_update_ref(x, e_c, e_u, ring, coefs[index], cfg_scale, phase, n_iters, index, pred_x0=pred_x0, x_tmp=x_tmp)

    def blend(self, img, mask, x0, t, step, noise=None, seed=0, first_id=0):
        assert noise is not None
        img.copy_(od.q_sample(od.Schedule(), x0, t, noise) * mask + (1. - mask) * img)

    monkeypatch.setattr(ops, "plms_step", step)
    monkeypatch.setattr(plms.PLMSSampler, "_blend", blend)
    return updates


@pytest.mark.parametrize("name", CASES)
def test_sampler_loop_reproduces_the_reference_loop_and_logs_by_its_rule(golden, cpu_kernels, name):
    from stedm_amd.plms import PLMSSampler
    c = f19_case(golden, name)
    toy = _CpuToy()
    kw = dict(unconditional_guidance_scale=c["scale"], unconditional_conditioning=c["uncond"]) if c["scale"] != 1.0 else {}
    if c["mask"] is not None:
        kw.update(mask=c["mask"], x0=c["x0"], mask_noises=c["q_noises"])
    seen = []
    x, inter = PLMSSampler(toy).sample(c["S"], 2, (4, 8, 8), c["cond"], x_T=c["xT"], log_every_t=5 if name == "s20c" else 100,
                                       callback=seen.append, **kw)
    n = c["t"].shape[0] - 1
    assert seen == list(range(n))
    cfg = c["scale"] != 1.0
    assert len(toy.calls) == (n + 1) * (2 if cfg else 1)      # duck-typed model: cond then uncond, two calls per evaluation
    rec = []
    want_x, want = _ref(c, log_every_t=5 if name == "s20c" else 100, record=rec)
    for k in range(n + 1):
        cx, ct = toy.calls[k * (2 if cfg else 1)]
        assert torch.equal(cx, rec[k][0]) and bool((ct == c["t"][k]).all()), k                      # same process: bit for bit
    assert torch.equal(x, want_x)
    assert rel_max(x, c["out"]) <= F19_TOL
    # the reference's update at every iteration: Euler + Heun at i = 0 (plms.py:219-223), then order min(i, 3) (:224-232)
    assert cpu_kernels == [(0, None), (1, None)] + [(2, min(i, 3)) for i in range(1, n)]
    assert len(inter["x_inter"]) == len(want["x_inter"]) and len(inter["pred_x0"]) == len(want["pred_x0"])
    assert all(torch.equal(a, b) for a, b in zip(inter["x_inter"], want["x_inter"]))
    assert all(torch.equal(a, b) for a, b in zip(inter["pred_x0"], want["pred_x0"]))
    if name == "s20c":          # the reference's rule: index % 5 == 0 or index == n - 1, after x_T
        res = lambda i: c["out"] if i == n - 1 else c["call_x"][i + 2]
        assert len(inter["x_inter"]) == len(c["log_iters"]) + 1 == 6
        assert all(rel_max(a, res(i)) <= F19_TOL for a, i in zip(inter["x_inter"][1:], c["log_iters"]))


def test_f19_timesteps_and_orders(golden):
    """F19's recorded model times: two calls in iteration 0 (t, then t_next; t_next == t for a single iteration), one per later iteration.
    s4 runs t = 751 (Euler / Heun with t_next 501), 501, 251, 1: orders 1, 2 and 3 once each; the product's tables give the same times."""
    from stedm_amd.schedule import make_ddim_tables
    f = golden("f19_plms")
    assert f["s4_t"].tolist() == [751, 501, 501, 251, 1]
    assert f["s1_t"].tolist() == [1, 1]
    for name in CASES:
        ts = make_ddim_tables(od.Schedule().alphas_cumprod.numpy(), int(f[f"{name}_S"]), 0.0).timesteps[::-1].tolist()
        assert f[f"{name}_t"].tolist() == [ts[0], ts[min(1, len(ts) - 1)]] + ts[1:], name


class _NoDeviceModel:
    """A model whose every use outside the constructor fails the test: the checks must come first."""
    num_timesteps = 1000

    @property
    def device(self):
        raise AssertionError("device work before the argument checks")

    @property
    def alphas_cumprod(self):
        raise AssertionError("schedule work before the argument checks")

    def apply_model(self, *a, **k):
        raise AssertionError("model call before the argument checks")


@pytest.mark.parametrize("kw,exc", [(dict(eta=0.5), ValueError), (dict(quantize_x0=True), NotImplementedError),
                                    (dict(score_corrector=object()), NotImplementedError), (dict(noise_dropout=0.1), NotImplementedError),
                                    (dict(temperature=0.9), NotImplementedError), (dict(noises=[torch.zeros(2, 4, 8, 8)]), NotImplementedError)])
def test_refusals_raise_before_device_work(kw, exc):
    from stedm_amd.plms import PLMSSampler
    s = PLMSSampler(_NoDeviceModel())
    with pytest.raises(exc):
        s.sample(4, 2, (4, 8, 8), torch.zeros(2, 4, 8, 8), x_T=torch.zeros(2, 4, 8, 8), **kw)
    if "eta" in kw:
        with pytest.raises(ValueError):
            s.make_schedule(4, ddim_eta=kw["eta"])


def test_plms_is_a_known_sampler_and_the_default_stays_ddim():
    import inspect
    from stedm_amd import latent_diffusion as ld
    assert ld.SAMPLERS == ("ddim", "dpm_solver", "plms")
    for fn in (ld.LatentDiffusion.sample_log, ld.predict_latents):
        assert inspect.signature(fn).parameters["sampler"].default == "ddim"
