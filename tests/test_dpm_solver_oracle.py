"""CPU tier: DPM-Solver++(2M) sampling (stedm_amd/dpm_solver.py) against fixture F18, the reference's own DPMSolverSampler with a
closed-form eps model (tests/golden/make_golden_dpm.py).
  * the product's model-time table equals the recorded model times bit for bit;
  * `ref_dpm_sample`, a test-local fp32 restatement of the reference's multistep loop, reproduces every call's input and the final x —
    it is the yardstick the GPU tier runs over the oracle U-Net;
  * the product's coefficient table, through `dpm_update_ref` (stedm_dpm_step's formula in torch), reproduces the same loop;
  * the general plan with the default keywords (dpm_plan) holds the same rows and model times as `dpm_tables` bit for bit, and its loop
    (`plan_sample`, stedm_dpm_update's formula) returns the bits of the 2M loop (`table_dpm_sample`);
  * the options the sampler does not build, and S < 2, raise before any device work."""
import numpy as np
import pytest
import torch

torch.set_grad_enabled(False)

CASES = ("s20", "s5", "s2")          # F18: S = 20 with CFG 1.5, S = 5 and S = 2 without


def toy_eps(x, t, bias):
    """F18's closed-form eps model (tests/golden/make_golden_dpm.py); the sin(t) term depends on the fraction of t."""
    tf = t.float()[:, None, None, None]
    u = tf / 1000.0
    return torch.tanh(x * (0.5 + u) + bias) * (0.8 + 0.3 * u) + 0.1 * bias + 0.05 * torch.sin(tf)


# ------------------------------------------------------------------------------------------------ test-local restatement
class VPDiscrete:
    """NoiseScheduleVP('discrete', alphas_cumprod) (dpm_solver.py:7-132) in fp32 torch: log(alpha_t) piecewise linear over t_n = (n+1)/N."""

    def __init__(self, alphas_cumprod):
        self.ya = 0.5 * torch.log(torch.as_tensor(alphas_cumprod, dtype=torch.float32))
        self.N = self.ya.shape[0]
        self.xa = torch.linspace(0., 1., self.N + 1)[1:]

    def lmc(self, t):
        j = torch.searchsorted(self.xa, t.contiguous()).clamp(1, self.N - 1) - 1     # segment [x_j, x_j+1] (first or last one outside the keys)
        return self.ya[j] + (t - self.xa[j]) * (self.ya[j + 1] - self.ya[j]) / (self.xa[j + 1] - self.xa[j])

    def alpha(self, t):
        return torch.exp(self.lmc(t))

    def sigma(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.lmc(t)))

    def lam(self, t):
        m = self.lmc(t)
        return m - 0.5 * torch.log(1. - torch.exp(2. * m))


def ref_dpm_sample(eps_fn, x_T, alphas_cumprod, S, scale=1.0, cond=None, uncond=None, record=None):
    """DPM_Solver.sample(steps=S, 'time_uniform', 'multistep', order=2, lower_order_final=True), predict_x0, on `eps_fn(x, t_input, c)`;
    CFG as model_wrapper (one call on [x, x] with [uncond, cond], eu + s (ec - eu)). record: list of (x, t_input) per call."""
    ns = VPDiscrete(alphas_cumprod)
    x = x_T.clone().float()
    B = x.shape[0]
    ts = torch.linspace(1., 1. / ns.N, S + 1)
    ex = lambda v: v[:, None, None, None]
    models = []
    for i in range(S):
        t = ts[i].expand(B)
        t_in = (t - 1. / ns.N) * 1000.
        if record is not None:
            record.append((x.clone(), t_in.clone()))
        if scale == 1.0 or uncond is None:
            e = eps_fn(x, t_in, cond)
        else:
            eu, ec = eps_fn(torch.cat([x, x]), torch.cat([t_in, t_in]), torch.cat([uncond, cond])).chunk(2)
            e = eu + scale * (ec - eu)
        m0 = (x - ex(ns.sigma(t)) * e) / ex(ns.alpha(t))         # data_prediction_fn
        models.append(m0)
        tn = ts[i + 1].expand(B)
        order = 1 if i == 0 or (S < 15 and i == S - 1) else 2
        if order == 1:
            h = ns.lam(tn) - ns.lam(t)
            x = ex(ns.sigma(tn) / ns.sigma(t)) * x - ex(ns.alpha(tn) * torch.expm1(-h)) * m0
        else:
            tp = ts[i - 1].expand(B)
            h0 = ns.lam(t) - ns.lam(tp)
            h = ns.lam(tn) - ns.lam(t)
            r0 = h0 / h
            D1 = ex(1. / r0) * (m0 - models[-2])
            A = ex(ns.alpha(tn) * (torch.exp(-h) - 1.))
            x = ex(ns.sigma(tn) / ns.sigma(t)) * x - A * m0 - 0.5 * A * D1
    return x


def dpm_update_ref(x, e_c, e_u, x0_prev, row, scale):
    """stedm_dpm_step's formula in fp32 torch for one coefficient row {alpha, sigma, r, A, inv_r0, 0.5 A}. Returns (x_new, x0)."""
    alpha, sigma, r, A, inv_r0, hA = [torch.tensor(float(v), dtype=torch.float32) for v in row]
    eps = e_c if e_u is None else e_u + scale * (e_c - e_u)
    x0 = (x - sigma * eps) / alpha
    out = r * x - A * x0
    if float(hA) != 0.0:
        out = out - hA * (inv_r0 * (x0 - x0_prev))
    return out, x0


def table_dpm_sample(eps_fn, x_T, coefs, t_input, scale=1.0, cond=None, uncond=None):
    """The product's loop on the host: t from the model-time table, the update from the coefficient table via dpm_update_ref."""
    x = x_T.clone().float()
    B = x.shape[0]
    x0_prev = torch.full_like(x, float("nan"))
    for i in range(coefs.shape[0]):
        t = torch.full((B,), float(t_input[i]), dtype=torch.float32)
        e_c = eps_fn(x, t, cond)
        e_u = None if (scale == 1.0 or uncond is None) else eps_fn(x, t, uncond)
        x, x0_prev = dpm_update_ref(x, e_c, e_u, x0_prev, coefs[i], scale)
    return x


def rows_2m(plan):
    """The 2M coefficient rows {alpha, sigma, r, A, inv_r0, 0.5 A} from the columns of a default plan (K_DIFF stores c = -(0.5 A))."""
    from stedm_amd import dpm_solver as D
    r = plan.rows
    return torch.stack([r[:, D.R_ALPHA], r[:, D.R_SIGMA], r[:, D.R_A], r[:, D.R_B], r[:, D.R_K0], -r[:, D.R_C]], 1)


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def f18_case(golden, name):
    f = golden("f18_dpm_solver")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    return {"xT": g("xT"), "cond": g("cond"), "uncond": g("uncond"), "ac": g("alphas_cumprod"), "S": int(f[f"{name}_S"]),
            "scale": float(f[f"{name}_scale"]), "t": g(f"{name}_t"), "call_x": g(f"{name}_call_x"), "out": g(f"{name}_out")}


def toy(x, t, c):
    return toy_eps(x, t, c)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", CASES)
def test_model_time_table_equals_the_reference_bitwise(golden, name):
    from stedm_amd.dpm_solver import dpm_tables
    c = f18_case(golden, name)
    tb = dpm_tables(c["ac"], c["S"])
    assert tb.t_input.dtype == torch.float32 and tb.t_input.shape == (c["S"],)
    assert torch.equal(tb.t_input, c["t"])
    assert tb.t_input[0] > 998.0 and (tb.t_input - tb.t_input.round()).abs().max() > 0.01     # fractional model times
    S = c["S"]
    assert tb.orders == [1] + [2] * (S - 2) + [1 if S < 15 else 2]


@pytest.mark.parametrize("name", CASES)
def test_restated_loop_reproduces_f18(golden, name):
    c = f18_case(golden, name)
    rec = []
    out = ref_dpm_sample(toy, c["xT"], c["ac"], c["S"], c["scale"], c["cond"], c["uncond"], record=rec)
    assert len(rec) == c["S"]
    for i, (x, t) in enumerate(rec):
        assert torch.equal(t, c["t"][i].expand(x.shape[0])), i
        assert rel(x, c["call_x"][i]) <= 1e-6, (i, rel(x, c["call_x"][i]))
    assert rel(out, c["out"]) <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_coefficient_table_reproduces_the_loop(golden, name):
    from stedm_amd.dpm_solver import dpm_tables
    c = f18_case(golden, name)
    tb = dpm_tables(c["ac"], c["S"])
    assert tb.coefs.dtype == torch.float32 and tuple(tb.coefs.shape) == (c["S"], 6)
    assert bool((tb.coefs[:, 5] == 0).eq(torch.tensor([o == 1 for o in tb.orders])).all())
    out = table_dpm_sample(toy, c["xT"], tb.coefs, tb.t_input, c["scale"], c["cond"], c["uncond"])
    assert rel(out, c["out"]) <= 1e-6
    assert rel(out, ref_dpm_sample(toy, c["xT"], c["ac"], c["S"], c["scale"], c["cond"], c["uncond"])) <= 1e-6


@pytest.mark.parametrize("scale", [1.0, 1.5])
@pytest.mark.parametrize("S", [2, 3, 5, 14, 15, 20, 33])
def test_default_plan_is_the_2m_update_bitwise(golden, S, scale):
    """The default keywords' plan: first order at step 0 (and at the last step when S < 15), K_DIFF elsewhere, data prediction, every
    row commits, model j in ring slot j mod 3 and the difference against slot (j - 1) mod 3. Its columns are dpm_tables' rows and its
    loop (plan_sample) returns the bits of the 2M expression (table_dpm_sample): (a x - b m) + (-(0.5 A)) D is (r x - A x0) - (0.5 A) D."""
    from stedm_amd import dpm_solver as D
    from tests.test_dpm_solver_general_oracle import plan_sample
    c = f18_case(golden, "s20")
    p, tb = D.dpm_plan(c["ac"], S), D.dpm_tables(c["ac"], S)
    first = [j == 0 or (S < 15 and j == S - 1) for j in range(S)]
    assert p.rows.shape == (S, 24) and not p.threshold
    assert p.orders == tb.orders == [1 if f else 2 for f in first] and p.commits == [True] * S
    col = lambda i: [int(v) for v in p.rows[:, i]]
    assert col(D.R_KIND) == [D.K_FIRST if f else D.K_DIFF for f in first]
    assert col(D.R_TO_X0) == [1] * S and col(D.R_THRESH) == [0] * S and col(D.R_COMMIT) == [1] * S
    assert col(D.R_W) == col(D.R_P) == [j % 3 for j in range(S)]
    for j in range(S):
        if not first[j]:
            assert (int(p.rows[j, D.R_U0]), int(p.rows[j, D.R_V0])) == (j % 3, (j - 1) % 3), j
    coefs = rows_2m(p)
    assert torch.equal(p.t_input, tb.t_input)
    assert torch.equal(coefs[:, :4], tb.coefs[:, :4])
    assert torch.equal(coefs[:, 5], tb.coefs[:, 5]) and bool((coefs[:, 5] == 0).eq(torch.tensor(first)).all())
    assert all(torch.equal(coefs[j, 4], tb.coefs[j, 4]) for j in range(S) if not first[j])       # inv_r0: unused at first order
    want = table_dpm_sample(toy, c["xT"], tb.coefs, tb.t_input, scale, c["cond"], c["uncond"])
    assert torch.equal(table_dpm_sample(toy, c["xT"], coefs, p.t_input, scale, c["cond"], c["uncond"]), want)
    got = plan_sample(p, toy, c["xT"], scale, c["cond"], c["uncond"])
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


class _NoDeviceModel:
    """A model whose every use outside the schedule fails the test: the checks must come first."""
    parameterization = "eps"
    num_timesteps = 1000

    def __init__(self, ac):
        self.alphas_cumprod = ac

    @property
    def device(self):
        raise AssertionError("device work before the argument checks")

    def apply_model(self, *a, **k):
        raise AssertionError("model call before the argument checks")


@pytest.mark.parametrize("kw", [dict(mask=torch.ones(1, 1, 8, 8)), dict(x0=torch.zeros(2, 4, 8, 8)), dict(eta=0.5), dict(quantize_x0=True),
                                dict(score_corrector=object()), dict(noise_dropout=0.1), dict(temperature=0.9)])
def test_unbuilt_options_raise_before_device_work(golden, kw):
    from stedm_amd.dpm_solver import DPMSolverSampler
    c = f18_case(golden, "s5")
    s = DPMSolverSampler(_NoDeviceModel(c["ac"]), device=torch.device("cpu"))
    with pytest.raises(NotImplementedError):
        s.sample(5, 2, (4, 8, 8), {"bias": c["cond"]}, x_T=c["xT"], **kw)


@pytest.mark.parametrize("S", [0, 1])
def test_fewer_than_two_steps_raise_before_device_work(golden, S):
    from stedm_amd.dpm_solver import DPMSolverSampler, dpm_tables
    c = f18_case(golden, "s5")
    with pytest.raises(ValueError):
        DPMSolverSampler(_NoDeviceModel(c["ac"]), device=torch.device("cpu")).sample(S, 2, (4, 8, 8), {"bias": c["cond"]}, x_T=c["xT"])
    with pytest.raises(ValueError):
        dpm_tables(c["ac"], S)

