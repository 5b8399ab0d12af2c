"""CPU tier: the general DPM-Solver (stedm_amd/dpm_solver.py: dpm_plan, DPMSolverSampler's new keywords) against fixture F22, the
reference's own DPM_Solver / NoiseScheduleVP('discrete') / model_wrapper with F18's closed-form eps model
(tests/golden/make_golden_dpm_general.py).
  * the plan's model-time table equals every recorded model time bit for bit;
  * `dpm_update_ref` / `dpm_threshold_ref`, test-local torch restatements of stedm_dpm_update / stedm_dpm_threshold, driven by the plan's
    rows, reproduce every recorded call input and every final x;
  * `dpm_threshold_ref`'s quantile equals torch.quantile bit for bit (ties, all-equal rows, -0.0, n from 7 to 65 536);
  * with no new keyword the sampler still runs the 2M path (stedm_dpm_step over dpm_tables), any new setting the plan path;
  * refused options raise before any device work."""
import numpy as np
import pytest
import torch

from tests.test_dpm_solver_oracle import toy_eps

torch.set_grad_enabled(False)

CASES = {     # F22: name -> (steps, CFG scale, DPMSolverSampler.sample keywords); make_golden_dpm_general.CASES
    "ms1_s6": (6, 1.0, dict(order=1, method="multistep")),
    "ms3_cfg_s20": (20, 1.5, dict(order=3, method="multistep")),
    "ms3_s8": (8, 1.0, dict(order=3, method="multistep")),
    "ms3_noise_s10": (10, 1.0, dict(order=3, method="multistep", predict_x0=False)),
    "ms2_taylor_s12": (12, 1.0, dict(order=2, method="multistep", solver_type="taylor", lower_order_final=False)),
    "ss3_logsnr_s9": (9, 1.0, dict(order=3, method="singlestep", skip_type="logSNR")),
    "ss3_noise_s10": (10, 1.0, dict(order=3, method="singlestep", predict_x0=False)),
    "ss3_s11": (11, 1.0, dict(order=3, method="singlestep")),
    "ss3_taylor_cfg_s9": (9, 1.5, dict(order=3, method="singlestep", solver_type="taylor")),
    "ss2_noise_taylor_s7": (7, 1.0, dict(order=2, method="singlestep", predict_x0=False, solver_type="taylor")),
    "ssfixed3_quad_s9": (9, 1.0, dict(order=3, method="singlestep_fixed", skip_type="time_quadratic")),
    "thr_ms2_cfg_s10": (10, 1.5, dict(order=2, method="multistep", thresholding=True, max_val=0.5)),
    "thr_ss3_s10": (10, 1.0, dict(order=3, method="singlestep", thresholding=True, max_val=0.5)),
    "d2z_ms2_s8": (8, 1.0, dict(order=2, method="multistep", denoise_to_zero=True)),
    "d2z_noise_thr_s8": (8, 1.0, dict(order=2, method="multistep", predict_x0=False, thresholding=True, max_val=0.5, denoise_to_zero=True)),
    "tse_ms3_s16": (16, 1.0, dict(order=3, method="multistep", t_start=0.8, t_end=0.01)),
}


def f22_case(golden, name):
    f = golden("f22_dpm_general")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    S, scale, kw = CASES[name]
    c = {"xT": g("xT"), "cond": g("cond"), "uncond": g("uncond"), "ac": g("alphas_cumprod"), "S": S, "scale": scale, "kw": kw,
         "t": g(f"{name}_t"), "out": g(f"{name}_out")}
    c["call_x"] = g(f"{name}_call_x") if f"{name}_call_x" in f.files else None
    return c


def plan_of(c):
    from stedm_amd.dpm_solver import dpm_plan
    return dpm_plan(c["ac"], c["S"], **c["kw"])


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


# ------------------------------------------------------------------------------------------------ test-local restatement
def _f(row, i):
    return torch.tensor(float(row[i]), dtype=torch.float32)


def dpm_update_ref(row, x_in, base, slots, e_c, e_u, scale, mode="all"):
    """stedm_dpm_update's formula in fp32 torch for one plan row. slots: list of 3 tensors (or None), updated in place of the list.
    mode 'all' / 'model' / 'combine'. Returns (x_new, base_new, pred_x0) (None for mode 'model')."""
    from stedm_amd import dpm_solver as D
    ri = lambda i: int(float(row[i]))
    w = ri(D.R_W)
    alpha, sigma = _f(row, D.R_ALPHA), _f(row, D.R_SIGMA)
    to_x0 = float(row[D.R_TO_X0]) != 0.0
    if mode != "combine":
        eps = e_c if e_u is None else e_u + scale * (e_c - e_u)
        slots[w] = (x_in - sigma * eps) / alpha if to_x0 else eps
    if mode == "model":
        return None, None, None
    m = lambda j: slots[ri(j)]
    kind = ri(D.R_KIND)
    a, b, c, d = (_f(row, i) for i in (D.R_A, D.R_B, D.R_C, D.R_D))
    k0, k1, e, f, q = (_f(row, i) for i in (D.R_K0, D.R_K1, D.R_E, D.R_F, D.R_Q))
    if kind == D.K_COPY:
        out = m(D.R_P).clone()
    else:
        out = a * base - b * m(D.R_P)
        if kind == D.K_DIFF:
            out = out + c * (k0 * (m(D.R_U0) - m(D.R_V0)))
        elif kind in (D.K_MS3, D.K_SS3T):
            d10 = k0 * (m(D.R_U0) - m(D.R_V0))
            d11 = k1 * (m(D.R_U1) - m(D.R_V1))
            if kind == D.K_MS3:
                D1, D2 = d10 + e * (d10 - d11), f * (d10 - d11)
            else:
                D1, D2 = (e * d10 - f * d11) / q, (2.0 * (d11 - d10)) / q
            out = (out + c * D1) + d * D2
    pred = slots[w] if to_x0 else (x_in - sigma * slots[w]) / alpha
    return out, (out if float(row[D.R_COMMIT]) != 0.0 else base), pred


def _fma32(a, b, c):
    """fp32 fma: the exact product of two fp32 values in fp64, plus c, rounded once to fp32."""
    return (a.double() * b.double() + c.double()).float()


def quantile_ref(a):
    """torch.quantile(a, 0.995, dim=1) for a [B, n] of non-negative fp32: rank = 0.995 (n - 1) in fp32, the order statistics at
    floor / ceil of it, torch's CPU lerp (an fma on either side of weight 0.5)."""
    n = a.shape[1]
    rank = torch.tensor(0.995, dtype=torch.float32) * (n - 1)
    lo, hi = int(rank.floor()), int(rank.ceil())
    w = rank - lo
    srt = a.sort(dim=1).values
    vb, va = srt[:, lo], srt[:, hi]
    d = va - vb
    if float(w.abs()) < 0.5:
        return _fma32(w.expand_as(d), d, vb)
    return _fma32((w - 1.).expand_as(d), d, va)


def dpm_threshold_ref(x0, max_val):
    """stedm_dpm_threshold's formula: per sample s = max(quantile(|x0|, 0.995), max_val); clamp(x0, -s, s) / s. Returns (x0', q)."""
    B = x0.shape[0]
    q = quantile_ref(x0.abs().reshape(B, -1))
    s = torch.maximum(q, max_val * torch.ones_like(q)).reshape((B,) + (1,) * (x0.dim() - 1))
    return torch.clamp(x0, -s, s) / s, q


def plan_sample(plan, eps_fn, x_T, scale=1.0, cond=None, uncond=None, record=None):
    """The product's loop on the host: row i of the plan per NFE, the kernels' formulas in torch. record: list of (x, t_input)."""
    from stedm_amd import dpm_solver as D
    x = x_T.clone().float()
    base = x.clone()
    B = x.shape[0]
    slots = [None, None, None]
    for i in range(plan.rows.shape[0]):
        row = plan.rows[i]
        t = torch.full((B,), float(plan.t_input[i]), dtype=torch.float32)
        if record is not None:
            record.append((x.clone(), t))
        e_c = eps_fn(x, t, cond)
        e_u = None if (scale == 1.0 or uncond is None) else eps_fn(x, t, uncond)
        if plan.threshold:
            dpm_update_ref(row, x, base, slots, e_c, e_u, scale, mode="model")
            if float(row[D.R_THRESH]) != 0.0:
                w = int(float(row[D.R_W]))
                slots[w] = dpm_threshold_ref(slots[w], plan.max_val)[0]
            x, base, _ = dpm_update_ref(row, x, base, slots, None, None, scale, mode="combine")
        else:
            x, base, _ = dpm_update_ref(row, x, base, slots, e_c, e_u, scale)
    return x


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(CASES))
def test_plan_model_times_equal_the_reference_bitwise(golden, name):
    c = f22_case(golden, name)
    p = plan_of(c)
    assert p.t_input.dtype == torch.float32 and p.rows.shape == (c["t"].shape[0], 24)
    assert torch.equal(p.t_input, c["t"]), (p.t_input - c["t"]).abs().max()
    assert p.commits[-1]


@pytest.mark.parametrize("name", list(CASES))
def test_plan_rows_through_the_restatement_reproduce_f22(golden, name):
    c = f22_case(golden, name)
    p = plan_of(c)
    rec = []
    out = plan_sample(p, toy_eps, c["xT"], c["scale"], c["cond"], c["uncond"], record=rec)
    assert len(rec) == c["t"].shape[0]
    if c["call_x"] is not None:
        for i, (x, _) in enumerate(rec):
            assert rel(x, c["call_x"][i]) <= 1e-5, (i, rel(x, c["call_x"][i]))
    err = rel(out, c["out"])
    print(f"[F22 {name}] plan + restatement vs the reference: max|diff|/std {err:.3e}")
    assert err <= 1e-5


def test_plan_shapes():
    from stedm_amd.dpm_solver import dpm_plan
    from oracle import ddim as od
    ac = od.Schedule().alphas_cumprod
    assert dpm_plan(ac, 20, order=3).orders == [1, 2] + [3] * 18
    assert dpm_plan(ac, 8, order=3).orders == [1, 2, 3, 3, 3, 3, 2, 1]                          # lower_order_final, steps < 15
    assert dpm_plan(ac, 9, order=3, method="singlestep").orders == [0, 0, 3, 0, 0, 3, 0, 2, 1]   # K = 4: [3, 3, 2, 1]
    assert dpm_plan(ac, 10, order=3, method="singlestep").orders == [0, 0, 3] * 3 + [1]
    assert dpm_plan(ac, 11, order=3, method="singlestep").orders == [0, 0, 3] * 3 + [0, 2]
    assert dpm_plan(ac, 10, order=3, method="singlestep_fixed").orders == [0, 0, 3] * 3
    p = dpm_plan(ac, 6, order=2, denoise_to_zero=True, thresholding=True, predict_x0=False)
    assert p.orders[-1] == -1 and len(p.orders) == 7
    assert [float(r[3]) for r in p.rows] == [0.0] * 6 + [1.0]      # only denoise_to_zero thresholds without predict_x0


@pytest.mark.parametrize("n", [7, 256, 2304, 4096, 65536])
def test_threshold_restatement_equals_torch_quantile(n):
    g = torch.Generator().manual_seed(n)
    a = torch.randn(3, n, generator=g) * torch.tensor([[0.3], [2.0], [11.0]])
    ties = (torch.randn(2, n, generator=g) * 4).round() / 4                   # many equal values
    flat = torch.full((1, n), 0.75)                                            # all equal
    zeros = torch.zeros(1, n)
    zeros[0, ::2] = -0.0                                                       # -0.0 and +0.0
    negz = torch.randn(1, n, generator=g)
    negz[0, : n // 2] = -0.0
    for x in (a, ties, flat, zeros, negz):
        q = quantile_ref(x.abs())
        want = torch.quantile(x.abs(), 0.995, dim=1)
        assert torch.equal(q, want), (n, (q - want).abs().max())
        out, q2 = dpm_threshold_ref(x, 1.0)
        s = torch.maximum(want, torch.ones_like(want))[:, None]
        assert torch.equal(out, torch.clamp(x, -s, s) / s) and torch.equal(q2, want)


# ------------------------------------------------------------------------------------------------ the sampler's paths
class _CPUToy:
    parameterization = "eps"
    num_timesteps = 1000
    device = torch.device("cpu")

    def __init__(self, ac):
        self.alphas_cumprod = ac

    def apply_model(self, x, t, c):
        return toy_eps(x, t, c["bias"])


@pytest.fixture
def recorded(monkeypatch):
    from stedm_amd import ops
    calls = []
    monkeypatch.setattr(ops, "dpm_step", lambda *a, **k: calls.append(("dpm_step", a, k)))
    monkeypatch.setattr(ops, "dpm_update", lambda *a, **k: calls.append(("dpm_update", a, k)))
    monkeypatch.setattr(ops, "dpm_threshold", lambda *a, **k: calls.append(("dpm_threshold", a, k)))
    monkeypatch.setattr(ops, "step_advance", lambda *a, **k: None)
    monkeypatch.setattr(ops, "f16_guard_check", lambda *a, **k: None)
    return calls


def test_default_keywords_keep_the_2m_path(golden, recorded):
    from stedm_amd.dpm_solver import DPMSolverSampler, dpm_tables
    c = f22_case(golden, "ms1_s6")
    smp = DPMSolverSampler(_CPUToy(c["ac"]), device=torch.device("cpu"))
    smp.sample(6, 2, (4, 8, 8), {"bias": c["cond"]}, x_T=c["xT"], max_val=3.0)      # max_val alone changes nothing
    assert [k for k, _, _ in recorded] == ["dpm_step"] * 6
    assert torch.equal(recorded[0][1][4], dpm_tables(c["ac"], 6).coefs)
    recorded.clear()
    smp.sample(6, 2, (4, 8, 8), {"bias": c["cond"]}, x_T=c["xT"], order=3)
    assert [k for k, _, _ in recorded] == ["dpm_update"] * 6
    recorded.clear()
    smp.sample(6, 2, (4, 8, 8), {"bias": c["cond"]}, x_T=c["xT"], thresholding=True)
    assert [k for k, _, _ in recorded] == ["dpm_update", "dpm_threshold", "dpm_update"] * 6


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


@pytest.mark.parametrize("kw,exc", [
    (dict(method="adaptive"), NotImplementedError), (dict(method="adaptive", order=3), NotImplementedError),
    (dict(order=0), ValueError), (dict(order=4), ValueError), (dict(order="3"), ValueError), (dict(skip_type="karras"), ValueError),
    (dict(method="euler"), ValueError), (dict(solver_type="heun"), ValueError), (dict(order=3, S=2), ValueError),
    (dict(order=3, eta=0.5), NotImplementedError), (dict(method="singlestep", mask=torch.ones(1, 1, 8, 8)), NotImplementedError),
    (dict(order=3, x0=torch.zeros(2, 4, 8, 8)), NotImplementedError), (dict(thresholding=True, quantize_x0=True), NotImplementedError),
    (dict(order=1, score_corrector=object()), NotImplementedError), (dict(order=3, noise_dropout=0.1), NotImplementedError),
    (dict(order=3, temperature=0.9), NotImplementedError)])
def test_refused_options_raise_before_device_work(golden, kw, exc):
    from stedm_amd.dpm_solver import DPMSolverSampler
    c = f22_case(golden, "ms1_s6")
    kw = dict(kw)
    S = kw.pop("S", 6)
    with pytest.raises(exc):
        DPMSolverSampler(_NoDeviceModel(c["ac"]), device=torch.device("cpu")).sample(S, 2, (4, 8, 8), {"bias": c["cond"]}, x_T=c["xT"], **kw)


def test_dpm_kernels_have_no_spills_or_scratch():
    """The code-object notes of the built dpm.o: stedm_dpm_update's two forms and stedm_dpm_threshold use no scratch and spill nothing."""
    import glob
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "stedm_amd", "csrc", "dpm.o")
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not all(os.path.exists(x) for x in (obj, objdump, readelf)):
        pytest.skip("built objects / llvm tools not present")
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(obj, os.path.join(d, "x.o"))
        subprocess.run([objdump, "--offloading", "x.o"], cwd=d, capture_output=True)
        dev = glob.glob(os.path.join(d, "x.o.*gfx950"))
        assert dev, "no gfx950 code object in dpm.o"
        notes = subprocess.run([readelf, "--notes", dev[0]], capture_output=True, text=True).stdout
    seen, kname = {}, None
    for ln in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", ln)
        if m:
            kname = m.group(1)
        m = re.match(r"\s+\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
        if m and kname and re.search(r"dpm_(update|threshold)_kernel", kname):
            seen.setdefault(kname, 0)
            seen[kname] += 1
            assert int(m.group(2)) == 0, f"{kname}: {m.group(1)} = {m.group(2)}"
    assert len(seen) == 3 and all(v == 3 for v in seen.values()), seen
