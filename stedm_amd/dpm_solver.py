"""DPM-Solver++(2M) sampler, HIP-backed.

Mirrors `ldm.models.diffusion.dpm_solver.sampler.DPMSolverSampler` (reference sampler.py:12-95): same constructor and `sample`
surface, the same solver — multistep DPM-Solver++ of order 2 (predict_x0=True, solver_type 'dpm_solver', thresholding off),
skip_type 'time_uniform', lower_order_final=True (sampler.py:82-93) — and exactly S model evaluations for S steps.

Step i evaluates the model at t_i and moves x from t_i to t_{i+1} (i = 0 .. S-1, the shape of the reference's loop,
dpm_solver.py:1053-1083). The host builds every per-step scalar once (`dpm_tables`, the reference's fp32 arithmetic restated with torch
CPU ops in its order); every tensor operation of a step runs in HIP kernels:
  * the model call at the fractional model time t_input = (t - 1/N) * 1000 (dpm_solver.py:246-253) -> the U-Net with float32
    timesteps (stedm_time_embed_f32), one shared-encoder CFG pass (`apply_model_cfg`) when the model offers it;
  * CFG combine, data prediction and the multistep update -> one fused kernel (stedm_dpm_step);
  * with `use_graph=True` the whole step (model time from the device table, U-Net, update, step counter) is captured once in a
    hipGraph and replayed for the remaining steps.

The rest of the reference's DPM_Solver.sample (orders 1-3, singlestep / singlestep_fixed, noise prediction, 'taylor', 'logSNR' /
'time_quadratic', denoise_to_zero, t_start / t_end, dynamic thresholding) runs from a host plan with one row per model evaluation
(`dpm_plan`) through stedm_dpm_update / stedm_dpm_threshold (`DPMPlanGraph`); the default keywords keep the 2M path above.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import torch

from . import ops
from .ddim import refuse_guidance_rows

MODEL_TYPES = {"eps": "noise"}      # sampler.py:7-10 ('v' is not a parameterization of the STEDM configs)


@dataclass
class DPMTables:
    """Host tables of one S-step run. t_cont: fp32 [S+1] continuous times, 1 -> 1/N (get_time_steps 'time_uniform'); t_input: fp32 [S]
    model times of the S evaluations; coefs: fp32 [S, ops.DPM_NCOEF] rows {alpha_i, sigma_i, r, A, inv_r0, 0.5 A} of stedm_dpm_step;
    orders: the solver order of every step."""
    t_cont: torch.Tensor
    t_input: torch.Tensor
    coefs: torch.Tensor
    orders: List[int]


class _VPSchedule:
    """NoiseScheduleVP('discrete', alphas_cumprod=...) (dpm_solver.py:7-152) on fp32 CPU tensors of any shape: log(alpha_t) is the
    piecewise-linear interpolation of 0.5 log(alphas_cumprod) over the keypoints t_n = (n + 1) / N, extended linearly beyond the ends;
    inverse_lambda (:140-152) is log_alpha = -0.5 logaddexp(0, -2 lambda), then the same interpolation over the flipped keypoints (t as
    a function of log_alpha)."""

    def __init__(self, alphas_cumprod):
        ac = torch.as_tensor(alphas_cumprod).detach().to("cpu", torch.float32)
        self.log_alpha = 0.5 * torch.log(ac)
        self.N = int(ac.shape[0])
        self.t_keys = torch.linspace(0., 1., self.N + 1)[1:]
        self.la_flip = torch.flip(self.log_alpha, [0])
        self.t_flip = torch.flip(self.t_keys, [0])

    @staticmethod
    def _interp(x, xp, yp):
        # segment j holds x: the last keypoint strictly below x, clamped to the first / last segment (the reference's sort-based search
        # places x ahead of an equal keypoint); then y_j + (x - x_j) (y_{j+1} - y_j) / (x_{j+1} - x_j), in that order
        K = xp.shape[0]
        shp = x.shape
        x = x.reshape(-1)
        j = ((xp[None, :] < x[:, None]).sum(1) - 1).clamp(0, K - 2)
        x0, x1, y0, y1 = xp[j], xp[j + 1], yp[j], yp[j + 1]
        return (y0 + (x - x0) * (y1 - y0) / (x1 - x0)).reshape(shp)

    def log_mean_coeff(self, t):
        return self._interp(t, self.t_keys, self.log_alpha)

    def alpha(self, t):
        return torch.exp(self.log_mean_coeff(t))

    def std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.log_mean_coeff(t)))

    def lam(self, t):
        lmc = self.log_mean_coeff(t)
        return lmc - 0.5 * torch.log(1. - torch.exp(2. * lmc))

    def inverse_lambda(self, lamb):
        log_alpha = -0.5 * torch.logaddexp(torch.zeros((1,)), -2. * lamb)
        return self._interp(log_alpha.reshape(-1), self.la_flip, self.t_flip).reshape((-1,))


def dpm_tables(alphas_cumprod, S: int, lower_order_final: bool = True) -> DPMTables:
    """Every per-step scalar of DPM_Solver.sample(steps=S, skip_type='time_uniform', method='multistep', order=2, lower_order_final)
    for a discrete-time model with these alphas_cumprod. Each scalar is one-element fp32 torch arithmetic in the reference's order:
    first-order rows (step 0; the last step when S < 15) follow dpm_solver_first_update (A = alpha_t expm1(-h)), second-order rows
    multistep_dpm_solver_second_update (A = alpha_t (exp(-h) - 1), inv_r0 = 1 / (h_0 / h))."""
    S = int(S)
    if S < 2:
        raise ValueError(f"DPM-Solver++(2M) needs S >= 2 steps (the reference asserts steps >= order), got {S}")
    ns = _VPSchedule(alphas_cumprod)
    t_cont = torch.linspace(1., 1. / ns.N, S + 1)
    t_input = ((t_cont[:S] - 1. / ns.N) * 1000.).contiguous()
    rows, orders = [], []
    one = lambda i: t_cont[i:i + 1]
    for i in range(S):
        s, t = one(i), one(i + 1)
        order = 1 if i == 0 or (lower_order_final and S < 15 and i == S - 1) else 2
        alpha_s, sigma_s = ns.alpha(s), ns.std(s)
        sigma_t, alpha_t = ns.std(t), torch.exp(ns.log_mean_coeff(t))
        if order == 1:
            h = ns.lam(t) - ns.lam(s)
            A = alpha_t * torch.expm1(-h)
            inv_r0 = torch.zeros_like(A)
            half_A = torch.zeros_like(A)
        else:
            l1, l0, lt = ns.lam(one(i - 1)), ns.lam(s), ns.lam(t)
            h_0 = l0 - l1
            h = lt - l0
            inv_r0 = 1. / (h_0 / h)
            A = alpha_t * (torch.exp(-h) - 1.)
            half_A = 0.5 * A
        rows.append(torch.cat([alpha_s, sigma_s, sigma_t / sigma_s, A, inv_r0, half_A]))
        orders.append(order)
    return DPMTables(t_cont=t_cont, t_input=t_input, coefs=torch.stack(rows).contiguous(), orders=orders)


# ------------------------------------------------------------------------------------------------ the general planner
METHODS = ("multistep", "singlestep", "singlestep_fixed")
SKIP_TYPES = ("time_uniform", "logSNR", "time_quadratic")
SOLVER_TYPES = ("dpm_solver", "taylor")
# stedm_dpm_update row layout (STEDM_DPMU_*): the fields of one model evaluation (NFE) and of the update after it
(R_ALPHA, R_SIGMA, R_TO_X0, R_THRESH, R_W, R_KIND, R_COMMIT, R_P, R_U0, R_V0, R_U1, R_V1,
 R_A, R_B, R_C, R_D, R_K0, R_K1, R_E, R_F, R_Q) = range(21)
# update kinds over the base x and the slots m_j; every "- c D" of the reference is stored as "+ (-c) D" (the same bits)
K_FIRST, K_DIFF, K_MS3, K_SS3T, K_COPY = range(5)
#   K_FIRST  a x - b m_P
#   K_DIFF   (a x - b m_P) + c (k0 (m_U0 - m_V0))
#   K_MS3    D10 = k0 (m_U0 - m_V0), D11 = k1 (m_U1 - m_V1), D1 = D10 + e (D10 - D11), D2 = f (D10 - D11);  ((a x - b m_P) + c D1) + d D2
#   K_SS3T   D10, D11 as K_MS3, D1 = (e D10 - f D11) / q, D2 = (2 (D11 - D10)) / q;                      ((a x - b m_P) + c D1) + d D2
#   K_COPY   m_P


@dataclass
class DPMPlan:
    """Host plan of a general DPM-Solver run, one row per model evaluation (NFE). t_input: fp32 [R] model times; rows: fp32
    [R, ops.DPMU_NCOEF] in the R_* layout; orders: the order of the update each row finishes (0: a singlestep intermediate, -1:
    denoise_to_zero); commits: whether the row's result replaces the base x."""
    t_input: torch.Tensor
    rows: torch.Tensor
    orders: List[int]
    commits: List[bool]
    threshold: bool
    max_val: float


def _get_time_steps(ns: _VPSchedule, skip_type, t_T, t_0, N):
    """DPM_Solver.get_time_steps (dpm_solver.py:396-421) on the CPU."""
    if skip_type == "logSNR":
        lambda_T = ns.lam(torch.tensor(t_T).reshape(1)).reshape(())
        lambda_0 = ns.lam(torch.tensor(t_0).reshape(1)).reshape(())
        logSNR_steps = torch.linspace(lambda_T.item(), lambda_0.item(), N + 1)
        return ns.inverse_lambda(logSNR_steps)
    if skip_type == "time_uniform":
        return torch.linspace(t_T, t_0, N + 1)
    if skip_type == "time_quadratic":
        t_order = 2
        return torch.linspace(t_T ** (1. / t_order), t_0 ** (1. / t_order), N + 1).pow(t_order)
    raise ValueError(f"Unsupported skip_type {skip_type!r}, need to be one of {SKIP_TYPES}")


def _singlestep_orders(steps, order):
    """get_orders_and_timesteps_for_singlestep_solver (dpm_solver.py:423-474): K and the orders."""
    if order == 3:
        K = steps // 3 + 1
        orders = [3] * (K - 2) + [2, 1] if steps % 3 == 0 else ([3] * (K - 1) + [1] if steps % 3 == 1 else [3] * (K - 1) + [2])
    elif order == 2:
        K = steps // 2 if steps % 2 == 0 else steps // 2 + 1
        orders = [2] * K if steps % 2 == 0 else [2] * (K - 1) + [1]
    else:
        K, orders = 1, [1] * steps
    return K, orders


def check_dpm_options(steps, order=2, method="multistep", skip_type="time_uniform", solver_type="dpm_solver"):
    """The checks of DPM_Solver.sample, before any device work: 'adaptive' -> NotImplementedError, the rest -> ValueError."""
    if method == "adaptive":
        raise NotImplementedError("DPM-Solver method 'adaptive': its NFE count depends on the data (a host decision every step)")
    if method not in METHODS:
        raise ValueError(f"DPM-Solver method {method!r}: one of {METHODS} (or 'adaptive', not built)")
    if isinstance(order, bool) or not isinstance(order, int) or order not in (1, 2, 3):
        raise ValueError(f"DPM-Solver order must be 1, 2 or 3, got {order!r}")
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"Unsupported skip_type {skip_type!r}, need to be one of {SKIP_TYPES}")
    if solver_type not in SOLVER_TYPES:
        raise ValueError(f"'solver_type' must be either 'dpm_solver' or 'taylor', got {solver_type!r}")
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"DPM-Solver needs steps >= 1, got {steps}")
    if method == "multistep" and steps < order:
        raise ValueError(f"multistep DPM-Solver of order {order} needs steps >= order (the reference asserts it), got {steps}")
    if method == "singlestep_fixed" and steps < order:
        raise ValueError(f"singlestep_fixed DPM-Solver of order {order} needs steps >= order, got {steps}")
    if method == "singlestep" and order == 1 and skip_type == "logSNR" and steps > 1:
        raise ValueError("singlestep order 1 with skip_type 'logSNR': the reference indexes its K + 1 = 2 outer times with `steps` orders")


def dpm_plan(alphas_cumprod, steps, order=2, method="multistep", skip_type="time_uniform", predict_x0=True, solver_type="dpm_solver",
             lower_order_final=True, denoise_to_zero=False, t_start=None, t_end=None, thresholding=False, max_val=1.0) -> DPMPlan:
    """Every per-NFE scalar of DPM_Solver(predict_x0, thresholding, max_val).sample(steps, t_start, t_end, order, skip_type, method,
    lower_order_final, denoise_to_zero, solver_type) (dpm_solver.py:1000-1090) for a discrete-time model with these alphas_cumprod.
    Each scalar is fp32 torch arithmetic in the reference's order, on one-element tensors (the reference's [B] vectors for B < 16).
    Multistep keeps the models in a ring of 3 slots (NFE j -> slot j mod 3); singlestep keeps model_s / model_s1 / model_s2 of the current
    outer step in slots 0 / 1 / 2. One deviation: with order 3, lower_order_final and steps < 15 the reference's second-order step unpacks
    its 3-entry model list into two names and raises; here it reads the last two entries, as later DPM-Solver releases do."""
    check_dpm_options(steps, order, method, skip_type, solver_type)
    steps = int(steps)
    ns = _VPSchedule(alphas_cumprod)
    t_0 = 1. / ns.N if t_end is None else float(t_end)
    t_T = 1. if t_start is None else float(t_start)
    one = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(1)
    rows, t_in, orders, commits = [], [], [], []

    def nfe(t, w, to_x0, kind, commit, P, coef, U=(0, 0, 0, 0), order_tag=0):
        """One row: the model at time t [1] into slot w, then the update `kind` with coefficients coef {a, b, c, d, k0, k1, e, f, q}."""
        r = torch.zeros(ops.DPMU_NCOEF)
        r[R_ALPHA], r[R_SIGMA] = ns.alpha(t)[0], ns.std(t)[0]
        r[R_TO_X0] = 1. if to_x0 else 0.
        r[R_THRESH] = 1. if (to_x0 and thresholding) else 0.
        r[R_W], r[R_KIND], r[R_COMMIT], r[R_P] = w, kind, 1. if commit else 0., P
        r[R_U0], r[R_V0], r[R_U1], r[R_V1] = U
        for name, idx in (("a", R_A), ("b", R_B), ("c", R_C), ("d", R_D), ("k0", R_K0), ("k1", R_K1), ("e", R_E), ("f", R_F), ("q", R_Q)):
            if name in coef:
                r[idx] = torch.as_tensor(coef[name], dtype=torch.float32).reshape(())
        rows.append(r)
        t_in.append(((t - 1. / ns.N) * 1000.)[0])
        orders.append(order_tag)
        commits.append(bool(commit))

    def first(s, t):
        """dpm_solver_first_update (:478-517): {a, b} of x_t = a x - b m_s."""
        lambda_s, lambda_t = ns.lam(s), ns.lam(t)
        h = lambda_t - lambda_s
        log_alpha_s, log_alpha_t = ns.log_mean_coeff(s), ns.log_mean_coeff(t)
        sigma_s, sigma_t = ns.std(s), ns.std(t)
        alpha_t = torch.exp(log_alpha_t)
        if predict_x0:
            return dict(a=sigma_t / sigma_s, b=alpha_t * torch.expm1(-h))
        return dict(a=torch.exp(log_alpha_t - log_alpha_s), b=sigma_t * torch.expm1(h))

    if method == "multistep":
        ts = _get_time_steps(ns, skip_type, t_T, t_0, steps)
        for j in range(steps):          # NFE j at ts[j], then the update to ts[j + 1]
            if j + 1 < order:
                step_order = j + 1
            else:
                step_order = min(order, steps - j) if (lower_order_final and steps < 15) else order
            t, p0 = one(ts[j + 1]), one(ts[j])
            sl = [j % 3, (j - 1) % 3, (j - 2) % 3]          # the slots of model_prev_0, _1, _2
            if step_order == 1:
                nfe(p0, sl[0], predict_x0, K_FIRST, True, sl[0], first(p0, t), order_tag=1)
                continue
            p1 = one(ts[j - 1])
            lambda_prev_1, lambda_prev_0, lambda_t = ns.lam(p1), ns.lam(p0), ns.lam(t)
            log_alpha_prev_0, log_alpha_t = ns.log_mean_coeff(p0), ns.log_mean_coeff(t)
            sigma_prev_0, sigma_t = ns.std(p0), ns.std(t)
            alpha_t = torch.exp(log_alpha_t)
            if step_order == 2:          # multistep_dpm_solver_second_update (:732-782)
                h_0 = lambda_prev_0 - lambda_prev_1
                h = lambda_t - lambda_prev_0
                r0 = h_0 / h
                if predict_x0:
                    a, B = sigma_t / sigma_prev_0, alpha_t * (torch.exp(-h) - 1.)
                    c = -(0.5 * B) if solver_type == "dpm_solver" else alpha_t * ((torch.exp(-h) - 1.) / h + 1.)
                else:
                    a, B = torch.exp(log_alpha_t - log_alpha_prev_0), sigma_t * (torch.exp(h) - 1.)
                    c = -(0.5 * B) if solver_type == "dpm_solver" else -(sigma_t * ((torch.exp(h) - 1.) / h - 1.))
                nfe(p0, sl[0], predict_x0, K_DIFF, True, sl[0], dict(a=a, b=B, c=c, k0=1. / r0), U=(sl[0], sl[1], 0, 0), order_tag=2)
                continue
            lambda_prev_2 = ns.lam(one(ts[j - 2]))         # multistep_dpm_solver_third_update (:784-829)
            h_1 = lambda_prev_1 - lambda_prev_2
            h_0 = lambda_prev_0 - lambda_prev_1
            h = lambda_t - lambda_prev_0
            r0, r1 = h_0 / h, h_1 / h
            co = dict(k0=1. / r0, k1=1. / r1, e=r0 / (r0 + r1), f=1. / (r0 + r1))
            if predict_x0:
                co.update(a=sigma_t / sigma_prev_0, b=alpha_t * (torch.exp(-h) - 1.), c=alpha_t * ((torch.exp(-h) - 1.) / h + 1.),
                          d=-(alpha_t * ((torch.exp(-h) - 1. + h) / h ** 2 - 0.5)))
            else:
                co.update(a=torch.exp(log_alpha_t - log_alpha_prev_0), b=sigma_t * (torch.exp(h) - 1.),
                          c=-(sigma_t * ((torch.exp(h) - 1.) / h - 1.)), d=-(sigma_t * ((torch.exp(h) - 1. - h) / h ** 2 - 0.5)))
            nfe(p0, sl[0], predict_x0, K_MS3, True, sl[0], co, U=(sl[0], sl[1], sl[1], sl[2]), order_tag=3)
    else:
        if method == "singlestep":
            K, ords = _singlestep_orders(steps, order)
            if skip_type == "logSNR":
                outer = _get_time_steps(ns, skip_type, t_T, t_0, K)
            else:
                outer = _get_time_steps(ns, skip_type, t_T, t_0, steps)[torch.cumsum(torch.tensor([0] + ords), dim=0)]
        else:
            K = steps // order
            ords = [order] * K
            outer = _get_time_steps(ns, skip_type, t_T, t_0, K)
        for i, o in enumerate(ords):
            t_T_inner, t_0_inner = outer[i], outer[i + 1]
            inner = _get_time_steps(ns, skip_type, t_T_inner.item(), t_0_inner.item(), o)
            lambda_inner = ns.lam(inner)
            s, t = one(t_T_inner), one(t_0_inner)
            hh = lambda_inner[-1] - lambda_inner[0]
            if o == 1:
                nfe(s, 0, predict_x0, K_FIRST, True, 0, first(s, t), order_tag=1)
                continue
            r1 = (lambda_inner[1] - lambda_inner[0]) / hh
            lambda_s, lambda_t = ns.lam(s), ns.lam(t)
            h = lambda_t - lambda_s
            s1 = ns.inverse_lambda(lambda_s + r1 * h)
            if o == 2:                   # singlestep_dpm_solver_second_update (:519-591)
                log_alpha_s, log_alpha_s1, log_alpha_t = ns.log_mean_coeff(s), ns.log_mean_coeff(s1), ns.log_mean_coeff(t)
                sigma_s, sigma_s1, sigma_t = ns.std(s), ns.std(s1), ns.std(t)
                alpha_s1, alpha_t = torch.exp(log_alpha_s1), torch.exp(log_alpha_t)
                if predict_x0:
                    phi_11, phi_1 = torch.expm1(-r1 * h), torch.expm1(-h)
                    u1 = dict(a=sigma_s1 / sigma_s, b=alpha_s1 * phi_11)
                    a, b = sigma_t / sigma_s, alpha_t * phi_1
                    c = -((0.5 / r1) * (alpha_t * phi_1)) if solver_type == "dpm_solver" else \
                        (1. / r1) * (alpha_t * ((torch.exp(-h) - 1.) / h + 1.))
                else:
                    phi_11, phi_1 = torch.expm1(r1 * h), torch.expm1(h)
                    u1 = dict(a=torch.exp(log_alpha_s1 - log_alpha_s), b=sigma_s1 * phi_11)
                    a, b = torch.exp(log_alpha_t - log_alpha_s), sigma_t * phi_1
                    c = -((0.5 / r1) * (sigma_t * phi_1)) if solver_type == "dpm_solver" else \
                        -((1. / r1) * (sigma_t * ((torch.exp(h) - 1.) / h - 1.)))
                nfe(s, 0, predict_x0, K_FIRST, False, 0, u1, order_tag=0)
                nfe(s1, 1, predict_x0, K_DIFF, True, 0, dict(a=a, b=b, c=c, k0=1.), U=(1, 0, 0, 0), order_tag=2)
                continue
            r2 = (lambda_inner[2] - lambda_inner[0]) / hh    # singlestep_dpm_solver_third_update (:593-700)
            s2 = ns.inverse_lambda(lambda_s + r2 * h)
            log_alpha_s, log_alpha_s1, log_alpha_s2, log_alpha_t = (ns.log_mean_coeff(s), ns.log_mean_coeff(s1), ns.log_mean_coeff(s2),
                                                                    ns.log_mean_coeff(t))
            sigma_s, sigma_s1, sigma_s2, sigma_t = ns.std(s), ns.std(s1), ns.std(s2), ns.std(t)
            alpha_s1, alpha_s2, alpha_t = torch.exp(log_alpha_s1), torch.exp(log_alpha_s2), torch.exp(log_alpha_t)
            if predict_x0:
                phi_11, phi_12, phi_1 = torch.expm1(-r1 * h), torch.expm1(-r2 * h), torch.expm1(-h)
                phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
                phi_2 = phi_1 / h + 1.
                phi_3 = phi_2 / h - 0.5
                u1 = dict(a=sigma_s1 / sigma_s, b=alpha_s1 * phi_11)
                u2 = dict(a=sigma_s2 / sigma_s, b=alpha_s2 * phi_12, c=r2 / r1 * (alpha_s2 * phi_22), k0=1.)
                a, b = sigma_t / sigma_s, alpha_t * phi_1
                c_dpm = (1. / r2) * (alpha_t * phi_2)
                c_tay, d_tay = alpha_t * phi_2, -(alpha_t * phi_3)
            else:
                phi_11, phi_12, phi_1 = torch.expm1(r1 * h), torch.expm1(r2 * h), torch.expm1(h)
                phi_22 = torch.expm1(r2 * h) / (r2 * h) - 1.
                phi_2 = phi_1 / h - 1.
                phi_3 = phi_2 / h - 0.5
                u1 = dict(a=torch.exp(log_alpha_s1 - log_alpha_s), b=sigma_s1 * phi_11)
                u2 = dict(a=torch.exp(log_alpha_s2 - log_alpha_s), b=sigma_s2 * phi_12, c=-(r2 / r1 * (sigma_s2 * phi_22)), k0=1.)
                a, b = torch.exp(log_alpha_t - log_alpha_s), sigma_t * phi_1
                c_dpm = -((1. / r2) * (sigma_t * phi_2))
                c_tay, d_tay = -(sigma_t * phi_2), -(sigma_t * phi_3)
            nfe(s, 0, predict_x0, K_FIRST, False, 0, u1, order_tag=0)
            nfe(s1, 1, predict_x0, K_DIFF, False, 0, u2, U=(1, 0, 0, 0), order_tag=0)
            if solver_type == "dpm_solver":
                nfe(s2, 2, predict_x0, K_DIFF, True, 0, dict(a=a, b=b, c=c_dpm, k0=1.), U=(2, 0, 0, 0), order_tag=3)
            else:
                nfe(s2, 2, predict_x0, K_SS3T, True, 0, dict(a=a, b=b, c=c_tay, d=d_tay, k0=1. / r1, k1=1. / r2, e=r2, f=r1, q=r2 - r1),
                    U=(1, 0, 2, 0), order_tag=3)
    if denoise_to_zero:      # denoise_to_zero_fn (:476-480): data_prediction_fn at t_0 whatever predict_x0 says, thresholding included
        nfe(one(t_0), 0, True, K_COPY, True, 0, {}, order_tag=-1)
    return DPMPlan(t_input=torch.stack(t_in).contiguous(), rows=torch.stack(rows).contiguous(), orders=orders, commits=commits,
                   threshold=bool(thresholding), max_val=float(max_val))


class DPMSolverSampler(object):
    def __init__(self, model, device=torch.device("cuda"), **kwargs):
        """sampler.py:13-18. The run happens where the model lives (its tensors and the HIP kernels); `device` is kept for the
        reference's signature. use_graph=True: hipGraph replay of the step (DPMStepGraph)."""
        super().__init__()
        self.model = model
        self.device = device
        self.use_graph = bool(kwargs.get("use_graph", False))
        self.alphas_cumprod = model.alphas_cumprod.detach().clone().to(torch.float32)

    def make_schedule(self, S, tables=None):
        """The host tables of an S-step run (dpm_tables) and their device copies: the model times and the coefficient rows."""
        tb = dpm_tables(self.alphas_cumprod, S) if tables is None else tables
        dev = self.model.device
        self.tables = tb
        self._coefs = tb.coefs.to(dev)
        self._t_table = tb.t_input.to(dev)
        return tb

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, order=2, method="multistep", skip_type="time_uniform", predict_x0=True,
               solver_type="dpm_solver", lower_order_final=True, denoise_to_zero=False, thresholding=False, max_val=1.0, t_start=None,
               t_end=None, **kwargs):
        """sampler.py:24-95 -> (x, None). The reference accepts mask / x0 / eta / quantize_x0 / score_corrector / noise_dropout /
        temperature and ignores them; here they raise NotImplementedError, and S < 2 raises ValueError, before any device work.
        callback(i) and img_callback(pred_x0, i) are called after step i (eager loop; the reference calls neither).

        The keywords order .. t_end are those of DPM_Solver(predict_x0, thresholding, max_val).sample(steps=S, t_start, t_end, order,
        skip_type, method, lower_order_final, denoise_to_zero, solver_type) (dpm_solver.py:1000-1090). With their defaults (the
        reference sampler's DPM-Solver++(2M)) the run takes the 2M path above (dpm_tables, stedm_dpm_step); any other setting runs the
        general plan (dpm_plan, stedm_dpm_update, stedm_dpm_threshold), one model evaluation (NFE) per row, callbacks per NFE.
        method 'adaptive' raises NotImplementedError; an order outside 1..3, an unknown method / skip_type / solver_type, or multistep
        S < order raise ValueError, before any device work. One unconditional_guidance_scale for the batch: per-sample scales (a sequence
        or 1-D tensor) raise NotImplementedError - DDIMSampler has them."""
        refuse_guidance_rows(unconditional_guidance_scale, "DPMSolverSampler")
        general = not (order == 2 and method == "multistep" and skip_type == "time_uniform" and predict_x0 is True
                       and solver_type == "dpm_solver" and lower_order_final is True and not denoise_to_zero and not thresholding
                       and t_start is None and t_end is None)
        if general:
            check_dpm_options(S, order, method, skip_type, solver_type)
        if mask is not None or x0 is not None or eta != 0. or quantize_x0 or score_corrector is not None or noise_dropout > 0. \
                or temperature != 1.:
            raise NotImplementedError("DPM-Solver++(2M) sampling: mask / x0 / eta / quantize_x0 / score_corrector / noise_dropout / "
                                      "temperature are not implemented (the reference's DPMSolverSampler ignores them)")
        ptype = getattr(self.model, "parameterization", "eps")
        if ptype not in MODEL_TYPES:
            raise NotImplementedError(f"DPM-Solver sampling for parameterization {ptype!r}: only 'eps' is built")
        if general:
            plan = dpm_plan(self.alphas_cumprod, S, order=order, method=method, skip_type=skip_type, predict_x0=bool(predict_x0),
                            solver_type=solver_type, lower_order_final=bool(lower_order_final), denoise_to_zero=bool(denoise_to_zero),
                            t_start=t_start, t_end=t_end, thresholding=bool(thresholding), max_val=float(max_val))
            return self._sample_plan(plan, batch_size, shape, conditioning, callback, img_callback, x_T, unconditional_guidance_scale,
                                     unconditional_conditioning), None
        tb = dpm_tables(self.alphas_cumprod, S)
        C, H, W = shape
        size = (batch_size, C, H, W)
        dev = self.model.device
        self.make_schedule(S, tb)
        img = torch.randn(size, device=dev) if x_T is None else x_T.to(dev).float().clone()
        cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        uncond = unconditional_conditioning if cfg else None
        scale = float(unconditional_guidance_scale)
        if self.use_graph and callback is None and img_callback is None and hasattr(self.model, "apply_model_cfg"):
            sg = DPMStepGraph(self, img, conditioning, uncond, scale)
            sg.reset(0)
            sg.step_eager()             # packs weights and allocates every buffer before capture
            if int(S) > 1:
                with sg.stream_ctx():
                    sg.capture()
                    for _ in range(1, int(S)):
                        sg.replay()
                sg.join()
        else:
            self._sample_eager(img, conditioning, uncond, scale, int(S), callback, img_callback)
        ops.f16_guard_check("the DPM-Solver sampling loop")    # fp16 modes: raise rather than return samples computed through an inf
        return img, None

    def _sample_plan(self, plan: DPMPlan, batch_size, shape, cond, callback, img_callback, x_T, scale, uncond):
        """The general run: one row of the plan per NFE, eager or (use_graph) one captured NFE replayed for the remaining rows."""
        dev = self.model.device
        self.plan = plan
        self._rows = plan.rows.to(dev)
        self._t_table = plan.t_input.to(dev)
        size = (batch_size,) + tuple(shape)
        img = torch.randn(size, device=dev) if x_T is None else x_T.to(dev).float().clone()
        cfg = not (uncond is None or scale == 1.)
        uncond = uncond if cfg else None
        R = int(plan.rows.shape[0])
        ng = DPMPlanGraph(self, img, cond, uncond, float(scale))
        if self.use_graph and callback is None and img_callback is None and hasattr(self.model, "apply_model_cfg"):
            ng.nfe()                 # packs weights and allocates every buffer before capture
            if R > 1:
                with ng.stream_ctx():
                    ng.capture()
                    for _ in range(1, R):
                        ng.replay()
                ng.join()
        else:
            pred_x0 = torch.empty_like(img) if img_callback else None
            for i in range(R):
                ng.nfe(pred_x0=pred_x0, eager_t=float(plan.t_input[i]))
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(pred_x0, i)
        ops.f16_guard_check("the DPM-Solver sampling loop")
        return img

    def _eps(self, x, t, cond, uncond, out=None):
        """(e_c, e_u or None) at model time t (float32 [B]); model_wrapper's classifier-free branch (dpm_solver.py:305-321)."""
        m = self.model
        if hasattr(m, "apply_model_cfg"):
            if uncond is None:
                return m.apply_model(x, t, cond, out=out, uniform_t=True), None
            return m.apply_model_cfg(x, t, cond, uncond, out=out, uniform_t=True)
        e_c = m.apply_model(x, t, cond)
        return e_c, (None if uncond is None else m.apply_model(x, t, uncond))

    def _sample_eager(self, img, cond, uncond, scale, S, callback, img_callback):
        dev = img.device
        B = img.shape[0]
        x0_prev = torch.empty_like(img)
        pred_x0 = torch.empty_like(img) if img_callback else None
        steps = torch.arange(S, dtype=torch.int32, device=dev)
        for i in range(S):
            t = torch.full((B,), float(self.tables.t_input[i]), dtype=torch.float32, device=dev)
            e_c, e_u = self._eps(img, t, cond, uncond)
            ops.dpm_step(img, e_c.float().contiguous(), None if e_u is None else e_u.float().contiguous(), x0_prev, self._coefs,
                         step_idx=steps[i:i + 1], cfg_scale=scale, pred_x0=pred_x0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)


class DPMStepGraph:
    """One DPM-Solver step = {model time from the device table (stedm_step_set_t_f32), U-Net (shared-encoder CFG pass) into a
    preallocated eps, fused update in place on `img` and x0_prev (stedm_dpm_step), step index + 1}, capturable once in a hipGraph and
    replayed for every later step (the pattern of ddim.StepGraph)."""

    def __init__(self, sampler: DPMSolverSampler, img: torch.Tensor, cond, uncond, scale: float):
        self.s = sampler
        self.img = img
        self.cond, self.uncond, self.scale = cond, uncond, float(scale)
        dev = img.device
        b = img.shape[0]
        self.step = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((b,), dtype=torch.float32, device=dev)
        self.x0_prev = torch.empty_like(img)
        self.eps = torch.empty((2 * b if uncond is not None else b,) + tuple(img.shape[1:]), dtype=torch.float32, device=dev)
        self.graph = None
        self.side = None

    def reset(self, index: int):
        self.step.fill_(int(index))

    def step_eager(self):
        s = self.s
        ops.step_set_t(s._t_table, self.step, self.t_buf)
        e_c, e_u = s._eps(self.img, self.t_buf, self.cond, self.uncond, out=self.eps)
        ops.dpm_step(self.img, e_c, e_u, self.x0_prev, s._coefs, step_idx=self.step, cfg_scale=self.scale)
        ops.step_advance(self.step, 1)

    def stream_ctx(self):
        if self.side is None:
            self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.side)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.side)

    def capture(self):
        """Must be called inside stream_ctx() after at least one step_eager()."""
        g = ops.Graph()
        with g:
            self.step_eager()
        self.graph = g

    def replay(self):
        self.graph.launch()


class DPMPlanGraph:
    """One NFE of a general DPM-Solver plan = {model time from the device table (stedm_step_set_t_f32), U-Net (shared-encoder CFG pass)
    into a preallocated eps, stedm_dpm_update (split around stedm_dpm_threshold when the plan thresholds), row index + 1}. The eager loop
    runs it per row; with use_graph it is captured once and replayed for every later row, the denoise_to_zero row included. `img` is the
    U-Net input and, after the last row (which always commits), the result; the base x is `img` itself when every row commits
    (multistep), else a buffer of its own; slots [3, *img.shape] hold the model outputs the updates read."""

    def __init__(self, sampler: DPMSolverSampler, img: torch.Tensor, cond, uncond, scale: float):
        self.s = sampler
        self.img = img
        self.cond, self.uncond, self.scale = cond, uncond, float(scale)
        plan = sampler.plan
        dev = img.device
        b = img.shape[0]
        self.base = img if all(plan.commits) else img.clone()
        self.slots = torch.empty((3,) + tuple(img.shape), dtype=torch.float32, device=dev)
        self.step = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((b,), dtype=torch.float32, device=dev)
        self.eps = torch.empty((2 * b if uncond is not None else b,) + tuple(img.shape[1:]), dtype=torch.float32, device=dev)
        self.threshold, self.max_val = plan.threshold, plan.max_val
        self.graph = None
        self.side = None

    def reset(self, index: int):
        self.step.fill_(int(index))

    def nfe(self, pred_x0=None, eager_t=None):
        s = self.s
        if eager_t is None:
            ops.step_set_t(s._t_table, self.step, self.t_buf)
            e_c, e_u = s._eps(self.img, self.t_buf, self.cond, self.uncond, out=self.eps)
        else:                        # the eager loop: the model time as a host value (any model surface)
            t = torch.full((self.img.shape[0],), eager_t, dtype=torch.float32, device=self.img.device)
            e_c, e_u = s._eps(self.img, t, self.cond, self.uncond)
            e_c = e_c.float().contiguous()
            e_u = None if e_u is None else e_u.float().contiguous()
        rows, step = s._rows, self.step
        if self.threshold:
            ops.dpm_update(self.img, self.base, e_c, e_u, self.slots, rows, step_idx=step, cfg_scale=self.scale, mode=ops.DPMU_MODEL)
            ops.dpm_threshold(self.slots, self.max_val, rows=rows, step_idx=step)
            ops.dpm_update(self.img, self.base, None, None, self.slots, rows, step_idx=step, mode=ops.DPMU_COMBINE, pred_x0=pred_x0)
        else:
            ops.dpm_update(self.img, self.base, e_c, e_u, self.slots, rows, step_idx=step, cfg_scale=self.scale, pred_x0=pred_x0)
        ops.step_advance(self.step, 1)

    def stream_ctx(self):
        if self.side is None:
            self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.side)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.side)

    def capture(self):
        """Must be called inside stream_ctx() after at least one nfe()."""
        g = ops.Graph()
        with g:
            self.nfe()
        self.graph = g

    def replay(self):
        self.graph.launch()
