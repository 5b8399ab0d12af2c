"""Host-side (numpy) noise schedule and DDIM tables — the reference also builds these on the host
once per `sample()` call (ddim.py:24-53; util.py:21-74; ddpm.py:120-172). Written from the formulas,
with the reference's precision staging reproduced explicitly:

  betas            f64: linspace(sqrt(l0), sqrt(l1), T)**2                    (util.py:23-25)
  alphas_cumprod   f64 cumprod, then narrowed to the fp32 buffer               (ddpm.py:127-141)
  ddim tables      computed FROM the fp32 buffer (ddim.py:27-33,43-49): a_t = acp32[ts];
                   a_prev = [acp32[0]] + acp32[ts[:-1]];  (1 - a_t), 1/(1 - a_t) and sqrt(1 - a_t) evaluated
                   in fp32, the rest of the sigma formula in f64; all four per-step scalars reach the
                   device as fp32 (torch.full, ddim.py:195-198).
Bit-checked against the reference's own outputs in tests/test_host_logic.py (golden F2).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


def make_beta_schedule(n_timestep: int = 1000, linear_start: float = 1e-4, linear_end: float = 2e-2,
                       schedule: str = "linear") -> np.ndarray:
    if schedule != "linear":
        raise NotImplementedError(f"beta schedule {schedule!r}: only 'linear' is used by the reference configs")
    import torch  # host-side f64 linspace, the very call of util.py:23-25 (bit-exactness of the table matters)
    lin = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64).numpy()
    return lin ** 2


@dataclass
class NoiseSchedule:
    """The fp32 buffers of DDPM.register_schedule (ddpm.py:120-172) that the hot path reads."""
    num_timesteps: int
    betas: np.ndarray                        # f32
    alphas_cumprod: np.ndarray               # f32
    alphas_cumprod_prev: np.ndarray          # f32
    sqrt_alphas_cumprod: np.ndarray          # f32
    sqrt_one_minus_alphas_cumprod: np.ndarray  # f32

    @staticmethod
    def make(timesteps: int = 1000, linear_start: float = 1e-4, linear_end: float = 2e-2,
             beta_schedule: str = "linear") -> "NoiseSchedule":
        betas = make_beta_schedule(timesteps, linear_start, linear_end, beta_schedule)
        ac = np.cumprod(1.0 - betas, axis=0)
        ac_prev = np.append(1.0, ac[:-1])
        f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
        return NoiseSchedule(int(timesteps), f32(betas), f32(ac), f32(ac_prev), f32(np.sqrt(ac)), f32(np.sqrt(1.0 - ac)))


def make_ddim_timesteps(num_ddim_timesteps: int, num_ddpm_timesteps: int = 1000, method: str = "uniform") -> np.ndarray:
    """util.py:46-60 — integer arithmetic, must be exact: c = T // S; ts = arange(0, T, c) + 1."""
    if method != "uniform":
        raise NotImplementedError("only the 'uniform' DDIM discretisation is used by the reference")
    c = num_ddpm_timesteps // num_ddim_timesteps
    return np.arange(0, num_ddpm_timesteps, c, dtype=np.int64) + 1


@dataclass
class DDIMTables:
    timesteps: np.ndarray   # int64 [n], ascending (ddim_timesteps)
    alphas: np.ndarray      # f32 [n]
    alphas_prev: np.ndarray  # f32 [n]
    sigmas: np.ndarray      # f32 [n]
    sqrt_one_minus_alphas: np.ndarray  # f32 [n]

    def coef_table(self) -> np.ndarray:
        """[n][4] fp32 rows {a_t, a_prev, sigma_t, sqrt(1 - a_t)} — the device table of stedm_ddim_step."""
        return np.stack([self.alphas, self.alphas_prev, self.sigmas, self.sqrt_one_minus_alphas], axis=1).astype(np.float32)


def make_ddim_tables(alphas_cumprod_f32: np.ndarray, S: int, eta: float = 0.0) -> DDIMTables:
    ts = make_ddim_timesteps(S, alphas_cumprod_f32.shape[0])
    acp = np.asarray(alphas_cumprod_f32, dtype=np.float32)
    a32 = acp[ts]                                                    # f32
    ap64 = np.concatenate([acp[:1], acp[ts[:-1]]]).astype(np.float64)  # f32 values held in f64
    one_minus_a = (np.float32(1.0) - a32)                            # evaluated in fp32 (torch f32 tensor op)
    ratio = a32.astype(np.float64) / ap64                            # f32 tensor / f64 array -> f64
    # ndarray / Tensor dispatches to Tensor.__rtruediv__ = reciprocal(fp32) * other: the reciprocal is rounded in fp32
    recip32 = (np.float32(1.0) / one_minus_a).astype(np.float64)
    sig64 = eta * np.sqrt(recip32 * (1.0 - ap64) * (1.0 - ratio))
    sq32 = np.sqrt(one_minus_a).astype(np.float32)                   # np.sqrt on the f32 tensor (ddim.py:49)
    return DDIMTables(ts, a32, ap64.astype(np.float32), sig64.astype(np.float32), sq32)


# ------------------------------------------------------------------------------------------------ ancestral (DDPM) sampling
POSTERIOR_BUFFERS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
                     "posterior_mean_coef1", "posterior_mean_coef2", "log_one_minus_alphas_cumprod")


@dataclass
class PosteriorSchedule:
    """The fp32 buffers of DDPM.register_schedule (ddpm.py:147-163) that the ancestral sampler reads (p_mean_variance / q_posterior,
    ddpm.py:219-232, 1050-1080): each evaluated in f64 numpy from the f64 betas, then narrowed to fp32 as `to_torch` does."""
    sqrt_recip_alphas_cumprod: np.ndarray       # f32 sqrt(1 / a)
    sqrt_recipm1_alphas_cumprod: np.ndarray     # f32 sqrt(1 / a - 1)
    posterior_variance: np.ndarray              # f32 (1 - v) b (1 - a_prev) / (1 - a) + v b
    posterior_log_variance_clipped: np.ndarray  # f32 log(max(posterior_variance, 1e-20))
    posterior_mean_coef1: np.ndarray            # f32 b sqrt(a_prev) / (1 - a)
    posterior_mean_coef2: np.ndarray            # f32 (1 - a_prev) sqrt(1 - b) / (1 - a)
    log_one_minus_alphas_cumprod: np.ndarray    # f32 log(1 - a)

    @staticmethod
    def make(timesteps: int = 1000, linear_start: float = 1e-4, linear_end: float = 2e-2, beta_schedule: str = "linear",
             v_posterior: float = 0.0) -> "PosteriorSchedule":
        betas = make_beta_schedule(timesteps, linear_start, linear_end, beta_schedule)
        alphas = 1. - betas
        ac = np.cumprod(alphas, axis=0)
        ac_prev = np.append(1., ac[:-1])
        f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
        pv = (1 - v_posterior) * betas * (1. - ac_prev) / (1. - ac) + v_posterior * betas       # ddpm.py:156-157, in its order
        return PosteriorSchedule(f32(np.sqrt(1. / ac)), f32(np.sqrt(1. / ac - 1)), f32(pv), f32(np.log(np.maximum(pv, 1e-20))),
                                 f32(betas * np.sqrt(ac_prev) / (1. - ac)), f32((1. - ac_prev) * np.sqrt(alphas) / (1. - ac)),
                                 f32(np.log(1. - ac)))


def ddpm_step_table(sqrt_recip, sqrt_recipm1, coef1, coef2, log_var_clipped) -> np.ndarray:
    """[T][5] fp32 rows {sr, srm1, c1, c2, sigma} of stedm_ddpm_step, from the fp32 buffers (numpy or CPU tensors). sigma_t =
    nonzero(t) exp(0.5 logvar_clipped[t]) is evaluated with torch's fp32 exp on the CPU, the expression of p_sample (ddpm.py:1100-1110),
    so that sigma_t * noise rounds as the reference's `nonzero_mask * (0.5 * model_log_variance).exp() * noise`; sigma_0 = 0."""
    import torch
    as32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    lv = as32(log_var_clipped)
    sigma = (0.5 * lv).exp()
    sigma[0] = 0.0
    cols = [as32(sqrt_recip), as32(sqrt_recipm1), as32(coef1), as32(coef2), sigma]
    return torch.stack(cols, dim=1).numpy().astype(np.float32)


# ------------------------------------------------------------------------------------------------ training objective
def lvlb_weights(timesteps: int = 1000, linear_start: float = 1e-4, linear_end: float = 2e-2, beta_schedule: str = "linear",
                 v_posterior: float = 0.0) -> np.ndarray:
    """`lvlb_weights` of DDPM.register_schedule for eps-parameterisation (ddpm.py:162-172), the weight of the variational-bound term of
    p_losses (ddpm.py:1042-1045): betas^2 / (2 posterior_variance alphas (1 - alphas_cumprod)), evaluated from the fp32 buffers with the
    reference's own fp32 torch expression in its order (every product and the quotient round in fp32), then entry 0 — where the posterior
    variance is 0 — takes entry 1's value. fp32 [T]."""
    import torch
    betas64 = make_beta_schedule(timesteps, linear_start, linear_end, beta_schedule)
    ns = NoiseSchedule.make(timesteps, linear_start, linear_end, beta_schedule)
    ps = PosteriorSchedule.make(timesteps, linear_start, linear_end, beta_schedule, v_posterior=v_posterior)
    betas = torch.from_numpy(ns.betas.copy())
    pv = torch.from_numpy(ps.posterior_variance.copy())
    alphas = torch.tensor(1. - betas64, dtype=torch.float32)
    ac = torch.from_numpy(ns.alphas_cumprod.copy())
    w = betas ** 2 / (2 * pv * alphas * (1 - ac))
    w[0] = w[1]
    return w.numpy().astype(np.float32)
