#!/usr/bin/env python3
"""F22: the general DPM-Solver (orders 1-3, multistep / singlestep / singlestep_fixed, noise and data prediction, both solver types,
three time spacings, denoise_to_zero, t_start / t_end, dynamic thresholding) through the REFERENCE's own `DPM_Solver`,
`NoiseScheduleVP('discrete')` and `model_wrapper` (ldm/models/diffusion/dpm_solver/dpm_solver.py) with F18's closed-form eps model.

Two deviations from the reference are patched in, only where the reference cannot run at all. First, with order 3, lower_order_final and
steps < 15 its multistep loop hands its 3-entry model list to `multistep_dpm_solver_second_update`, which unpacks two names and raises
(ValueError: too many values to unpack). The patch passes the last two entries (model_prev_list[-2:], t_prev_list[-2:]), the fix later
DPM-Solver releases carry. Likewise its singlestep time grid calls `torch.cumsum(orders)` without the `dim` this torch requires (a
TypeError); the generator supplies dim=0, as later releases write it. Everything else runs the reference untouched.

Cases (B = 2, latents 4 x 8 x 8; one x_T): see CASES. Stored per case: <case>_t, the model time of every call [R] (all rows of a call
equal), <case>_out, the final x, and for a few cases <case>_call_x [R, B, 4, 8, 8], every call's input (the first B rows: the CFG batch
is [x, x]).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dpm_general.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("STEDM_REFERENCE", "/root/reference"))

from stedm_amd.utils import prng  # noqa: E402

torch.set_grad_enabled(False)
SEED = 22
SHAPE = (2, 4, 8, 8)
# name: (steps, CFG scale, DPM_Solver.sample / constructor keywords, record every call's x)
CASES = {
    "ms1_s6": (6, 1.0, dict(order=1, method="multistep"), False),
    "ms3_cfg_s20": (20, 1.5, dict(order=3, method="multistep"), True),
    "ms3_s8": (8, 1.0, dict(order=3, method="multistep"), False),
    "ms3_noise_s10": (10, 1.0, dict(order=3, method="multistep", predict_x0=False), False),
    "ms2_taylor_s12": (12, 1.0, dict(order=2, method="multistep", solver_type="taylor", lower_order_final=False), False),
    "ss3_logsnr_s9": (9, 1.0, dict(order=3, method="singlestep", skip_type="logSNR"), True),
    "ss3_noise_s10": (10, 1.0, dict(order=3, method="singlestep", predict_x0=False), True),
    "ss3_s11": (11, 1.0, dict(order=3, method="singlestep"), False),
    "ss3_taylor_cfg_s9": (9, 1.5, dict(order=3, method="singlestep", solver_type="taylor"), False),
    "ss2_noise_taylor_s7": (7, 1.0, dict(order=2, method="singlestep", predict_x0=False, solver_type="taylor"), False),
    "ssfixed3_quad_s9": (9, 1.0, dict(order=3, method="singlestep_fixed", skip_type="time_quadratic"), False),
    "thr_ms2_cfg_s10": (10, 1.5, dict(order=2, method="multistep", thresholding=True, max_val=0.5), True),
    "thr_ss3_s10": (10, 1.0, dict(order=3, method="singlestep", thresholding=True, max_val=0.5), False),
    "d2z_ms2_s8": (8, 1.0, dict(order=2, method="multistep", denoise_to_zero=True), False),
    "d2z_noise_thr_s8": (8, 1.0, dict(order=2, method="multistep", predict_x0=False, thresholding=True, max_val=0.5,
                                      denoise_to_zero=True), True),
    "tse_ms3_s16": (16, 1.0, dict(order=3, method="multistep", t_start=0.8, t_end=0.01), False),
}
SOLVER_KEYS = ("predict_x0", "thresholding", "max_val")


def toy_eps(x: torch.Tensor, t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """F18's closed-form eps model (make_golden_dpm.py); the sin(t) term makes it depend on the fraction of t."""
    tf = t.float()[:, None, None, None]
    u = tf / 1000.0
    return torch.tanh(x * (0.5 + u) + bias) * (0.8 + 0.3 * u) + 0.1 * bias + 0.05 * torch.sin(tf)


def main():
    from ldm.models.diffusion.dpm_solver import dpm_solver as rdpm
    from ldm.modules.diffusionmodules import util as rutil

    second = rdpm.DPM_Solver.multistep_dpm_solver_second_update

    def second_last_two(self, x, model_prev_list, t_prev_list, t, solver_type="dpm_solver"):
        return second(self, x, model_prev_list[-2:], t_prev_list[-2:], t, solver_type=solver_type)

    rdpm.DPM_Solver.multistep_dpm_solver_second_update = second_last_two
    cumsum = torch.cumsum
    torch.cumsum = lambda input, dim=0, **kw: cumsum(input, dim, **kw)

    betas = rutil.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205)
    ac = torch.tensor(np.cumprod(1.0 - betas, axis=0), dtype=torch.float32)
    xT = prng.normal(SEED, "dpmg.xT", SHAPE)
    cond = {"bias": prng.normal(SEED, "dpmg.c", SHAPE) * 0.3}
    unc = {"bias": prng.normal(SEED, "dpmg.u", SHAPE) * 0.3}
    out = {"xT": xT.numpy(), "cond": cond["bias"].numpy(), "uncond": unc["bias"].numpy(), "alphas_cumprod": ac.numpy()}
    B = SHAPE[0]
    for name, (S, scale, kw, rec) in CASES.items():
        calls = []

        def model(x, t, c):
            calls.append((x.clone(), t.clone()))
            return toy_eps(x, t, c["bias"])

        ns = rdpm.NoiseScheduleVP("discrete", alphas_cumprod=ac)
        fn = rdpm.model_wrapper(model, ns, model_type="noise", guidance_type="classifier-free", condition=cond,
                                unconditional_condition=unc if scale != 1.0 else None, guidance_scale=scale)
        skw = {k: kw[k] for k in SOLVER_KEYS if k in kw}
        solver = rdpm.DPM_Solver(fn, ns, predict_x0=skw.pop("predict_x0", True), **skw)
        x = solver.sample(xT.clone(), steps=S, **{k: v for k, v in kw.items() if k not in SOLVER_KEYS})
        ts = []
        for cx, ct in calls:
            assert ct.dtype == torch.float32 and bool((ct == ct[0]).all()), ct
            assert cx.shape[0] == (2 * B if scale != 1.0 else B)
            ts.append(float(ct[0]))
        out[f"{name}_t"] = np.array(ts, dtype=np.float32)
        if rec:
            out[f"{name}_call_x"] = torch.stack([cx[:B] for cx, _ in calls]).numpy()
        out[f"{name}_out"] = x.numpy()
        print(f"{name}: {len(calls)} calls")

    path = os.path.join(HERE, "f22_dpm_general.npz")
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f22_dpm_general.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
