#!/usr/bin/env python3
"""F18: DPM-Solver++(2M) sampling through the REFERENCE's own `DPMSolverSampler` (ldm/models/diffusion/dpm_solver/sampler.py:12-95:
multistep, order 2, predict_x0, skip_type 'time_uniform', lower_order_final) with a closed-form `Toy` eps model. `ddpm.py` is not
importable here (it needs torchvision), so `Toy` carries what the sampler reads of the model: the fp32 betas / alphas_cumprod buffers as
register_schedule builds them (ddpm.py:120-172), parameterization 'eps', a CPU device, and an `apply_model(x, t, c)` that depends on the
fractional model time t. Every model call's (x, t) is recorded.

Cases (B = 2, latents 4 x 8 x 8; the same x_T):
  s20: S = 20, CFG 1.5 (second order to the end);
  s5:  S = 5, no CFG (first-order final step, lower_order_final with S < 15);
  s2:  S = 2, no CFG.
Stored per case: the model time of every call (<case>_t [S], all rows equal), every call's input x (<case>_call_x [S, B, 4, 8, 8], the
first B rows: the CFG batch is [x, x]) and the final x (<case>_out).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dpm.py
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
SEED = 18
SHAPE = (2, 4, 8, 8)
CASES = (("s20", 20, 1.5), ("s5", 5, 1.0), ("s2", 2, 1.0))


def toy_eps(x: torch.Tensor, t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The closed-form eps model (torch, any device); the sin(t) term makes it depend on the fraction of t."""
    tf = t.float()[:, None, None, None]
    u = tf / 1000.0
    return torch.tanh(x * (0.5 + u) + bias) * (0.8 + 0.3 * u) + 0.1 * bias + 0.05 * torch.sin(tf)


def main():
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler
    from ldm.modules.diffusionmodules import util as rutil

    betas = rutil.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)

    class Toy:
        """Duck-typed model surface DPMSolverSampler reads (sampler.py:16-17, 79, 84-90)."""
        def __init__(self):
            self.num_timesteps = 1000
            self.betas = f32(betas)
            self.alphas_cumprod = f32(ac)
            self.parameterization = "eps"
            self.device = torch.device("cpu")
            self.calls = []

        def apply_model(self, x, t, c):
            self.calls.append((x.clone(), t.clone()))
            return toy_eps(x, t, c["bias"])

    xT = prng.normal(SEED, "dpm.xT", SHAPE)
    cond = {"bias": prng.normal(SEED, "dpm.c", SHAPE) * 0.3}
    unc = {"bias": prng.normal(SEED, "dpm.u", SHAPE) * 0.3}
    out = {"xT": xT.numpy(), "cond": cond["bias"].numpy(), "uncond": unc["bias"].numpy(), "alphas_cumprod": f32(ac).numpy()}
    B = SHAPE[0]
    for name, S, scale in CASES:
        toy = Toy()
        kw = dict(unconditional_guidance_scale=scale, unconditional_conditioning=unc) if scale != 1.0 else {}
        x, none = DPMSolverSampler(toy, device=torch.device("cpu")).sample(S, B, SHAPE[1:], cond, verbose=False, x_T=xT.clone(), **kw)
        assert none is None and len(toy.calls) == S, (name, len(toy.calls))
        ts = []
        for cx, ct in toy.calls:
            assert ct.dtype == torch.float32 and bool((ct == ct[0]).all()), ct
            assert cx.shape[0] == (2 * B if scale != 1.0 else B)
            ts.append(float(ct[0]))
        out[f"{name}_S"] = np.int64(S)
        out[f"{name}_scale"] = np.float32(scale)
        out[f"{name}_t"] = np.array(ts, dtype=np.float32)
        out[f"{name}_call_x"] = torch.stack([cx[:B] for cx, _ in toy.calls]).numpy()
        out[f"{name}_out"] = x.numpy()

    path = os.path.join(HERE, "f18_dpm_solver.npz")
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f18_dpm_solver.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
