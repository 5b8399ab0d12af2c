#!/usr/bin/env python3
"""F19: PLMS sampling through the REFERENCE's own `PLMSSampler` (ldm/models/diffusion/plms.py:11-239) under a register_buffer override
for the CPU, with a closed-form `Toy` eps model. `ddpm.py` is not importable here (it needs torchvision), so `Toy` carries what the sampler
reads of the model: the fp32 schedule buffers as register_schedule builds them (ddpm.py:120-172), a CPU device, an `apply_model(x, t, c)`
and, for the masked case, a `q_sample(x0, t, noise=None)` with the body of ddpm.py:277-280 whose noise is drawn from a recorded stream.
The conditioning is a plain tensor: the reference's CFG batch is torch.cat([unconditional_conditioning, c]) (plms.py:184), which a dict
cannot pass through. Every model call's (x, t) is recorded.

Cases (B = 2, latents 4 x 8 x 8; the same x_T):
  s20c: S = 20, CFG 1.5 (reaches the 4th-order update), log_every_t = 5 (the indices of the logged iterations stored);
  s4:   S = 4, no CFG (iterations at t = 751, 501, 251, 1: the Euler / Heun first step and orders 1, 2, 3 once each);
  s1:   S = 1, no CFG (one iteration, t_next == t);
  m10:  S = 10, CFG 1.5, binary mask [2, 1, 8, 8] with x0; q_sample's noise of its k-th call is q_noise(k) (not stored: the tests
        rebuild it from the same recipe, and every blended call input pins it).
(S = 3 is not a case: its stride reaches t = 1000, out of range in the reference too.)
Stored per case: every call's timestep (<case>_t [n + 1]), every call's input x (<case>_call_x [n + 1, B, 4, 8, 8], the first B rows: the
CFG batch is [x, x]) and the final x (<case>_out). The fixture stays under 100 KB: x_inter is not stored, its entries are x_T, call inputs
and the final x (s20c_log_iters: the iterations whose result is logged; checked against the reference's intermediates here).
The stored bits depend on the machine that ran this script: the toy model's tanh (and so every later value) can round differently by an
ulp on another CPU or libm build, which the loop carries to ~2e-7 of the largest value. tests/test_plms_oracle.py therefore pins F19
within a tolerance and compares bit for bit only loops it computes itself.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plms.py
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
SEED = 19
SHAPE = (2, 4, 8, 8)
CASES = (("s20c", 20, 1.5, False), ("s4", 4, 1.0, False), ("s1", 1, 1.0, False), ("m10", 10, 1.5, True))


def toy_eps(x: torch.Tensor, t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The closed-form eps model of F10 / F17 (torch, any device)."""
    tf = t.float()[:, None, None, None] / 1000.0
    return torch.tanh(x * (0.5 + tf) + bias) * (0.8 + 0.3 * tf) + 0.1 * bias


def q_noise(k: int) -> torch.Tensor:
    """The noise of m10's k-th q_sample call."""
    return prng.normal(SEED, f"plms.m10.q{k}", SHAPE)


def main():
    import ldm.models.diffusion.plms as rplms
    from ldm.modules.diffusionmodules import util as rutil

    betas = rutil.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)

    class CPUSampler(rplms.PLMSSampler):
        def register_buffer(self, name, attr):  # harness override: the original pins "cuda" (plms.py:18-22)
            setattr(self, name, attr)

    class Toy:
        """Duck-typed model surface the PLMS sampler reads (plms.py:15, 29-35, 121, 149, 180-185)."""
        def __init__(self, tag):
            self.tag = tag
            self.num_timesteps = 1000
            self.betas = f32(betas)
            self.alphas_cumprod = f32(ac)
            self.alphas_cumprod_prev = f32(np.append(1.0, ac[:-1]))
            self.sqrt_alphas_cumprod = f32(np.sqrt(ac))                    # ddpm.py:155-156
            self.sqrt_one_minus_alphas_cumprod = f32(np.sqrt(1.0 - ac))
            self.device = torch.device("cpu")
            self.calls = []
            self.q_noises = []

        def apply_model(self, x, t, c):
            self.calls.append((x.clone(), t.clone()))
            return toy_eps(x, t, c)

        def q_sample(self, x_start, t, noise=None):
            if noise is None:
                assert self.tag == "m10" and tuple(x_start.shape) == SHAPE
                noise = q_noise(len(self.q_noises))
            self.q_noises.append(noise.clone())
            return (rutil.extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                    rutil.extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    xT = prng.normal(SEED, "plms.xT", SHAPE)
    x0 = prng.normal(SEED, "plms.x0", SHAPE)
    cond = prng.normal(SEED, "plms.c", SHAPE) * 0.3
    unc = prng.normal(SEED, "plms.u", SHAPE) * 0.3
    mask = (prng.uniform(SEED, "plms.mask", (2, 1, 8, 8)) > 0).float()
    out = {"xT": xT.numpy(), "x0": x0.numpy(), "cond": cond.numpy(), "uncond": unc.numpy(), "mask": mask.numpy()}
    B = SHAPE[0]
    for name, S, scale, masked in CASES:
        toy = Toy(name)
        kw = dict(unconditional_guidance_scale=scale, unconditional_conditioning=unc) if scale != 1.0 else {}
        if masked:
            kw.update(mask=mask, x0=x0)
        log_every_t = 5 if name == "s20c" else 100
        x, inter = CPUSampler(toy).sample(S, B, SHAPE[1:], cond, verbose=False, x_T=xT.clone(), log_every_t=log_every_t, **kw)
        ts = []
        for cx, ct in toy.calls:
            assert ct.dtype == torch.int64 and bool((ct == ct[0]).all()), ct
            assert cx.shape[0] == (2 * B if scale != 1.0 else B)
            ts.append(int(ct[0]))
        out[f"{name}_S"] = np.int64(S)
        out[f"{name}_scale"] = np.float32(scale)
        out[f"{name}_t"] = np.array(ts, dtype=np.int64)
        out[f"{name}_call_x"] = torch.stack([cx[:B] for cx, _ in toy.calls]).numpy()
        out[f"{name}_out"] = x.numpy()
        if masked:
            assert len(toy.q_noises) == len(ts) - 1
        if name == "s20c":
            # x_inter = [x_T] + the results of the logged iterations; the result of iteration i (< n - 1) is the next iteration's first
            # call input (calls 0, 1 are iteration 0's, call i + 1 is iteration i's), the last one the final x
            n = len(ts) - 1
            logged = [i for i in range(n) if (n - 1 - i) % log_every_t == 0 or i == 0]
            res = lambda i: x if i == n - 1 else toy.calls[i + 2][0][:B]
            assert len(inter["x_inter"]) == len(logged) + 1 and torch.equal(inter["x_inter"][0], xT)
            assert all(torch.equal(a, res(i)) for a, i in zip(inter["x_inter"][1:], logged))
            out[f"{name}_log_iters"] = np.array(logged, dtype=np.int64)

    path = os.path.join(HERE, "f19_plms.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f19_plms.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
