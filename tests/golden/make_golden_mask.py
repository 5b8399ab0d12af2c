#!/usr/bin/env python3
"""F17: masked DDIM sampling (mask / x0) through the REFERENCE's own `DDIMSampler` (ldm/models/diffusion/ddim.py:113-162, the blend of
:143-146) under the CPUSampler override of F10 (make_golden.py), with the closed-form `Toy` eps model. `ddpm.py` is not importable here
(it needs torchvision), so `Toy` carries what the masked loop reads of the model: the fp32 schedule buffers as register_schedule builds them
(ddpm.py:120-172) and a `q_sample(x0, t, noise=None)` with the body of ddpm.py:277-280 over the reference's extract_into_tensor. Every noise
the loop draws is recorded and stored, so that a loop fed the same noises must reproduce the outputs:
  * q_sample's noise (one draw per step, ddim.py:145),
  * the step noise of p_sample_ddim (ddim.py:206, through `noise_like`, patched for the duration).

Cases (B = 2, latents 4 x 8 x 8):
  a) S = 20, eta = 0, CFG 1.5 (rescale phi 0.7), binary mask [2, 1, 8, 8], log_every_t = 5 (x_inter stack stored);
  b) S = 10, eta = 1, no CFG, soft mask [1, 4, 8, 8].

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mask.py
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
SEED = 17
SHAPE = (2, 4, 8, 8)


def main():
    import ldm.models.diffusion.ddim as rddim
    from ldm.modules.diffusionmodules import util as rutil

    betas = rutil.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)

    class CPUSampler(rddim.DDIMSampler):
        def register_buffer(self, name, attr):  # harness override: the original pins "cuda" (ddim.py:18-22)
            setattr(self, name, attr)

    class Toy:
        """Duck-typed model surface the masked sampler reads (ddim.py:15, 27-33, 119, 145)."""
        def __init__(self, tag):
            self.tag = tag
            self.num_timesteps = 1000
            self.betas = f32(betas)
            self.alphas_cumprod = f32(ac)
            self.alphas_cumprod_prev = f32(np.append(1.0, ac[:-1]))
            self.sqrt_alphas_cumprod = f32(np.sqrt(ac))                    # ddpm.py:155-156
            self.sqrt_one_minus_alphas_cumprod = f32(np.sqrt(1.0 - ac))
            self.device = torch.device("cpu")
            self.calls = 0
            self.q_noises = []

        def apply_model(self, x, t, c):
            self.calls += 1
            tf = t.float()[:, None, None, None] / 1000.0
            return torch.tanh(x * (0.5 + tf) + c["bias"]) * (0.8 + 0.3 * tf) + 0.1 * c["bias"]

        def q_sample(self, x_start, t, noise=None):
            if noise is None:
                noise = prng.normal(SEED, f"mask.{self.tag}.q{len(self.q_noises)}", x_start.shape)
            self.q_noises.append(noise.clone())
            return (rutil.extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start +
                    rutil.extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    step_noises = []

    def noise_like(shape, device, repeat=False):
        assert not repeat
        n = prng.normal(SEED, f"mask.step{len(step_noises)}", shape)
        step_noises.append(n.clone())
        return n

    orig_noise_like = rddim.noise_like
    rddim.noise_like = noise_like
    try:
        xT = prng.normal(SEED, "mask.xT", SHAPE)
        x0 = prng.normal(SEED, "mask.x0", SHAPE)
        cond = {"bias": prng.normal(SEED, "mask.c", SHAPE) * 0.3}
        unc = {"bias": prng.normal(SEED, "mask.u", SHAPE) * 0.3}
        out = {"xT": xT.numpy(), "x0": x0.numpy(), "cond": cond["bias"].numpy(), "uncond": unc["bias"].numpy()}

        # a) binary per-sample mask, eta 0, CFG
        mask_a = (prng.uniform(SEED, "mask.a", (2, 1, 8, 8)) > 0).float()
        toy = Toy("a")
        s, inter = CPUSampler(toy).sample(20, 2, SHAPE[1:], cond, verbose=False, eta=0.0, x_T=xT, mask=mask_a, x0=x0, log_every_t=5,
                                          unconditional_guidance_scale=1.5, unconditional_conditioning=unc)
        out.update(a_mask=mask_a.numpy(), a_out=s.numpy(), a_calls=np.int64(toy.calls),
                   a_q_noises=torch.stack(toy.q_noises).numpy(), a_x_inter=torch.stack(inter["x_inter"]).numpy())

        # b) soft mask shared by the batch, eta 1, no CFG
        step_noises.clear()
        mask_b = prng.uniform(SEED, "mask.b", (1, 4, 8, 8), lo=0.0, hi=1.0)
        toy = Toy("b")
        s, _ = CPUSampler(toy).sample(10, 2, SHAPE[1:], cond, verbose=False, eta=1.0, x_T=xT, mask=mask_b, x0=x0)
        out.update(b_mask=mask_b.numpy(), b_out=s.numpy(), b_calls=np.int64(toy.calls),
                   b_q_noises=torch.stack(toy.q_noises).numpy(), b_step_noises=torch.stack(step_noises).numpy())
    finally:
        rddim.noise_like = orig_noise_like

    path = os.path.join(HERE, "f17_ddim_mask.npz")
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f17_ddim_mask.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
