#!/usr/bin/env python3
"""F24: the training objective through the REFERENCE's own code: `DDPM.register_schedule`, `DDPM.get_loss`, `DDPM.q_sample` and
`LatentDiffusion.p_losses` (ldm/models/diffusion/ddpm.py:120-172, 277-295, 1015-1048), called on a duck-typed `Toy` self that carries
the attributes they read (parameterization 'eps', v_posterior 0, loss_type, l_simple_weight, original_elbo_weight, learn_logvar, logvar,
training, device, the buffers register_schedule writes) and the closed-form `apply_model` of F10 / F19 / F20. The imports ddpm.py makes
but this fixture does not need are stubbed as in make_golden_ddpm.py (this script only).

`apply_model` hands p_losses a leaf tensor (the toy model's output, detached, requires_grad), and `logvar` is a leaf in every case — the
arithmetic p_losses runs does not depend on whether it is a buffer or a parameter — so torch autograd over the reference's own graph gives
dloss/dmodel_output and dloss/dlogvar.

Contents (STEDM schedule: linear 0.0015 .. 0.0205, T = 1000; B = 4, sample shape [4, 6, 5]: n = 120; t = [0, 999, 417, 417]: both ends —
lvlb_weights[0] is the patched entry — and a duplicate):
  lvlb_weights [1000] fp32, t, x_start, noise, cond (shared by the cases), and per case <c> in CASES:
  <c>_model_output, <c>_target [4, 4, 6, 5]; <c>_loss_simple, <c>_loss_vlb, <c>_loss (the loss_dict values 'train/...'), <c>_loss_gamma and
  <c>_logvar_mean when learn_logvar; <c>_d_model_output [4, 4, 6, 5], <c>_d_logvar [1000]; <c>_cfg = (kind: 0 l1 / 1 l2, l_simple_weight,
  original_elbo_weight, logvar_init, learn_logvar) as float64.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objective.py
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
from tests.golden.make_golden_ddpm import _stub_imports, toy_eps  # noqa: E402

SEED = 24
SHAPE = (4, 4, 6, 5)
T_STEPS = (0, 999, 417, 417)
# (name, loss_type, l_simple_weight, original_elbo_weight, logvar_init, learn_logvar)
CASES = (("l1_default", "l1", 1.0, 0.0, 0.0, False),
         ("l2_default", "l2", 1.0, 0.0, 0.0, False),
         ("l2_elbo", "l2", 1.0, 0.5, 0.0, False),
         ("l1_weighted", "l1", 0.25, 0.0, -0.7, False),
         ("l2_learned", "l2", 1.0, 1e-3, 0.3, True))


def main():
    torch.set_grad_enabled(True)          # (make_golden_ddpm switches autograd off when imported)
    _stub_imports()
    import ldm.models.diffusion.ddpm as rddpm

    class Toy:
        """The reference's DDPM / LatentDiffusion functions over a duck-typed self."""
        register_schedule = rddpm.DDPM.register_schedule
        q_sample = rddpm.DDPM.q_sample
        get_loss = rddpm.DDPM.get_loss
        p_losses = rddpm.LatentDiffusion.p_losses
        training = True
        device = torch.device("cpu")

        def __init__(self, loss_type, lsw, ew, logvar_init, learn):
            self.parameterization = "eps"
            self.v_posterior = 0.
            self.loss_type, self.l_simple_weight, self.original_elbo_weight, self.learn_logvar = loss_type, lsw, ew, learn
            self.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.0015, linear_end=0.0205)
            self.logvar = torch.full(fill_value=logvar_init, size=(self.num_timesteps,)).requires_grad_(True)      # ddpm.py:115-117

        def register_buffer(self, name, value, persistent=True):
            setattr(self, name, value)

        def apply_model(self, x, t, c, return_ids=False):
            self.model_output = toy_eps(x, t, c).detach().requires_grad_(True)
            return self.model_output

    x_start = prng.normal(SEED, "obj.x0", SHAPE)
    noise = prng.normal(SEED, "obj.noise", SHAPE)
    cond = prng.normal(SEED, "obj.c", SHAPE) * 0.3
    t = torch.tensor(T_STEPS, dtype=torch.long)
    out = {"t": t.numpy(), "x_start": x_start.numpy(), "noise": noise.numpy(), "cond": cond.numpy()}
    for name, loss_type, lsw, ew, lv0, learn in CASES:
        toy = Toy(loss_type, lsw, ew, lv0, learn)
        if "lvlb_weights" not in out:
            assert toy.lvlb_weights.dtype == torch.float32 and toy.lvlb_weights.shape == (1000,)
            out["lvlb_weights"] = toy.lvlb_weights.numpy()
        loss, ld = toy.p_losses(x_start, cond, t, noise=noise)
        loss.backward()
        assert set(ld) == {"train/loss_simple", "train/loss_vlb", "train/loss"} | ({"train/loss_gamma", "logvar"} if learn else set())
        out[f"{name}_cfg"] = np.array([{"l1": 0, "l2": 1}[loss_type], lsw, ew, lv0, float(learn)], np.float64)
        out[f"{name}_model_output"] = toy.model_output.detach().numpy()
        out[f"{name}_target"] = noise.numpy()
        for k in ("loss_simple", "loss_vlb", "loss"):
            out[f"{name}_{k}"] = ld[f"train/{k}"].detach().numpy()
        if learn:
            out[f"{name}_loss_gamma"] = ld["train/loss_gamma"].detach().numpy()
            out[f"{name}_logvar_mean"] = ld["logvar"].detach().numpy()
        out[f"{name}_d_model_output"] = toy.model_output.grad.numpy()
        out[f"{name}_d_logvar"] = toy.logvar.grad.numpy()
        print(f"{name}: loss {float(loss):.6f}  simple {float(ld['train/loss_simple']):.6f}  vlb {float(ld['train/loss_vlb']):.6f}  "
              f"|d_logvar| nonzero at {np.flatnonzero(out[f'{name}_d_logvar']).tolist()}")

    path = os.path.join(HERE, "f24_objective.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f24_objective.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
