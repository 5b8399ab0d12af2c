#!/usr/bin/env python3
"""F20: ancestral DDPM sampling through the REFERENCE's own code: `LatentDiffusion.sample` / `p_sample_loop` / `p_sample` /
`p_mean_variance` and `DDPM.register_schedule` / `predict_start_from_noise` / `q_posterior` / `q_sample` (ldm/models/diffusion/ddpm.py),
called on a duck-typed `Toy` self that carries the attributes they read (num_timesteps, clip_denoised, log_every_t,
shorten_cond_schedule = False, parameterization 'eps', v_posterior 0, the buffers register_schedule writes) and a closed-form
`apply_model` (the toy_eps of F10 / F19). `ddpm.py` imports pytorch_lightning, torchvision and taming, none of which this fixture needs:
small stub modules stand in for them in sys.modules before the import (this script only). The noise is recorded, not stored: `noise_like`
in the ddpm module's namespace returns prng.normal(SEED, "ddpm.<case>.n<k>") at the k-th step (t = timesteps - 1 - k), and q_sample's
draw of the masked case prng.normal(SEED, "ddpm.<case>.q<k>"); the tests rebuild both from the same recipe.

Contents (STEDM schedule: linear 0.0015 .. 0.0205, T = 1000; B = 2, latents 4 x 8 x 8; the same x_T and cond):
  the seven fp32 buffers (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_variance, posterior_log_variance_clipped,
  posterior_mean_coef1, posterior_mean_coef2, log_one_minus_alphas_cumprod);
  full:   the whole 1000-step chain, clip_denoised on, log_every_t 100: its 12 list intermediates (x_T first; the last is the result);
  short:  timesteps = 20, clip_denoised off;
  masked: timesteps = 50, clip on, a binary [2, 1, 8, 8] mask and x0 (blend after every step, t = 0 included).
  <case>_clamped: how many x0 elements the clamp changed over the chain (|x0| > 1 before clamp_), so a test can see it fire.
The stored bits depend on the machine that ran this script: the toy model's tanh can round differently by an ulp on another CPU or libm
build, and the chain carries that on. tests/test_ddpm_oracle.py therefore pins the chains within F20_TOL = 1e-4 (max |diff| / max |ref|;
the 1000-step chain re-injects fresh noise at every step, so the drift stays near the single-step level, measured <= 1e-6 here) and compares
bit for bit only loops it computes itself; the buffers, computed in f64 and narrowed once, are compared bit for bit.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddpm.py
"""
from __future__ import annotations

import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path.insert(0, os.environ.get("STEDM_REFERENCE", "/root/reference"))

from stedm_amd.utils import prng  # noqa: E402

torch.set_grad_enabled(False)
SEED = 20
SHAPE = (2, 4, 8, 8)
BUFFERS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
           "posterior_mean_coef1", "posterior_mean_coef2", "log_one_minus_alphas_cumprod")
CASES = (("full", None, True, False), ("short", 20, False, False), ("masked", 50, True, True))     # (name, timesteps, clip, masked)


def toy_eps(x: torch.Tensor, t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The closed-form eps model of F10 / F19 (torch, any device)."""
    tf = t.float()[:, None, None, None] / 1000.0
    return torch.tanh(x * (0.5 + tf) + bias) * (0.8 + 0.3 * tf) + 0.1 * bias


def _stub_imports():
    """Empty stand-ins for the modules ddpm.py imports but this fixture does not use."""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules.setdefault(name, m)

    stub("pytorch_lightning", LightningModule=type("LightningModule", (object,), {}))
    stub("pytorch_lightning.utilities")
    stub("pytorch_lightning.utilities.rank_zero", rank_zero_only=lambda f: f)
    stub("pytorch_lightning.utilities.distributed", rank_zero_only=lambda f: f)
    stub("torchvision")
    stub("torchvision.utils", make_grid=None)
    for name in ("taming", "taming.modules", "taming.modules.vqvae"):
        stub(name)
    stub("taming.modules.vqvae.quantize", VectorQuantizer2=object)


def main():
    _stub_imports()
    import ldm.models.diffusion.ddpm as rddpm

    class Toy:
        """The reference's DDPM / LatentDiffusion functions over a duck-typed self."""
        register_schedule = rddpm.DDPM.register_schedule
        q_posterior = rddpm.DDPM.q_posterior
        p_mean_variance = rddpm.LatentDiffusion.p_mean_variance
        p_sample = rddpm.LatentDiffusion.p_sample
        p_sample_loop = rddpm.LatentDiffusion.p_sample_loop
        sample = rddpm.LatentDiffusion.sample

        def __init__(self, tag, clip):
            self.tag = tag
            self.parameterization = "eps"
            self.v_posterior = 0.
            self.clip_denoised = clip
            self.log_every_t = 100
            self.shorten_cond_schedule = False
            self.channels, self.image_size = SHAPE[1], SHAPE[2]
            self.register_schedule(beta_schedule="linear", timesteps=1000, linear_start=0.0015, linear_end=0.0205)
            self.ts = []
            self.q_calls = 0
            self.clamped = 0

        def register_buffer(self, name, value, persistent=True):
            setattr(self, name, value)

        def apply_model(self, x, t, c, return_ids=False):
            self.ts.append(t.clone())
            return toy_eps(x, t, c)

        def predict_start_from_noise(self, x_t, t, noise):
            x0 = rddpm.DDPM.predict_start_from_noise(self, x_t, t, noise)
            self.clamped += int((x0.abs() > 1).sum())            # what clamp_(-1, 1) changes when clip_denoised is on
            return x0

        def q_sample(self, x_start, t, noise=None):
            if noise is None:
                noise = prng.normal(SEED, f"ddpm.{self.tag}.q{self.q_calls}", tuple(x_start.shape))
                self.q_calls += 1
            return rddpm.DDPM.q_sample(self, x_start, t, noise)

    step = {"k": 0, "tag": None}

    def noise_like(shape, device, repeat=False):
        assert not repeat and tuple(shape) == SHAPE
        n = prng.normal(SEED, f"ddpm.{step['tag']}.n{step['k']}", SHAPE)
        step["k"] += 1
        return n.to(device)

    xT = prng.normal(SEED, "ddpm.xT", SHAPE)
    x0 = prng.normal(SEED, "ddpm.x0", SHAPE).clamp(-1, 1)
    cond = prng.normal(SEED, "ddpm.c", SHAPE) * 0.3
    mask = (prng.uniform(SEED, "ddpm.mask", (2, 1, 8, 8)) > 0).float()
    out = {"xT": xT.numpy(), "x0": x0.numpy(), "cond": cond.numpy(), "mask": mask.numpy()}
    orig = rddpm.noise_like
    rddpm.noise_like = noise_like
    try:
        for name, timesteps, clip, masked in CASES:
            toy = Toy(name, clip)
            if name == "full":
                for b in BUFFERS:
                    v = getattr(toy, b)
                    assert v.dtype == torch.float32 and v.shape == (1000,)
                    out[b] = v.numpy()
            step.update(k=0, tag=name)
            kw = dict(mask=mask, x0=x0) if masked else {}
            x, inter = toy.sample(cond, batch_size=SHAPE[0], return_intermediates=True, x_T=xT.clone(), verbose=False,
                                  timesteps=timesteps, **kw)
            T = 1000 if timesteps is None else timesteps
            assert step["k"] == T and [int(t[0]) for t in toy.ts] == list(range(T - 1, -1, -1))
            assert toy.q_calls == (T if masked else 0)
            assert isinstance(inter, list) and torch.equal(inter[0], xT) and torch.equal(inter[-1], x)
            out[f"{name}_T"] = np.int64(T)
            out[f"{name}_clip"] = np.int64(clip)
            out[f"{name}_out"] = x.numpy()
            out[f"{name}_clamped"] = np.int64(toy.clamped if clip else 0)
            out[f"{name}_n_inter"] = np.int64(len(inter))
            if name == "full":
                assert len(inter) == 12
                out["full_inter"] = torch.stack(inter).numpy()
    finally:
        rddpm.noise_like = orig

    path = os.path.join(HERE, "f20_ddpm.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f20_ddpm.npz  {os.path.getsize(path) / 1024:.1f} KB; clamped full {out['full_clamped']} masked {out['masked_clamped']}")


if __name__ == "__main__":
    main()
