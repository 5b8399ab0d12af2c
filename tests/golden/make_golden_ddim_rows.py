#!/usr/bin/env python3
"""F26: DDIM sampling with one guidance scale per sample, assembled from the REFERENCE's own `DDIMSampler.sample` / `ddim_sampling` /
`p_sample_ddim` (ldm/models/diffusion/ddim.py:56-210) under the CPUSampler override of F10 / F17 / F21, with the closed-form `Toy` eps
model of F10 / F21. The reference takes one scalar scale, and a sample's update depends on that sample alone (the rescale statistic of
ddim.py:182-183 is per sample and column), so the per-sample result is defined row by row: the reference runs once per DISTINCT scale on
the whole batch, and row b is taken from the run that used scales[b]. A row at scale 1 comes from the reference's unguided branch
(ddim.py:170-171). Nothing random is drawn from torch's generator; the noise is recorded, not stored: `noise_like` (ddim.py:206) returns
prng.normal(SEED, "rows.n<k>") at iteration k, the same tensor in every run. The tests rebuild it, and x_T and the two conditionings
(`inputs`), from the same recipes; the file holds the scales, the final latents and the last iteration's pred_x0.

Setup: B = 4, latents 3 x 8 x 8, S = 6 (7 iterations), scales [1, 3, 5, 3], rescale phi 0.7, eta 0 and eta 1.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddim_rows.py

The reference tree is looked for at $STEDM_REFERENCE, else next to this repository's checkout (../reference).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stedm_amd.utils import prng  # noqa: E402

SEED = 26
SHAPE = (4, 3, 8, 8)
S = 6
ITERS = len(range(0, 1000, 1000 // S))      # 7: the uniform stride of ddim.py's make_ddim_timesteps
SCALES = (1.0, 3.0, 5.0, 3.0)
ETAS = {"eta0": 0.0, "eta1": 1.0}
PATH = os.path.join(HERE, "f26_ddim_rows.npz")


def reference_dir() -> str:
    return os.environ.get("STEDM_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")


def inputs():
    """x_T, the conditional and the unconditional conditioning of the toy model: recipes, not stored."""
    return (prng.normal(SEED, "rows.xT", SHAPE), {"bias": prng.normal(SEED, "rows.c", SHAPE) * 0.3},
            {"bias": prng.normal(SEED, "rows.u", SHAPE) * 0.3})


def noises():
    """iteration k's N(0, 1) draw (eta 1)"""
    return [prng.normal(SEED, f"rows.n{k}", SHAPE) for k in range(ITERS)]


def generate() -> dict:
    """The fixture's arrays, computed from the reference (ImportError when its tree is not there)."""
    sys.dont_write_bytecode = True
    ref = reference_dir()
    if ref not in sys.path:
        sys.path.insert(0, ref)
    import ldm.models.diffusion.ddim as rddim
    from ldm.modules.diffusionmodules import util as rutil

    betas = rutil.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)

    class CPUSampler(rddim.DDIMSampler):
        def register_buffer(self, name, attr):  # harness override: the original pins "cuda" (ddim.py:18-22)
            setattr(self, name, attr)

    class Toy:
        """Duck-typed model surface of ddim.py:15, 27-33, 119, 177-178."""
        def __init__(self):
            self.num_timesteps = 1000
            self.betas = f32(betas)
            self.alphas_cumprod = f32(ac)
            self.alphas_cumprod_prev = f32(np.append(1.0, ac[:-1]))
            self.device = torch.device("cpu")
            self.calls = 0

        def apply_model(self, x, t, c):
            self.calls += 1
            tf = t.float()[:, None, None, None] / 1000.0
            return torch.tanh(x * (0.5 + tf) + c["bias"]) * (0.8 + 0.3 * tf) + 0.1 * c["bias"]

    state = {"n": 0}

    def noise_like(shape, device, repeat=False):
        assert not repeat and tuple(shape) == SHAPE
        n = prng.normal(SEED, f"rows.n{state['n']}", SHAPE)
        state["n"] += 1
        return n

    orig_nl = rddim.noise_like
    rddim.noise_like = noise_like
    try:
        with torch.no_grad():
            xT, cond, unc = inputs()
            out = {"scales": np.asarray(SCALES, dtype=np.float32)}
            for tag, eta in ETAS.items():
                runs = {}
                calls = 0
                for s in sorted(set(SCALES)):
                    state["n"] = 0
                    toy = Toy()
                    smp, inter = CPUSampler(toy).sample(S, SHAPE[0], SHAPE[1:], cond, verbose=False, eta=eta, x_T=xT, log_every_t=1,
                                                        unconditional_guidance_scale=s, unconditional_conditioning=unc)
                    assert state["n"] == ITERS
                    runs[s] = (smp, inter["pred_x0"][-1])
                    calls += toy.calls
                out[f"{tag}_out"] = torch.stack([runs[s][0][b] for b, s in enumerate(SCALES)]).numpy()
                out[f"{tag}_pred_x0"] = torch.stack([runs[s][1][b] for b, s in enumerate(SCALES)]).numpy()
                out[f"{tag}_calls"] = np.int64(calls)        # ITERS for the unguided run + 2 ITERS for each guided one
    finally:
        rddim.noise_like = orig_nl
    return {k: np.asarray(v) for k, v in out.items()}


def main():
    np.savez_compressed(PATH, **generate())
    print(f"wrote f26_ddim_rows.npz  {os.path.getsize(PATH) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
