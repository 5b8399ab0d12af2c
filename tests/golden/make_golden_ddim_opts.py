#!/usr/bin/env python3
"""F21: DDIM sampling with temperature, noise_dropout and quantize_x0 through the REFERENCE's own `DDIMSampler.sample` / `ddim_sampling` /
`p_sample_ddim` (ldm/models/diffusion/ddim.py:56-210) under the CPUSampler override of F10 / F17, with the closed-form `Toy` eps model of
F10 / F19. quantize_x0 calls `model.first_stage_model.quantize(pred_x0)` (ddim.py:202-203); taming is not importable here, so the toy
first stage restates VectorQuantizer2's eval path (placement pinned by the reference, quantiser unpinned: SURVEY §8c): d = |z|^2 + |e|^2 -
2 z.e per latent pixel, argmin, z + (e - z).detach(). Nothing random is drawn from torch's generator; the noise is recorded, not stored:
  * `noise_like` (ddim.py:206) returns prng.normal(SEED, "opts.<case>.n<k>") at iteration k;
  * torch.nn.functional.dropout (ddim.py:208) keeps element i at iteration k iff prng.uniform(SEED, "opts.<case>.d<k>", lo=0, hi=1)[i]
    >= p and multiplies by keep / (1 - p) (torch's train-mode rule, its mask replaced by the recorded one).
The tests rebuild both from the same recipes.

Cases (B = 2, latents 3 x 8 x 8, S = 10, a 64 x 3 codebook; the same x_T, cond, uncond):
  a) eta = 1, temperature 0.7;
  b) eta = 0.5, noise_dropout 0.2;
  c) eta = 0, quantize_x0;
  d) eta = 1, temperature 0.7, noise_dropout 0.2, quantize_x0, CFG 1.5 (rescale phi 0.7).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddim_opts.py
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
SEED = 21
SHAPE = (2, 3, 8, 8)
N_E = 64
S = 10
CASES = {"a": dict(eta=1.0, temperature=0.7), "b": dict(eta=0.5, noise_dropout=0.2), "c": dict(eta=0.0, quantize_x0=True),
         "d": dict(eta=1.0, temperature=0.7, noise_dropout=0.2, quantize_x0=True, cfg=1.5)}


def vq_quantize(z: torch.Tensor, emb: torch.Tensor):
    """VectorQuantizer2.forward's eval path (legacy, no remap): -> (z_q, loss, (perplexity, min_encodings, indices))."""
    zp = z.permute(0, 2, 3, 1).contiguous()
    zf = zp.view(-1, emb.shape[1])
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(emb ** 2, dim=1) - 2 * torch.einsum('bd,dn->bn', zf, emb.t())
    idx = torch.argmin(d, dim=1)
    zq = emb[idx].view(zp.shape)
    zq = zp + (zq - zp).detach()
    return zq.permute(0, 3, 1, 2).contiguous(), None, (None, None, idx)


def main():
    import ldm.models.diffusion.ddim as rddim
    from ldm.modules.diffusionmodules import util as rutil

    betas = rutil.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0205)
    ac = np.cumprod(1.0 - betas, axis=0)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    codebook = prng.normal(SEED, "opts.codebook", (N_E, SHAPE[1])) * 0.8

    class CPUSampler(rddim.DDIMSampler):
        def register_buffer(self, name, attr):  # harness override: the original pins "cuda" (ddim.py:18-22)
            setattr(self, name, attr)

    class Quantizer:
        def __init__(self):
            self.calls = 0

        def __call__(self, z):
            self.calls += 1
            return vq_quantize(z, codebook)

    class FirstStage:
        def __init__(self):
            self.quantize = Quantizer()

    class Toy:
        """Duck-typed model surface of ddim.py:15, 27-33, 119, 177-178, 202."""
        def __init__(self):
            self.num_timesteps = 1000
            self.betas = f32(betas)
            self.alphas_cumprod = f32(ac)
            self.alphas_cumprod_prev = f32(np.append(1.0, ac[:-1]))
            self.device = torch.device("cpu")
            self.first_stage_model = FirstStage()
            self.calls = 0

        def apply_model(self, x, t, c):
            self.calls += 1
            tf = t.float()[:, None, None, None] / 1000.0
            return torch.tanh(x * (0.5 + tf) + c["bias"]) * (0.8 + 0.3 * tf) + 0.1 * c["bias"]

    state = {"case": None, "n": 0, "d": 0}

    def noise_like(shape, device, repeat=False):
        assert not repeat and tuple(shape) == SHAPE
        n = prng.normal(SEED, f"opts.{state['case']}.n{state['n']}", SHAPE)
        state["n"] += 1
        return n

    def dropout(x, p=0.5, training=True, inplace=False):
        assert training and not inplace and tuple(x.shape) == SHAPE
        keep = prng.uniform(SEED, f"opts.{state['case']}.d{state['d']}", SHAPE, lo=0.0, hi=1.0) >= p
        state["d"] += 1
        return x * (keep.float().div_(1 - p))

    orig_nl, orig_do = rddim.noise_like, torch.nn.functional.dropout
    rddim.noise_like = noise_like
    torch.nn.functional.dropout = dropout
    try:
        xT = prng.normal(SEED, "opts.xT", SHAPE)
        cond = {"bias": prng.normal(SEED, "opts.c", SHAPE) * 0.3}
        unc = {"bias": prng.normal(SEED, "opts.u", SHAPE) * 0.3}
        out = {"xT": xT.numpy(), "cond": cond["bias"].numpy(), "uncond": unc["bias"].numpy(), "codebook": codebook.numpy()}
        for case, o in CASES.items():
            state.update(case=case, n=0, d=0)
            toy = Toy()
            kw = dict(unconditional_guidance_scale=o["cfg"], unconditional_conditioning=unc) if "cfg" in o else {}
            smp, inter = CPUSampler(toy).sample(S, SHAPE[0], SHAPE[1:], cond, verbose=False, eta=o["eta"], x_T=xT,
                                                temperature=o.get("temperature", 1.0), noise_dropout=o.get("noise_dropout", 0.0),
                                                quantize_x0=o.get("quantize_x0", False), log_every_t=1, **kw)
            assert state["n"] == S and state["d"] == (S if o.get("noise_dropout", 0.0) > 0 else 0)
            assert toy.first_stage_model.quantize.calls == (S if o.get("quantize_x0") else 0)
            out[f"{case}_out"] = smp.numpy()
            out[f"{case}_pred_x0"] = torch.stack(inter["pred_x0"][1:]).numpy()
            out[f"{case}_calls"] = np.int64(toy.calls)
    finally:
        rddim.noise_like = orig_nl
        torch.nn.functional.dropout = orig_do

    path = os.path.join(HERE, "f21_ddim_opts.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote f21_ddim_opts.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
