#!/usr/bin/env python3
"""F32 — the U-Net with resblock_updown=True (every resolution change is a ResBlock(up / down) whose two branches are resampled without
parameters; openaimodel.py:220-229, 268-275, 596-613, 709-724): the reference's own `UNetModel` is imported from the reference tree, filled from the PRNG recipe and run on the CPU, forward and
forward + L1 loss + backward, in the TINY configuration of tests/test_gpu_unet.py / tests/test_gpu_train.py (B = 2, 16 x 16, seed 6,
t = [951, 21]); once plain and once with use_scale_shift_norm=True, so that the option combination is pinned by the reference as well.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_updown.py
Only numbers and names are written, nothing of the reference travels:
  f32_unet_<tag>.npz     the output y, t, n_params, summaries
  f32_grads_<tag>.npz    the loss, dx, dctx and per-parameter gradient summaries as in make_golden_grads.py
  f32_unet_<tag without _tiny>_names.json   the reference's state-dict names and shapes
for <tag> in updown_tiny, updown_film_tiny. Every tensor is deterministic (utils/prng.py; the CPU forward and backward are run single-threaded).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
REF = os.environ.get("STEDM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from stedm_amd.utils import prng  # noqa: E402
from tests.golden.make_golden_grads import grad_summary  # noqa: E402
from tests.golden.summary import summarize  # noqa: E402

TINY_UPDOWN = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
                   attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4, resblock_updown=True)
CONFIGS = {"updown_tiny": TINY_UPDOWN, "updown_film_tiny": dict(TINY_UPDOWN, use_scale_shift_norm=True)}
B, HW, SEED = 2, 16, 6


def one(rom, tag, kw):
    tt = torch.tensor(([951, 21, 500, 1] * B)[:B], dtype=torch.long)

    # ---- forward (eval, no autograd)
    m = rom.UNetModel(**kw).eval()
    prng.fill_module_(m, seed=SEED)
    x = prng.normal(SEED, f"unet.{tag}.x", (B, kw["in_channels"], HW, HW))
    ctx = prng.normal(SEED, f"unet.{tag}.ctx", (B, kw["model_channels"] * 4))
    with torch.no_grad():
        y = m(x, tt, context=ctx)
    d = {"t": tt.numpy(), "n_params": np.int64(sum(p.numel() for p in m.parameters())), "y": y.numpy()}
    for k, v in summarize(y).items():
        d[f"y.{k}"] = v
    path = os.path.join(HERE, f"f32_unet_{tag}.npz")
    np.savez(path, **d)
    print(f"wrote {os.path.basename(path)} {os.path.getsize(path) / 1024:.1f} KB  y std {float(y.std()):.4f}  n_params {int(d['n_params'])}")
    path = os.path.join(HERE, f"f32_unet_{tag[:-5]}_names.json")
    with open(path, "w") as f:
        json.dump({k: list(v.shape) for k, v in m.state_dict().items()}, f, indent=0)
        f.write("\n")
    print(f"wrote {os.path.basename(path)}")

    # ---- forward + L1 loss + backward (train(): dropout = 0, checkpointing active as in training)
    m = rom.UNetModel(**kw).train()
    prng.fill_module_(m, seed=SEED)
    x = prng.normal(SEED, f"unet.{tag}.x", (B, kw["in_channels"], HW, HW)).requires_grad_(True)
    ctx = prng.normal(SEED, f"unet.{tag}.ctx", (B, kw["model_channels"] * 4)).requires_grad_(True)
    target = prng.normal(SEED, f"unet.{tag}.target", (B, kw["out_channels"], HW, HW))
    y = m(x, tt, context=ctx)
    loss = (y - target).abs().mean(dim=(1, 2, 3)).mean()
    loss.backward()
    d = {"t": tt.numpy(), "loss": np.float64(loss.item())}
    for k, v in summarize(x.grad).items():
        d[f"dx.{k}"] = v
    d["dctx"] = ctx.grad.numpy()
    d["dx"] = x.grad.numpy()
    missing = [n for n, p in m.named_parameters() if p.grad is None]
    assert not missing, missing
    d.update(grad_summary((n, p.grad) for n, p in m.named_parameters()))
    path = os.path.join(HERE, f"f32_grads_{tag}.npz")
    np.savez(path, **d)
    print(f"wrote {os.path.basename(path)} {os.path.getsize(path) / 1024:.1f} KB  loss {loss.item():.6f}")


def main():
    from ldm.modules.diffusionmodules import openaimodel as rom
    torch.set_num_threads(1)          # a fixed reduction order: the files regenerate bit-equal
    for tag, kw in CONFIGS.items():
        one(rom, tag, kw)


if __name__ == "__main__":
    main()
