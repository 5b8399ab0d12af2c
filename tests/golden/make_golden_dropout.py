#!/usr/bin/env python3
"""F30 - the U-Net with train-mode dropout in its ResBlocks (UNetModel(dropout=0.1), openaimodel.py:241, :473): the reference's own
`UNetModel` is imported from the reference tree, filled from the PRNG recipe and run on the CPU in train(), forward + L1 loss + backward,
in the TINY configuration of tests/test_gpu_unet.py / tests/test_gpu_train.py (B = 2, 16 x 16, seed 6, t = [951, 21]), plain and with
use_scale_shift_norm=True. torch's generator stream cannot be reproduced by another implementation, so every out_layers[2] (nn.Dropout) is
replaced by a module that applies the project's counter-based mask (tests/refs_dropout.py: seed DROP_SEED, step DROP_STEP, site
0x55000000 + the ResBlock's ordinal in execution order; the NHWC mask permuted to NCHW) with the reference's own arithmetic around it;
the reference's checkpointing recomputes with the same deterministic masks.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dropout.py
Only numbers are written, in the f29 format (f30_unet_dropout[_film]_tiny.npz: the output y; f30_grads_dropout[_film]_tiny.npz: the loss,
dx, dctx and per-parameter gradient summaries), plus p, drop_seed and drop_step; nothing of the reference travels.
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
REF = os.environ.get("STEDM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from stedm_amd.utils import prng  # noqa: E402
from tests import refs_dropout as RD  # noqa: E402
from tests.golden.make_golden_grads import grad_summary  # noqa: E402
from tests.golden.summary import summarize  # noqa: E402

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
B, HW, SEED = 2, 16, 6
P, DROP_SEED, DROP_STEP = 0.1, 0x5EED0D120F00D, 3


class StreamDropout(torch.nn.Module):
    """nn.Dropout(p) in train() with the mask of site 0x55000000 + k at (DROP_SEED, DROP_STEP) instead of torch's generator"""

    def __init__(self, p, k):
        super().__init__()
        self.p, self.k = p, k

    def forward(self, x):
        b, c, h, w = x.shape
        m = RD.resblock_mask(b, h * w, c, self.p, DROP_SEED, self.k, DROP_STEP).view(b, h, w, c).permute(0, 3, 1, 2)
        return x * (m.to(x.dtype) * float(RD.inv_keep(self.p)))


def run(film: bool):
    from ldm.modules.diffusionmodules import openaimodel as rom

    tag = "dropout_film_tiny" if film else "dropout_tiny"
    src = "film_tiny" if film else "tiny"            # (the input tensors of the f29 / f14 fixtures of the same net)
    kw = dict(TINY, dropout=P, use_scale_shift_norm=film)
    tt = torch.tensor(([951, 21, 500, 1] * B)[:B], dtype=torch.long)
    m = rom.UNetModel(**kw).train()
    prng.fill_module_(m, seed=SEED)
    k = 0
    for blk in list(m.input_blocks) + [m.middle_block] + list(m.output_blocks):
        for layer in blk:
            rb = layer if isinstance(layer, rom.ResBlock) else layer.block if isinstance(layer, rom.ResBlockStyle) else None
            if rb is not None:
                assert isinstance(rb.out_layers[2], torch.nn.Dropout) and rb.out_layers[2].p == P
                rb.out_layers[2] = StreamDropout(P, k)
                k += 1
    assert k == 18
    x = prng.normal(SEED, f"unet.{src}.x", (B, kw["in_channels"], HW, HW)).requires_grad_(True)
    ctx = prng.normal(SEED, f"unet.{src}.ctx", (B, kw["model_channels"] * 4)).requires_grad_(True)
    target = prng.normal(SEED, f"unet.{src}.target", (B, kw["out_channels"], HW, HW))
    y = m(x, tt, context=ctx)
    loss = (y - target).abs().mean(dim=(1, 2, 3)).mean()
    loss.backward()
    common = {"t": tt.numpy(), "p": np.float64(P), "drop_seed": np.int64(DROP_SEED), "drop_step": np.int64(DROP_STEP)}

    d = dict(common, n_params=np.int64(sum(p.numel() for p in m.parameters())), y=y.detach().numpy())
    for kk, v in summarize(y.detach()).items():
        d[f"y.{kk}"] = v
    path = os.path.join(HERE, f"f30_unet_{tag}.npz")
    np.savez(path, **d)
    print(f"wrote {os.path.basename(path)} {os.path.getsize(path) / 1024:.1f} KB  y std {float(y.detach().std()):.4f}")

    d = dict(common, loss=np.float64(loss.item()))
    for kk, v in summarize(x.grad).items():
        d[f"dx.{kk}"] = v
    d["dctx"] = ctx.grad.numpy()
    d["dx"] = x.grad.numpy()
    missing = [n for n, p in m.named_parameters() if p.grad is None]
    assert not missing, missing
    d.update(grad_summary((n, p.grad) for n, p in m.named_parameters()))
    path = os.path.join(HERE, f"f30_grads_{tag}.npz")
    np.savez(path, **d)
    print(f"wrote {os.path.basename(path)} {os.path.getsize(path) / 1024:.1f} KB  loss {loss.item():.6f}")


if __name__ == "__main__":
    run(False)
    run(True)
