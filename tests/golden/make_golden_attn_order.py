#!/usr/bin/env python3
"""F33 — the U-Net with use_new_attention_order=True (the middle AttentionBlock runs QKVAttention, openaimodel.py:401-428: the 3C channels
of the qkv convolution split into q | k | v first and into heads second, where QKVAttentionLegacy, :369-394, splits heads first): the
reference's own `UNetModel` is imported from the reference tree, filled from the PRNG recipe and run on the CPU, forward and forward + L1
loss + backward, in the TINY configuration of tests/test_gpu_unet.py / tests/test_gpu_train.py (B = 2, seed 6, t = [951, 21]):

    neworder_tiny        16 x 16: the middle attention has T = 16 tokens, 4 heads of 32          forward, backward
    neworder_t64         image_size = 32, 32 x 32: T = 64, 4 heads of 32 (the 64-token forms)    forward, backward
    neworder_nhc_tiny    16 x 16, num_heads=-1, num_head_channels=64: 2 heads of 64               forward

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn_order.py
Only numbers and names are written, nothing of the reference travels:
  f33_unet_<tag>.npz     the output y, t, n_params, summaries, order_gap
  f33_grads_<tag>.npz    the loss, dx, dctx and per-parameter gradient summaries as in make_golden_grads.py, order_gap, qkv_grad_gap
  f33_qkvattention.npz   the reference's QKVAttention module itself on a small random qkv [2][3 * 3 * 8][5] (3 heads of 8): input and output
  f33_unet_neworder_names.json   the reference constructor's state-dict names and shapes (the same for every tag but nhc's head count,
                                 which no parameter's shape depends on)
The state dict is the same in both orders, so a checkpoint of one order loads into the other and gives a wrong picture with no error.
The same weights are therefore also run with use_new_attention_order=False:
  order_gap = max|y_new - y_legacy| / std(y_new) is stored and asserted > 0.1, twice the loosest mode threshold of the GPU tests (bf16:
  5e-2), so that no mode's tolerance can hide a swapped layout; qkv_grad_gap = |g_new - g_legacy| / |g_new| (L2) of the gradient of
  middle_block.2.qkv.weight is stored with the gradients.
Every tensor is deterministic (utils/prng.py; the CPU forward and backward are run single-threaded).
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

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
# tag -> (constructor arguments, input height / width, with the backward)
CONFIGS = {"neworder_tiny": (TINY, 16, True),
           "neworder_t64": (dict(TINY, image_size=32), 32, True),
           "neworder_nhc_tiny": (dict(TINY, num_heads=-1, num_head_channels=64), 16, False)}
B, SEED = 2, 6
MIN_GAP = 0.1
QKV = "middle_block.2.qkv.weight"


def one(rom, tag, kw, HW, backward):
    tt = torch.tensor(([951, 21, 500, 1] * B)[:B], dtype=torch.long)

    def model(new, train):
        m = rom.UNetModel(use_new_attention_order=new, **kw)
        m = m.train() if train else m.eval()
        prng.fill_module_(m, seed=SEED)
        return m

    # ---- forward (eval, no autograd), both orders on the same weights
    x = prng.normal(SEED, f"unet.{tag}.x", (B, kw["in_channels"], HW, HW))
    ctx = prng.normal(SEED, f"unet.{tag}.ctx", (B, kw["model_channels"] * 4))
    m = model(True, False)
    with torch.no_grad():
        y = m(x, tt, context=ctx)
        y_legacy = model(False, False)(x, tt, context=ctx)
    gap = float((y - y_legacy).abs().max() / y.std())
    assert gap > MIN_GAP, f"{tag}: the two orders differ by {gap:.3f} std only"
    d = {"t": tt.numpy(), "n_params": np.int64(sum(p.numel() for p in m.parameters())), "y": y.numpy(), "order_gap": np.float64(gap)}
    for k, v in summarize(y).items():
        d[f"y.{k}"] = v
    path = os.path.join(HERE, f"f33_unet_{tag}.npz")
    np.savez(path, **d)
    print(f"wrote {os.path.basename(path)} {os.path.getsize(path) / 1024:.1f} KB  y std {float(y.std()):.4f}  n_params {int(d['n_params'])}  "
          f"order_gap {gap:.3f}")
    names = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert names == {k: list(v.shape) for k, v in model(False, False).state_dict().items()}, "the state dict is the same in both orders"
    if not backward:
        return names, gap

    # ---- forward + L1 loss + backward (train(): dropout = 0, checkpointing active as in training), both orders
    target = prng.normal(SEED, f"unet.{tag}.target", (B, kw["out_channels"], HW, HW))
    res = {}
    for new in (True, False):
        m = model(new, True)
        xg = prng.normal(SEED, f"unet.{tag}.x", (B, kw["in_channels"], HW, HW)).requires_grad_(True)
        cg = prng.normal(SEED, f"unet.{tag}.ctx", (B, kw["model_channels"] * 4)).requires_grad_(True)
        yt = m(xg, tt, context=cg)
        loss = (yt - target).abs().mean(dim=(1, 2, 3)).mean()
        loss.backward()
        res[new] = (m, xg, cg, loss)
    m, xg, cg, loss = res[True]
    g_new, g_leg = dict(m.named_parameters())[QKV].grad.double(), dict(res[False][0].named_parameters())[QKV].grad.double()
    qgap = float((g_new - g_leg).norm() / g_new.norm())
    d = {"t": tt.numpy(), "loss": np.float64(loss.item()), "order_gap": np.float64(gap), "qkv_grad_gap": np.float64(qgap)}
    for k, v in summarize(xg.grad).items():
        d[f"dx.{k}"] = v
    d["dctx"] = cg.grad.numpy()
    d["dx"] = xg.grad.numpy()
    missing = [n for n, p in m.named_parameters() if p.grad is None]
    assert not missing, missing
    d.update(grad_summary((n, p.grad) for n, p in m.named_parameters()))
    path = os.path.join(HERE, f"f33_grads_{tag}.npz")
    np.savez(path, **d)
    print(f"wrote {os.path.basename(path)} {os.path.getsize(path) / 1024:.1f} KB  loss {loss.item():.6f}  qkv_grad_gap {qgap:.3f}")
    return names, gap


def main():
    from ldm.modules.diffusionmodules import openaimodel as rom
    torch.set_num_threads(1)          # a fixed reduction order: the files regenerate bit-equal
    all_names = []
    for tag, (kw, HW, backward) in CONFIGS.items():
        all_names.append(one(rom, tag, kw, HW, backward)[0])
    assert all(n == all_names[0] for n in all_names), "one names file serves every tag"
    qkv = prng.normal(SEED, "qkvattention.qkv", (2, 3 * 3 * 8, 5))
    with torch.no_grad():
        out = rom.QKVAttention(3)(qkv)
    path = os.path.join(HERE, "f33_qkvattention.npz")
    np.savez(path, qkv=qkv.numpy(), out=out.numpy(), heads=np.int64(3))
    print(f"wrote {os.path.basename(path)}")
    path = os.path.join(HERE, "f33_unet_neworder_names.json")
    with open(path, "w") as f:
        json.dump(all_names[0], f, indent=0)
        f.write("\n")
    print(f"wrote {os.path.basename(path)}")


if __name__ == "__main__":
    main()
