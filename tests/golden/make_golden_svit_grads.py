#!/usr/bin/env python3
"""F34: parameter gradients of the reference's set-ViT in TRAIN mode. Imports the reference's own `networks.vit_set.sViT` (read-only
checkout, STEDM_REFERENCE), PRNG-recipe weights, `.train()` with torch.nn.functional.dropout replaced by the oracle/dropmask.py mask injector
(as make_golden_train_drop.py; site order of sViT.forward), autograd ON, loss = (out * g).sum() for a recorded g. Stores the inputs, g, the
output and the gradient of every parameter (fp32) in f34_svit_grads.npz.

The same module is then run in fp64 (`.double()`, same masks): f34_svit_grads_f64.npz holds, per parameter, the difference fp64 - fp32 of
the two gradients as fp16 fractions of its own largest magnitude (`<name>` and `<name>.scale`), from which a test rebuilds the fp64 gradient
(to ~1e-3 of the fp32 rounding error) and measures fp32 autograd against fp64 autograd of the reference module itself. A second file,
because a committed file stays under 1 MiB.

    STEDM_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_svit_grads.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
if "STEDM_REFERENCE" not in os.environ:
    sys.exit("set STEDM_REFERENCE to a checkout of the reference (OettlM/STEDM): its networks.vit_set.sViT is imported from there")
sys.path.insert(0, os.environ["STEDM_REFERENCE"])

from oracle import dropmask  # noqa: E402
from stedm_amd.utils import prng  # noqa: E402

SEED = 0x5EED00D5
SITE_EMB, SITE_ATTN, SITE_OUT, SITE_FF1, SITE_FF2 = 0x10000, 1, 2, 3, 4
NUM_CLASSES = 32
#        tag              image ns B depth heads mlp  pool    dropout
CASES = {"i16_ns2_d2":    (16,  2, 2, 2,    3,   64,  "mean", 0.1),
         "i64_ns1_d1_p0": (64,  1, 1, 1,    2,   128, "cls",  0.0)}


def main():
    import torch.nn.functional as F
    from networks.vit_set import sViT
    out = {"seed": np.array([SEED], dtype=np.int64)}
    out64 = {}
    for tag, (img, ns, B, depth, heads, mlp, pool, p) in CASES.items():
        m = sViT(image_size=img, patch_size=8, num_classes=NUM_CLASSES, dim=64, depth=depth, heads=heads, mlp_dim=mlp, pool=pool,
                 channels=3, dropout=p, emb_dropout=p, ns=ns, t_dim=256).train()
        with torch.no_grad():
            prng.fill_module_(m, seed=34)
            for l, (attn, _ff) in enumerate(m.transformer.layers):
                attn.fn.temperature.fill_(float(np.log(64 ** -0.5)) + 0.05 * l)
        x = prng.uniform(34, f"svit.grads.{tag}.img", (B, ns, img, img, 3))
        g = prng.normal(34, f"svit.grads.{tag}.g", (B, NUM_CLASSES))
        calls = []

        def injected(inp, p=0.5, training=True, inplace=False):
            assert training and not inplace
            i = len(calls)
            if i == 0:
                site, kind = SITE_EMB, "emb"
            else:
                layer, k = divmod(i - 1, 4)
                site, kind = 8 * layer + (SITE_ATTN, SITE_OUT, SITE_FF1, SITE_FF2)[k], ("attn", "out", "ff1", "ff2")[k]
            calls.append((kind, tuple(inp.shape), p))
            if p == 0:
                return inp
            if kind == "attn":
                b, h, n, _ = inp.shape
                keep = dropmask.keep_attention(b * h, n, p, SEED, site).reshape(inp.shape)
            else:
                keep = dropmask.keep_elementwise(inp.numel(), p, SEED, site).reshape(inp.shape)
            return inp * (torch.from_numpy(keep.copy()).float() / (1.0 - p))

        import copy
        m64 = copy.deepcopy(m).double()
        orig = F.dropout
        F.dropout = injected
        try:
            y = m(x)
            (y * g).sum().backward()
            ncalls = len(calls)
            del calls[:]
            (m64(x.double()) * g.double()).sum().backward()
            assert len(calls) == ncalls
        finally:
            F.dropout = orig
        assert len(calls) == 1 + 4 * depth and calls[1][0] == "attn" and len(calls[1][1]) == 4, calls
        out[tag + ".img"] = x.numpy()
        out[tag + ".g"] = g.numpy()
        out[tag + ".out"] = y.detach().numpy()
        for name, prm in m.named_parameters():
            g32 = (torch.zeros_like(prm) if prm.grad is None else prm.grad).detach()
            out[f"{tag}.grad.{name}"] = g32.numpy()
            p64 = dict(m64.named_parameters())[name]
            delta = (torch.zeros_like(p64) if p64.grad is None else p64.grad.detach()) - g32.double()
            scale = float(delta.abs().max())
            out64[f"{tag}.grad.{name}"] = (delta / scale if scale > 0 else delta).numpy().astype(np.float16)
            out64[f"{tag}.grad.{name}.scale"] = np.array([scale], dtype=np.float64)
        print(tag, "out", tuple(y.shape), "params", sum(1 for _ in m.parameters()))
    path = os.path.join(HERE, "f34_svit_grads.npz")
    np.savez_compressed(path, **out)
    print("wrote f34_svit_grads.npz", os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "f34_svit_grads_f64.npz")
    np.savez_compressed(path, **out64)
    print("wrote f34_svit_grads_f64.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
