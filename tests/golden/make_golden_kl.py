#!/usr/bin/env python3
"""F27: KL first-stage golden vectors. Imports the reference's own `ldm.modules.diffusionmodules.model.Encoder / Decoder` and
`ldm.modules.distributions.distributions.DiagonalGaussianDistribution` (read-only, at run time) and composes AutoencoderKL's `encode` /
`decode` exactly as ldm/models/autoencoder.py:324-333 does, with nn.Conv2d glue (`ldm.models.autoencoder` itself needs pytorch_lightning
+ taming, absent here). Everything is filled from the PRNG recipe under the AutoencoderKL state-dict names (`encoder.*`, `decoder.*`,
`quant_conv.*`, `post_quant_conv.*`). Writes f27_kl_first_stage.npz (the reference's outputs) and f27_kl_names.json (the ordered state-dict
names and shapes: the contract of stedm_amd.vq.AutoencoderKL).

    STEDM_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kl.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
if "STEDM_REFERENCE" not in os.environ:
    sys.exit("set STEDM_REFERENCE to a checkout of the reference (the directory that holds ldm/)")
sys.path.insert(0, os.environ["STEDM_REFERENCE"])

from stedm_amd.utils import prng  # noqa: E402

torch.set_grad_enabled(False)
SEED = 27
SIDE, BATCH = 64, 2
CASES = {  # tag: (ddconfig, embed_dim)
    # four levels, the kl-f8 family: 64^2 image -> 8^2 latents
    "kl_tiny": (dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4], num_res_blocks=1,
                     attn_resolutions=[], dropout=0.0), 4),
    # three levels, embed_dim != z_channels (the glue convolutions are not square): 64^2 image -> 16^2 latents
    "kl_f4e": (dict(double_z=True, z_channels=3, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4], num_res_blocks=2,
                    attn_resolutions=[], dropout=0.0), 4),
}


def dist_moments():
    """synthetic moments [2, 8, 4, 4]: log-variances over -60 .. 40 in a fixed shuffled order, -30 and 20 (the clamp's ends) exactly among them"""
    mean = prng.normal(SEED, "kl.dist.mean", (2, 4, 4, 4))
    lv = np.linspace(-60.0, 40.0, 128, dtype=np.float32)
    lv[37], lv[101] = -30.0, 20.0
    lv = lv[np.random.Generator(np.random.Philox(key=[SEED, 1])).permutation(128)]
    return torch.cat([mean, torch.from_numpy(lv).view(2, 4, 4, 4)], dim=1).contiguous()


def dist_other():
    return torch.cat([prng.normal(SEED, "kl.dist.other.mean", (2, 4, 4, 4)), prng.uniform(SEED, "kl.dist.other.logvar", (2, 4, 4, 4), -2.0, 2.0)], dim=1)


def main():
    from ldm.modules.diffusionmodules import model as rm
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    out, names = {}, {}
    for tag, (dd, e) in CASES.items():
        net = torch.nn.Module()
        with contextlib.redirect_stdout(io.StringIO()):
            net.encoder, net.decoder = rm.Encoder(**dd), rm.Decoder(**dd)
        net.quant_conv = torch.nn.Conv2d(2 * dd["z_channels"], 2 * e, 1)          # autoencoder.py:302-303
        net.post_quant_conv = torch.nn.Conv2d(e, dd["z_channels"], 1)
        net.eval()
        prng.fill_module_(net, seed=SEED)
        f = 2 ** (len(dd["ch_mult"]) - 1)
        x = prng.uniform(SEED, f"kl.{tag}.x", (BATCH, 3, SIDE, SIDE))
        z = prng.normal(SEED, f"kl.{tag}.z", (BATCH, e, SIDE // f, SIDE // f))
        enc_out = net.encoder(x)
        moments = net.quant_conv(enc_out)                                         # encode, autoencoder.py:324-328
        post = DiagonalGaussianDistribution(moments)
        dec = net.decoder(net.post_quant_conv(z))                                 # decode, autoencoder.py:330-333
        rec = {"enc_out": enc_out, "moments": moments, "dec_out": dec, "mean": post.mean, "logvar": post.logvar, "std": post.std, "var": post.var,
               "kl": post.kl(), "nll": post.nll(z)}
        out.update({f"{tag}.{k}": v.numpy() for k, v in rec.items()})
        print(f"{tag}: moments {tuple(moments.shape)}, logvar in [{float(post.logvar.min()):.3f}, {float(post.logvar.max()):.3f}], "
              f"decoder output {tuple(dec.shape)}")
        names[tag] = {"ddconfig": dd, "embed_dim": e, "params": [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    m, o = dist_moments(), dist_other()
    s = prng.normal(SEED, "kl.dist.sample", (2, 4, 4, 4))
    d, other, det = DiagonalGaussianDistribution(m), DiagonalGaussianDistribution(o), DiagonalGaussianDistribution(m, deterministic=True)
    rec = {"moments": m, "other": o, "sample": s, "mean": d.mean, "logvar": d.logvar, "std": d.std, "var": d.var, "mode": d.mode(), "kl": d.kl(),
           "kl_other": d.kl(other), "nll": d.nll(s), "nll_dim1": d.nll(s, dims=[1]), "det.std": det.std, "det.var": det.var, "det.kl": det.kl(),
           "det.nll": det.nll(s), "det.mode": det.mode()}
    out.update({f"dist.{k}": v.numpy() for k, v in rec.items()})
    path = os.path.join(HERE, "f27_kl_first_stage.npz")
    np.savez_compressed(path, **out)
    print("wrote f27_kl_first_stage.npz", os.path.getsize(path), "bytes")
    with open(os.path.join(HERE, "f27_kl_names.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(tag)}: {json.dumps(v)}" for tag, v in names.items()) + "\n}\n")
    print("wrote f27_kl_names.json", os.path.getsize(os.path.join(HERE, "f27_kl_names.json")), "bytes")


if __name__ == "__main__":
    main()
