#!/usr/bin/env python3
"""F23: the patch-distributed first stage through the REFERENCE's own code: `LatentDiffusion.get_weighting`, `get_fold_unfold`,
`decode_first_stage` and `encode_first_stage` (ldm/models/diffusion/ddpm.py:567-654, 709-766, 829-866), called as unbound functions on a
small receiver that carries `split_input_params`, `scale_factor = 0.7` and the toy first stage below. `ddpm.py` imports pytorch_lightning,
torchvision and taming, none of which this fixture needs: stub modules stand in for them (make_golden_ddpm._stub_imports).

The toy stage (ToyStage; the tests import it from here):
  decode(z) = nearest x uf upsample of a fixed 3 x C channel mix of z, plus 0.1 (y_in_tile / (th - 1) - x_in_tile / (tw - 1));
  encode(x) = avg_pool2d(x, df) through a fixed channel mix, plus the same ramp over its output tile.
The ramp depends on the position inside the crop, so a misplaced or mis-ordered crop shows in the stitched result.

Inputs come from stedm_amd.utils.prng (case_input), so the tests regenerate them; the file stores, per case, the stitched output, the
reference's weighting [th*tw, L] (get_weighting), its tile table (get_weighting with the tie-breaker off) and its crop table (delta_border over
the crop grid, clipped to the tie limits; ones without the tie-breaker). Every case has full coverage and minimum weights above 0, so the
reference's normalisation is strictly positive; the outputs are asserted finite before writing.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tiled.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stedm_amd.utils import prng  # noqa: E402

SEED = 23
SCALE_FACTOR = 0.7
_W = dict(clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
# name -> (input shape, encode?, output channels, split_input_params)
CASES = {
    "a": ((2, 3, 12, 16), False, 3, dict(ks=(8, 8), stride=(4, 4), vqf=2, patch_distributed_vq=True, tie_braker=False, **_W)),
    "b": ((2, 3, 12, 16), False, 3, dict(ks=(8, 8), stride=(4, 4), vqf=2, patch_distributed_vq=True, tie_braker=True, **_W)),
    "c": ((2, 4, 11, 13), False, 3, dict(ks=(5, 5), stride=(2, 2), vqf=1, patch_distributed_vq=True, tie_braker=False, **_W)),
    "d": ((2, 3, 24, 32), True, 3, dict(ks=(16, 16), stride=(8, 8), vqf=4, patch_distributed_vq=True, tie_braker=False, **_W)),
    "e": ((2, 3, 10, 10), False, 3, dict(ks=(64, 64), stride=(64, 64), vqf=2, patch_distributed_vq=True, tie_braker=False, **_W)),
}


def case_input(name: str) -> torch.Tensor:
    return prng.normal(SEED, f"tiled.{name}.x", CASES[name][0])


def case_split(name: str) -> dict:
    return dict(CASES[name][3])


class ToyStage:
    """A first stage with `.encode` / `.decode` on NCHW fp32 whose output depends on the position inside the crop."""

    def __init__(self, cin: int, cout: int, factor: int):
        self.factor = int(factor)
        self.mix = prng.normal(SEED, f"tiled.mix.{cin}.{cout}", (cout, cin)) * 0.5

    def _mix(self, x):
        m = self.mix.to(x.device, x.dtype)
        rows = []
        for o in range(m.shape[0]):
            acc = x[:, 0] * m[o, 0]
            for c in range(1, m.shape[1]):
                acc = acc + x[:, c] * m[o, c]
            rows.append(acc)
        return torch.stack(rows, 1)

    @staticmethod
    def _ramp(y):
        th, tw = y.shape[-2:]
        yy = torch.arange(th, dtype=y.dtype, device=y.device).view(th, 1) / (th - 1)
        xx = torch.arange(tw, dtype=y.dtype, device=y.device).view(1, tw) / (tw - 1)
        return y + 0.1 * (yy - xx)

    def decode(self, z):
        y = self._mix(z)
        f = self.factor
        if f > 1:
            y = y.repeat_interleave(f, dim=2).repeat_interleave(f, dim=3)
        return self._ramp(y)

    def encode(self, x):
        f = self.factor
        return self._ramp(self._mix(F.avg_pool2d(x, f) if f > 1 else x))


def case_stage(name: str) -> ToyStage:
    shape, _, cout, split = CASES[name]
    return ToyStage(shape[1], cout, split["vqf"])


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.environ.get("STEDM_REFERENCE", "/root/reference"))
    from tests.golden.make_golden_ddpm import _stub_imports
    _stub_imports()
    import ldm.models.diffusion.ddpm as rddpm

    torch.set_grad_enabled(False)
    LD = rddpm.LatentDiffusion

    class Recv:
        """The reference's tiling functions over a duck-typed self."""
        meshgrid = LD.meshgrid
        delta_border = LD.delta_border
        get_weighting = LD.get_weighting
        get_fold_unfold = LD.get_fold_unfold
        decode_first_stage = LD.decode_first_stage
        encode_first_stage = LD.encode_first_stage

        def __init__(self, stage, split):
            self.first_stage_model = stage
            self.split_input_params = split
            self.scale_factor = SCALE_FACTOR

    out = {}
    for name, (shape, encode, cout, _) in CASES.items():
        split = case_split(name)
        r = Recv(case_stage(name), split)
        x = case_input(name)
        y = r.encode_first_stage(x) if encode else r.decode_first_stage(x)
        assert torch.isfinite(y).all(), name
        h, w = shape[2:]
        ks = (min(split["ks"][0], h), min(split["ks"][1], w))
        st = (min(split["stride"][0], h), min(split["stride"][1], w))
        f = split["vqf"]
        Ly, Lx = (h - ks[0]) // st[0] + 1, (w - ks[1]) // st[1] + 1
        th, tw = (ks[0] // f, ks[1] // f) if encode else (ks[0] * f, ks[1] * f)
        assert tuple(y.shape) == (shape[0], cout, (Ly - 1) * (st[0] // f if encode else st[0] * f) + th,
                                  (Lx - 1) * (st[1] // f if encode else st[1] * f) + tw), (name, tuple(y.shape))
        weighting = r.get_weighting(th, tw, Ly, Lx, "cpu")[0]                                   # [th*tw, L]
        r.split_input_params = dict(split, tie_braker=False)
        w_tile = r.get_weighting(th, tw, 1, 1, "cpu")[0, :, 0].reshape(th, tw)
        if split["tie_braker"]:
            w_tie = torch.clip(r.delta_border(Ly, Lx), split["clip_min_tie_weight"], split["clip_max_tie_weight"]).reshape(-1)
        else:
            w_tie = torch.ones(Ly * Lx)
        assert weighting.min() > 0 and w_tile.dtype == torch.float32 and w_tie.dtype == torch.float32
        out[f"{name}_out"] = y.numpy()
        out[f"{name}_weighting"] = weighting.numpy()
        out[f"{name}_w_tile"] = w_tile.numpy()
        out[f"{name}_w_tie"] = w_tie.numpy()
        out[f"{name}_grid"] = np.asarray([Ly, Lx], dtype=np.int64)
        print(f"case {name}: crops {Ly} x {Lx}, tile {th} x {tw}, out {tuple(y.shape)}, max |out| {float(y.abs().max()):.4f}")
    path = os.path.join(HERE, "f23_tiled_first_stage.npz")
    np.savez_compressed(path, **out)
    print(f"wrote f23_tiled_first_stage.npz  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
