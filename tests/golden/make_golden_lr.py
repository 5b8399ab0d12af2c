#!/usr/bin/env python3
"""F28: learning-rate multipliers of the REFERENCE's own scheduler classes (ldm/lr_scheduler.py), called as `LambdaLR` calls them
(`schedule(n)`, n = 0, 1, ...), stored as float64. Three configurations (CONFIGS below, the constructor arguments the tests rebuild the
product's classes from):

  cosine   LambdaWarmUpCosineScheduler: 7 warm-up steps, half a cosine down to step 40, n up to 60 (past max_decay_steps: constant lr_min)
  cosine2  LambdaWarmUpCosineScheduler2, two cycles of 20 and 30 steps (warm-ups 5 and 3)
  linear   LambdaLinearScheduler, two cycles of 16 and 24 steps (warm-ups 4 and 6)

n runs over every integer from 0 to the configuration's last step, so each warm-up end, each cycle boundary (a step ON a boundary belongs to
the cycle that ends there) and the steps around them are all in the file.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lr.py

The reference tree is looked for at $STEDM_REFERENCE, else next to this repository's checkout (../reference).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "f28_lr_schedules.npz")

CONFIGS = {
    "cosine": ("LambdaWarmUpCosineScheduler", dict(warm_up_steps=7, lr_min=0.05, lr_max=1.0, lr_start=0.001, max_decay_steps=40), 60),
    "cosine2": ("LambdaWarmUpCosineScheduler2", dict(warm_up_steps=[5, 3], f_min=[0.1, 0.02], f_max=[1.0, 0.6], f_start=[1e-6, 0.05],
                                                      cycle_lengths=[20, 30]), 50),
    "linear": ("LambdaLinearScheduler", dict(warm_up_steps=[4, 6], f_min=[0.25, 0.01], f_max=[1.0, 0.5], f_start=[1e-6, 0.1],
                                             cycle_lengths=[16, 24]), 40),
}


def reference_dir() -> str:
    return os.environ.get("STEDM_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")


def generate() -> dict:
    """The fixture's arrays, computed from the reference (ImportError when its tree is not there)."""
    sys.dont_write_bytecode = True
    ref = reference_dir()
    if ref not in sys.path:
        sys.path.insert(0, ref)
    import ldm.lr_scheduler as rls
    out = {}
    for tag, (cls, params, last) in CONFIGS.items():
        sch = getattr(rls, cls)(**params)
        out[f"{tag}_n"] = np.arange(last + 1, dtype=np.int64)
        out[f"{tag}_f"] = np.asarray([float(sch.schedule(int(n))) for n in range(last + 1)], dtype=np.float64)
    return out


def main():
    np.savez_compressed(PATH, **generate())
    print(f"wrote f28_lr_schedules.npz  {os.path.getsize(PATH) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
