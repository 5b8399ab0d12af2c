"""References for gradient-norm clipping and the scheduled learning rate of the fused training step (tests/test_clip_lr_cpu.py,
tests/test_gpu_clip_lr.py): the total norm in float64, torch's coefficient formula in fp32, and three clipped AdamW + EMA steps built from
torch.nn.utils.clip_grad_norm_ and the oracle's optimizer restatement."""
from __future__ import annotations

import functools
import math
from typing import Iterable, List, Sequence

import numpy as np
import torch

EPS = np.float32(1e-6)          # clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6)
REL_NORM = 2.0 ** -22           # stedm_grad_norm: squares and sum exact to float64 rounding, ONE rounding to fp32 (2^-24) — bound of 2 fp32 ulp


def total_norm64(tensors: Iterable, grad_scale: float = 1.0) -> float:
    """grad_scale * sqrt(sum over every element of every tensor of g^2), squares and sums in float64 (math.fsum over the per-tensor sums)"""
    sums = []
    for t in tensors:
        a = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64).reshape(-1)
        sums.append(float(np.dot(a, a)))
    s = math.fsum(sums)
    return float(grad_scale) * math.sqrt(s)          # (an inf or NaN element makes the sum, hence the norm, inf or NaN)


def clip_coef32(norm_f32, max_norm: float) -> np.float32:
    """torch's coefficient from an fp32 norm: c = max_norm / (norm + 1e-6) in fp32, clamped to at most 1; NaN stays NaN; max_norm <= 0: 1"""
    if not max_norm > 0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm_f32) + EPS)
    return np.float32(1.0) if c >= np.float32(1.0) else np.float32(c)


def clip_grads_(grads: Sequence[torch.Tensor], max_norm: float):
    """The reference clip: float64 norm rounded once to fp32, torch's coefficient, every gradient multiplied by it in its own dtype.
    Returns (norm as np.float32, coefficient as np.float32)."""
    norm = np.float32(total_norm64(grads))
    coef = clip_coef32(norm, max_norm)
    for g in grads:
        g.mul_(float(coef))
    return norm, coef


TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)          # the TINY U-Net of tests/test_gpu_train.py

CLIP_STEP_SCALES = (0.01, 1.0, 0.1)       # gradients of step s: prng.normal(s, f"g{i}") * CLIP_STEP_SCALES[s - 1]


def clip_step_grads(shapes: Sequence[tuple], step: int) -> List[torch.Tensor]:
    from stedm_amd.utils import prng
    return [prng.normal(step, f"g{i}", tuple(sh)) * CLIP_STEP_SCALES[step - 1] for i, sh in enumerate(shapes)]


def clip_steps_max_norm(shapes: Sequence[tuple]) -> float:
    """a max_norm between the norm of step 1 (scale 0.01) and those of steps 2 and 3 (scales 1.0, 0.1): unit normals give about
    scale * sqrt(N), so 0.03 sqrt(N) leaves step 1 alone and clips the other two"""
    n = sum(int(np.prod(sh)) for sh in shapes)
    return 0.03 * math.sqrt(n)


def clipped_adamw_reference(params0: Sequence[torch.Tensor], dtype=torch.float32, lr: float = 1e-3, weight_decay: float = 0.01, steps: int = 3,
                            with_moments: bool = False):
    """Three steps of clip_grad_norm_ (on CPU tensors of `dtype`) + oracle AdamW + oracle EMA from the parameters params0, on the gradients of
    clip_step_grads. -> (parameters, EMA shadows, the norms clip_grad_norm_ returned); with_moments: + (AdamW's m, AdamW's v)"""
    from oracle import train as otrain
    shapes = [tuple(p.shape) for p in params0]
    mx = clip_steps_max_norm(shapes)
    p = [q.detach().cpu().to(dtype).clone() for q in params0]
    m = [torch.zeros_like(q) for q in p]
    v = [torch.zeros_like(q) for q in p]
    e = [q.clone() for q in p]
    norms = []
    for step in range(1, steps + 1):
        holders = [torch.nn.Parameter(q.clone()) for q in p]
        for h, g in zip(holders, clip_step_grads(shapes, step)):
            h.grad = g.to(dtype)
        norms.append(float(torch.nn.utils.clip_grad_norm_(holders, mx)))
        d = otrain.ema_decay(step)
        for i, h in enumerate(holders):
            otrain.adamw_step(p[i], h.grad, m[i], v[i], step, lr, weight_decay=weight_decay)
            otrain.ema_update(e[i], p[i], d)
    return (p, e, norms, m, v) if with_moments else (p, e, norms)


@functools.lru_cache(maxsize=None)
def _tiny_unet_clip_reference(dtype_name: str):
    from stedm_amd.unet import UNetModel
    from stedm_amd.utils import prng
    m = UNetModel(precision="parity", **TINY).eval()
    prng.fill_module_(m, seed=6)
    return clipped_adamw_reference([q for q in m.parameters()], getattr(torch, dtype_name), with_moments=True)


def tiny_unet_clip_reference(dtype_name: str = "float32"):
    """clipped_adamw_reference for the TINY U-Net of tests/test_gpu_train.py filled from seed 6, in module.parameters() order; computed
    once per process and shared (callers must not modify it)."""
    return _tiny_unet_clip_reference(dtype_name)[:3]


def tiny_unet_clip_moments(dtype_name: str = "float32"):
    """(m, v) of the same three steps (same computation, same cache)"""
    return _tiny_unet_clip_reference(dtype_name)[3:]
