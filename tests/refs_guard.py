"""The fp16 operand range guard (stedm_f16_guard_set, include/stedm_hip.h) stated in plain torch and numpy on the CPU: no kernel and no
project code is imported. Shared by tests/test_guard_refs_cpu.py (pins these statements against torch's own cast) and
tests/test_gpu_f16_guard.py (pins every kernel that rounds to fp16 against them).

The guard's definition: a kernel that rounds an fp32 value to an fp16 operand plane flags it iff the stored 16-bit word is an fp16 inf or
NaN, i.e. iff round-to-nearest-even of the fp32 value to fp16 is not finite. The boundary lies between two neighbouring multiples of 1/64:

  MAX   = 65504            the largest finite fp16 (0x7bff)
  BELOW = 65520 - 1/64     exact in fp32 (65520 * 64 - 1 < 2^24); the nearest fp16 is still 65504
  OVER  = 65520            the tie between 65504 (0x7bff, odd) and 2^16 (even): rounds to even = inf (0x7c00)

Both BELOW and OVER are multiples of 1/64 below 2^24 / 64, so a dyadic convolution (refs_conv.dyadic_ok) whose output is steered to one of
them through its residual or bias stores exactly that value in every summation order (plant_ok states the condition)."""
import numpy as np
import torch

MAX = 65504.0
BELOW = 65520.0 - 1.0 / 64.0
OVER = 65520.0

# site bits of the flag word, as include/stedm_hip.h documents them
RAW, NORM, CONV_OUT16, S2D, CAST, CONV_SRC = 1, 2, 4, 8, 16, 32

# the block-uniform switch of stedm_gn_apply16c's raw planes: the per-element test runs only when a channel partial's sum of squares
# reaches this value (gn_fold.hpp: STEDM_F16_SQ_SAFE)
SQ_SAFE = 4.0e9
# a value whose fp32 square passes SQ_SAFE while its fp16 cast is finite: the switch is on and nothing may be flagged
SWITCH_ON_FINITE = 63300.0


def over(x):
    """the guard's definition, elementwise: torch's round-to-nearest-even cast of the fp32 value to float16 is not finite"""
    return ~torch.isfinite(x.float().to(torch.float16))


def expected_bits(planes):
    """planes: {site bit: reference plane (any float dtype; fp64 references are rounded to fp32 first, as the kernels hold fp32)}.
    The OR of the site bits whose plane, cast by torch, holds a non-finite value."""
    bits = 0
    for site, ref in planes.items():
        if bool(over(ref).any()):
            bits |= int(site)
    return bits


def bittrick16(u16):
    """the kernels' predicate on a stored 16-bit word (csrc/common.hpp, f16_over2): exponent 11111 carries into the cleared sign position"""
    w = np.asarray(u16).astype(np.uint32)
    return (((w & 0x7c00) + 0x0400) & 0x8000) != 0


def plant_ok(ref64):
    """proof obligation of a planted dyadic case (the condition test_gpu_conv_exact.py asserts of its tier-1 references): every element of
    the fp64 reference is a multiple of 1/64 of magnitude < 2^24 / 64, so the kernel's fp32 sums are exact and it must store this value"""
    r = ref64.double() * 64
    return bool((r == r.round()).all()) and float(ref64.abs().max()) * 64 < 2 ** 24


def plant_residual(ref_wo, res, positions, target):
    """res' = res with res'[p] = target - (ref_wo[p]) at every position p = (b, y, x, n): ref_wo is the exact reference WITHOUT the
    residual, so the reference with res' is exactly `target` there"""
    res = res.clone()
    for p in positions:
        res[p] = float(target - ref_wo[p])
    return res


def plant_bias(ref_wo, bias, channels, target):
    """bias' = bias with bias'[n] = target - max over (b, y, x) of ref_wo[..., n]: ref_wo is the exact reference WITHOUT the bias, so
    the maximum of channel n becomes exactly `target` and nothing of it lies above"""
    bias = bias.clone()
    for n in channels:
        bias[n] = float(target - ref_wo[..., n].max())
    return bias
