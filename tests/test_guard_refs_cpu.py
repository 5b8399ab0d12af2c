"""CPU tier: the statements of tests/refs_guard.py held against torch's own fp32 -> fp16 cast, and the proof obligations of the planted
cases of tests/test_gpu_f16_guard.py (no kernel runs here):

  - the kernels' bit predicate on a stored word (bittrick16) is `not finite`, on all 65 536 fp16 bit patterns;
  - MAX, BELOW and OVER are the boundary, for both signs;
  - the block-uniform switch of the raw planes (sum of squares >= 4.0e9) can never miss: the smallest fp32 value whose cast is not finite
    has a square well above the threshold, and the switch's on-region still holds finite values (the GPU tier's "switch on, nothing to
    flag" case);
  - every convolution case that plants its value through the residual or the bias of a dyadic problem has an fp64 reference that is still a
    multiple of 1/64 below 2^18 with the planted element in place: the condition under which test_gpu_conv_exact.py demands bit equality."""
import numpy as np
import pytest
import torch

from tests import refs_conv as RC
from tests import refs_guard as RG
from tests import test_gpu_conv_exact as CE
from tests import test_gpu_f16_guard as TG

torch.set_grad_enabled(False)

CPU = torch.device("cpu")


def test_bit_predicate_is_not_finite_on_every_fp16_pattern():
    u = np.arange(1 << 16, dtype=np.uint16)
    v = torch.from_numpy(u.view(np.int16).copy()).view(torch.float16)
    assert np.array_equal(RG.bittrick16(u), (~torch.isfinite(v)).numpy())
    assert int(RG.bittrick16(u).sum()) == 2 * 1024          # +-inf and the 2 * 1023 NaN patterns
    # the kernels test two words per register: the packed form is the same predicate on each half
    w = (u.astype(np.uint32) << 16) | 0x3c00
    assert np.array_equal((((w & 0x7c007c00) + 0x04000400) & 0x80008000) != 0, RG.bittrick16(u))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_boundary_constants(sign):
    bits = lambda v: int(torch.tensor([sign * v], dtype=torch.float32).to(torch.float16).view(torch.int16)[0]) & 0x7fff
    assert bits(RG.MAX) == 0x7bff
    assert bits(RG.BELOW) == 0x7bff and RG.BELOW * 64 == round(RG.BELOW * 64) == 65520 * 64 - 1
    assert float(torch.tensor([RG.BELOW], dtype=torch.float32)[0]) == RG.BELOW          # exact in fp32
    assert bits(RG.OVER) == 0x7c00
    t = torch.tensor([sign * RG.MAX, sign * RG.BELOW, sign * RG.OVER, sign * float("inf"), float("nan"), 0.0])
    assert RG.over(t).tolist() == [False, False, True, True, True, False]
    # no fp32 value between BELOW and OVER is over: the fp32 neighbour below OVER still rounds to 65504
    below_over = float(torch.nextafter(torch.tensor([RG.OVER]), torch.tensor([0.0]))[0])
    assert RG.BELOW < below_over < RG.OVER and not bool(RG.over(torch.tensor([sign * below_over])))
    # bf16 has the exponent range of fp32: finite there
    assert bool(torch.isfinite(torch.tensor([sign * RG.OVER]).to(torch.bfloat16)).all())


def test_expected_bits_is_the_or_of_the_over_sites():
    fin = torch.tensor([1.0, RG.BELOW, -RG.MAX]); bad = torch.tensor([0.0, -RG.OVER])
    assert RG.expected_bits({RG.RAW: fin, RG.NORM: fin}) == 0
    assert RG.expected_bits({RG.RAW: bad, RG.NORM: fin, RG.CONV_OUT16: bad.double()}) == RG.RAW | RG.CONV_OUT16
    assert RG.expected_bits({RG.CAST: torch.tensor([float("nan")])}) == RG.CAST
    assert sorted([RG.RAW, RG.NORM, RG.CONV_OUT16, RG.S2D, RG.CAST, RG.CONV_SRC]) == [1, 2, 4, 8, 16, 32]


def test_sum_of_squares_switch_is_sound():
    f32 = lambda v: torch.tensor([v], dtype=torch.float32)
    sq = lambda v: float(f32(v) * f32(v))          # the fp32 square, as the statistics kernels form it
    # the smallest fp32 value whose cast is not finite is OVER itself
    assert bool(RG.over(f32(RG.OVER))) and not bool(RG.over(torch.nextafter(f32(RG.OVER), f32(0.0))))
    # its square clears the threshold by 7 %: an fp32 sum of squares that contains it (every term >= 0, relative error of a 256-term sum
    # <= 256 * 2^-24) cannot fall below 4.0e9
    assert sq(RG.OVER) > 1.07 * RG.SQ_SAFE and sq(RG.OVER) * (1 - 256 * 2.0 ** -24) > RG.SQ_SAFE
    # the smallest fp32 with x * x >= 4.0e9 is still finite in fp16: the on-region of the switch includes values it must not flag
    lo = f32(float(np.sqrt(RG.SQ_SAFE)))
    while sq(float(lo)) >= RG.SQ_SAFE:
        lo = torch.nextafter(lo, f32(0.0))
    first_on = torch.nextafter(lo, f32(1e9))
    assert sq(float(first_on)) >= RG.SQ_SAFE > sq(float(lo)) and not bool(RG.over(first_on))
    assert float(first_on) < RG.SWITCH_ON_FINITE < RG.MAX and sq(RG.SWITCH_ON_FINITE) >= RG.SQ_SAFE and not bool(RG.over(f32(RG.SWITCH_ON_FINITE)))


@pytest.mark.parametrize("value", [RG.OVER, RG.BELOW])
@pytest.mark.parametrize("case", TG.CONV16, ids=TG.CONV16_IDS)
def test_planted_residual_cases_stay_exact(case, value):
    """the residual-planted convolution cases (also the base of the conv_finish and composite cases): the reference with the planted
    elements is the value there, a multiple of 1/64 below 2^18 everywhere"""
    name, c, form, posfn = case
    o = CE._operands(CPU, c, 1)
    Ho, Wo = RC.out_hw(c["H"], c["W"], {"up2": "up"}.get(c["mode"], c["mode"]))
    for p in posfn(c["B"], Ho, Wo, c["cout"]):
        res, ref = TG.conv16_planted(c, o, [p], value)
        assert RG.plant_ok(ref) and float(ref[p]) == value
        assert float(res[p]) == value - float(o["ref_wo"][p]) and RG.plant_ok(res)          # the residual itself is exact in fp32
        assert int(RG.over(ref).sum()) == (1 if value == RG.OVER else 0)


@pytest.mark.parametrize("value", [RG.OVER, RG.BELOW])
@pytest.mark.parametrize("M,K,N,HD", [(49300, 128, 200, 0), (11 * 514, 128, 768, 256), (13 * 4098, 128, 384, 128)])
def test_planted_bias_cases_stay_exact(M, K, N, HD, value):
    """the bias-planted flat GEMMs (the lean 16-bit-only loops, the qkv epilogues with their q scale of 1/2)"""
    scales = (lambda n: 0.5 if n < HD else 1.0) if HD else None
    for plant in [(M - 1, N - 1), (0, 3), (M // 2 + 7, HD + 1)]:
        x, w, bias, ref = TG._flat_operands(CPU, M, K, N, [plant], value, scales)
        assert RG.plant_ok(ref) and RG.plant_ok(bias)
        stored = ref.clone()
        stored[:, :HD] *= 0.5
        assert float(stored[plant]) == value and float(stored[:, plant[1]].max()) == value
        assert bool((stored.float().double() == stored).all())          # exact in fp32 after the scale
        assert int(RG.over(stored).sum()) == (int((stored[:, plant[1]] == value).sum()) if value == RG.OVER else 0)
