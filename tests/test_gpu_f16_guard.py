"""GPU tier (-m gpu): the fp16 operand range guard (stedm_f16_guard_set, include/stedm_hip.h), store loop by store loop. Every kernel that
rounds fp32 values to fp16 operand planes ORs a site bit into one device word when a stored word is inf / NaN; the sampling loops raise on
it. Here each such loop is driven on its own with ONE value planted at the boundary, and held against tests/refs_guard.py:

  OVER  = 65520 (the tie that rounds to inf): the word must equal the site's bit, the plane must hold inf exactly there;
  BELOW = 65520 - 1/64 (rounds to 65504): the word must stay 0, the plane holds 65504 there;
  OVER with bf16 planes: the word must stay 0, the plane is finite.

Protocol of every launch (_Guard): zero the word, fill the outputs with a sentinel, launch, synchronise; the WHOLE word equals the expected
OR of site bits (refs_guard.expected_bits of the reference planes), words 1 .. 3 stay 0, and the stored hi plane is torch's own cast of the
reference (int16 views, torch.equal). One launch per planted position: a second position could hide a lane that stores without testing.
An autouse fixture zeroes the word after every test, so that no later f16_guard_check inherits a bit. No assertion has a tolerance.

The convolution outputs are steered to the value through the residual or the bias of a dyadic problem (test_gpu_conv_exact.py, tier 1):
the fp64 reference with the planted element is a multiple of 1/64 below 2^18 (refs_guard.plant_ok, asserted here and on the CPU tier), so
the kernel must store exactly that value in any summation order. The GroupNorm planes are steered through gamma = 0: the value is beta.

Site -> case, from the source line of each f16_guard_commit and the rule that sends the case there:

  gn.hip:263   gn_apply16_kernel, CAST (gamma == NULL)          test_cast_plain_conversion[apply16-*]
  gn.hip:263   gn_apply16_kernel, NORM (gamma given)            test_norm_gn_apply16
  gn.hip:335   gn_chan_stats_kernel<CAST>                       test_cast_plain_conversion[chan_stats16-*]
  gn.hip:493/4 gn_apply16c_kernel (quad): c1 % 8 != 0           test_gn_apply16c_raw / _norm [quad]
  gn.hip:619/20 gn_apply16c_v8_kernel: C % 8 == 0, c1 % 8 == 0, 3 C floats <= 48 KiB; pixel runs (cb == 0: B * C / t < 768 for every
               admissible run t) [v8_pixel]; channel runs (HW <= 256, B * C / 128 >= 768: cb = 128) [v8_chan, v8_chan_bmod]; the hi + lo
               planes take this kernel too [v8_hilo]
  gn.hip:734/5 gn_apply16c_o8_kernel: stedm_gn_apply16c_x16; PAIR when C, c1 (and cb) are multiples of 16 [x16_pair_chan,
               x16_pair_pixel], else not [x16_unpaired]
  pack.hip:355 space_to_depth16_kernel                          test_s2d
  conv_igemm.hip:267  fp32-source loader (src1, no src16)       test_conv_src
  conv_igemm_dma.inc:363   128-row 1x1 LDS kernel (no fragment pack)          test_conv_out16[lds_1x1-side]
  conv_igemm_dma9.inc:288  128-row 3x3 LDS kernel (no fragment pack)          test_conv_out16[lds_3x3_partial_tile-side]
  conv_rs.inc:1425  generic row loop (fp32 output + side output)              test_conv_out16[rs3x3_ragged-side]
                    ... its scalar tail (cout % 4 != 0)                        test_conv_out16[rs3x3_tail-side]
                    fast path (out == NULL, statistics)                        test_conv_out16[rs3x3_ragged-only]
                    ... into a wider plane (out16_stride)                      test_conv_out16[rs3x3_ragged-wide]
                    sub-pixel scatter (CONV_UP_SUBPIXEL rows, 4 parities)      test_conv_out16[sub_full-side / -only]
  conv_rs.inc:1152  lean 8-channel loop (out == NULL, no res / emb / stats)   test_conv_out16_flat[lean_tiled], [lean_npers] under
                    STEDM_CONV_NO_NPERS
  conv_rs.inc:933   N-persistent form, 16-bit store from the accumulators     test_conv_out16_flat[lean_npers]
  conv_rs.inc:933   N-persistent form, q / k and v^T planes                   test_conv_out16_qkv[qkv_npers]
  conv_rs.inc:1122  qkv epilogue of the tiled form (q / k rows, v transposed) test_conv_out16_qkv[qkv_tiled], [qkv_npers] under
                    STEDM_CONV_NO_NPERS
  conv_rs.inc:1503  split-K reduce pass                                        test_conv_out16[splitk3x3_b2-side / -only]
                    ... as a call of its own (stedm_conv_finish)               test_conv_out16_finish
  conv_rs.inc:1064  LayerNorm epilogue (ln_after)                              test_norm_layernorm_epilogue
  conv_rs.inc:1426  riding GroupNorm, in-tile (gn_tile: the plain 3x3 kinds without a K split, i.e. tiles for 3/4 of the chip; HW divides
                    256; cout % 128 == 0; cpg % 4 == 0)                        test_norm_riding_groupnorm[in_tile]
                    ... cooperative across the tiles of a sample (gn_coop: HW = 2 .. 4 tiles, cout = 128, the words handed over)
                                                                               test_norm_riding_groupnorm[coop]
  conv_rs.inc:1558  riding GroupNorm on the split-K reduce pass                test_norm_riding_groupnorm[splitk]
  composite         conv (split K, chan_stats, one element at OVER) -> gn_apply16c(raw=): RAW from the epilogue's partials
                                                                               test_composite_conv_statistics_switch_the_raw_test_on

Where the dispatcher does not take the epilogue form of a riding GroupNorm, its separate stedm_gn_apply16c pass writes the planes: the
expected word is the same. The cooperative case keeps the fp32 output NaN-filled (gn_only) to know that the epilogue form ran.
"""
import math
import os

import pytest
import torch

from tests import refs_conv as RC
from tests import refs_guard as RG
from tests import test_gpu_conv_exact as CE

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
INF = float("inf")
FILL16 = 0x7e7e          # sentinel of every 16-bit output (a finite pattern in both formats: a skipped store shows in the plane comparison)
EMB_OFF = CE.EMB_OFF


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_word(dev):
    """the flag word is process-wide state: zero before and after every test of this file, so that no later f16_guard_check inherits a bit"""
    from stedm_amd import ops
    w = ops.f16_guard_enable()
    w.zero_()
    yield
    torch.cuda.synchronize()
    w.zero_()


# (id, precision, planted value): the three variants every case runs
VARIANTS = [pytest.param("f16", RG.OVER, id="over"), pytest.param("f16", RG.BELOW, id="below"), pytest.param("bf16", RG.OVER, id="bf16")]


def _dt(prec):
    return torch.float16 if prec in ("f16", "parity") else torch.bfloat16


def _cast16(ref, prec):
    """torch's own round-to-nearest-even cast of the (fp32-held) reference, as int16 words"""
    return ref.float().to(_dt(prec)).contiguous().view(torch.int16)


class _Guard:
    """one launch under the protocol: `with _Guard({site: reference plane}, prec) as g: launch`; then g.plane(stored, ref) for every
    16-bit output whose exact value is known"""

    def __init__(self, planes, prec, what=""):
        from stedm_amd import ops
        self.w = ops.f16_guard_enable()
        self.prec, self.what = prec, what
        # bf16 planes are not watched: the word stays 0 whatever they hold
        self.expected = RG.expected_bits({s: r.float().cpu() for s, r in planes.items()}) if _dt(prec) == torch.float16 else 0

    def __enter__(self):
        torch.cuda.synchronize()
        self.w.zero_()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        torch.cuda.synchronize()
        got = self.w.cpu().tolist()
        assert got[0] == self.expected, f"{self.what}: flag word {got[0]:#x}, expected {self.expected:#x}"
        assert got[1:] == [0, 0, 0], f"{self.what}: words 1..3 touched: {got[1:]}"
        return False

    def plane(self, stored, ref, had_nan=False):
        want = _cast16(ref, self.prec)
        assert stored.shape == want.shape, (stored.shape, want.shape)
        if had_nan:      # a NaN input: the payload of the stored NaN is the hardware's; NaN where NaN, equal bits elsewhere
            dt = _dt(self.prec)
            m = torch.isnan(want.view(dt))
            assert torch.equal(torch.isnan(stored.view(dt)), m), f"{self.what}: NaN positions differ"
            assert torch.equal(stored[~m], want[~m]), f"{self.what}: plane differs from torch's cast off the NaN"
            return
        if not torch.equal(stored, want):
            i = (stored != want).nonzero()
            raise AssertionError(f"{self.what}: plane differs from torch's cast of the reference at {len(i)} elements, first {i[0].tolist()}: "
                                 f"{int(stored[tuple(i[0])]) & 0xffff:#06x} != {int(want[tuple(i[0])]) & 0xffff:#06x}")


def _randn(shape, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(tuple(shape), generator=g) * std + mean


def _concat(x1, x2, bmod):
    """the virtual concat [x1 | x2] the GroupNorm kernels read: x2's sample b % bmod under bmod"""
    if x2 is None:
        return x1
    B = x1.shape[0]
    return torch.cat([x1, x2 if not bmod else x2.repeat(B // bmod, 1, 1, 1)], -1)


# ================================================================================================ CAST: the plain conversions
# (name, B, H, W, c1, c2, bmod). 20 x 20 x 96: gn_apply16 cuts a sample into slabs of ceil(16384 / 96) = 171 pixels (171 + 171 + 58),
# gn_chan_stats16 into 256-pixel slots (256 + 144): a ragged last slab either way
CAST_SHAPES = [("one_block", 1, 4, 4, 32, 0, 0), ("ragged", 2, 20, 20, 96, 0, 0), ("x2", 2, 20, 20, 64, 32, 0), ("x2_bmod", 4, 20, 20, 64, 32, 2)]
# the sign matters here: +-OVER, BELOW (both signs are covered on the CPU tier), inf and NaN inputs
CAST_VALUES = [pytest.param("f16", RG.OVER, id="over"), pytest.param("f16", RG.BELOW, id="below"), pytest.param("bf16", RG.OVER, id="bf16"),
               pytest.param("f16", -RG.OVER, id="neg_over"), pytest.param("f16", -RG.BELOW, id="neg_below"), pytest.param("f16", INF, id="inf"),
               pytest.param("f16", NAN, id="nan")]


def _cast_positions(B, H, W, c1, c2, bmod):
    """(tensor 1 | 2, index): first element, last element of the tensor, last pixel of sample 0 (its ragged last slab), the first pixel of
    the ragged slab; with x2: a channel of x2, and under bmod the last (shared) sample of x2"""
    first = max(0, H * W - 58)      # 400 = 171 + 171 + 58: the first pixel of gn_apply16's last slab at 96 channels
    pos = [(1, (0, 0, 0, 0)), (1, (B - 1, H - 1, W - 1, c1 - 1)), (1, (0, H - 1, W - 1, c1 // 2)), (1, (B - 1, first // W, first % W, 1))]
    if c2:
        B2 = bmod or B
        pos += [(2, (0, 1, 2, 3)), (2, (B2 - 1, H - 1, W - 1, c2 - 1))]
    return pos


@pytest.mark.parametrize("planes", ["hi", "hilo"])
@pytest.mark.parametrize("prec,value", CAST_VALUES)
@pytest.mark.parametrize("kernel,shape", [("apply16", s) for s in CAST_SHAPES] + [("chan_stats16", s) for s in CAST_SHAPES[:2]],
                         ids=lambda v: v if isinstance(v, str) else v[0])
def test_cast_plain_conversion(dev, kernel, shape, prec, value, planes):
    """stedm_gn_apply16 without gamma and stedm_gn_chan_stats16: bit CAST, single-product and hi + lo forms"""
    from stedm_amd import ops
    name, B, H, W, c1, c2, bmod = shape
    pr = ops.Precision(ops.Precision.parse(prec).mm_dtype, 3 if planes == "hilo" else 1)
    x1_0 = _randn((B, H, W, c1), 1, 3.0)
    x2_0 = _randn((bmod or B, H, W, c2), 2, 3.0) if c2 else None
    for which, idx in _cast_positions(B, H, W, c1, c2, bmod):
        x1, x2 = x1_0.clone(), None if x2_0 is None else x2_0.clone()
        (x1 if which == 1 else x2)[idx] = value
        ref = _concat(x1, x2, bmod)
        hi = torch.full((B, H, W, c1 + c2), FILL16, dtype=torch.int16, device=dev)
        lo = torch.full_like(hi, FILL16) if planes == "hilo" else None
        d1, d2 = x1.to(dev), None if x2 is None else x2.to(dev)
        with _Guard({RG.CAST: ref}, prec, f"{kernel} {name} x{which}{list(idx)}") as g:
            if kernel == "apply16":
                ops.gn_apply16(d1, d2, hi, lo, pr, x2_bmod=bmod)
            else:
                cs = torch.full((B, ops.gn_chan_nslab(H * W), c1, 2), NAN, device=dev)
                ops.gn_chan_stats16(d1, cs, hi, lo, pr)
        g.plane(hi, ref.to(dev), had_nan=math.isnan(value))
        if prec == "f16":
            assert g.expected == (0 if abs(value) == RG.BELOW else RG.CAST)      # (the reference's own answer, stated once in full)


def test_guard_switched_off_leaves_the_word_alone(dev):
    """stedm_f16_guard_set(NULL): the same conversion writes the same plane and never touches the word"""
    from stedm_amd import _lib, ops
    pr = ops.Precision.parse("f16")
    x = _randn((2, 20, 20, 96), 3, 3.0)
    x[1, 19, 19, 95] = RG.OVER
    d = x.to(dev)
    on = torch.full((2, 20, 20, 96), FILL16, dtype=torch.int16, device=dev); off = torch.full_like(on, FILL16)
    with _Guard({RG.CAST: x}, "f16", "guard on") as g:
        ops.gn_apply16(d, None, on, None, pr)
    assert g.expected == RG.CAST
    w = ops.f16_guard_enable()
    w.zero_()
    try:
        _lib.check(_lib.lib().stedm_f16_guard_set(None), "stedm_f16_guard_set")
        ops.gn_apply16(d, None, off, None, pr)
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.lib().stedm_f16_guard_set(w.data_ptr()), "stedm_f16_guard_set")
    assert w.cpu().tolist() == [0, 0, 0, 0], "the word was written with the guard switched off"
    assert torch.equal(on, off)
    with _Guard({RG.CAST: x}, "f16", "guard on again"):      # restored: the same launch flags again
        ops.gn_apply16(d, None, off, None, pr)


# ================================================================================================ NORM: stedm_gn_apply16 with gamma
# gamma[c] = 0 makes every value of channel c exactly beta[c] ((x - mean) * rstd * 0 + beta, finite operands): beta = 7e4 is beyond the
# range, beta = MAX stores 65504 (act = 0)
NORM_VARIANTS = [pytest.param("f16", 7.0e4, id="over"), pytest.param("f16", RG.MAX, id="below"), pytest.param("bf16", 7.0e4, id="bf16")]


def _check_norm_planes(g, planes16, prec, chans, beta_c, what):
    """the planted channels hold torch's cast of beta everywhere; every other value is finite (their exact value is not this test's)"""
    dt = _dt(prec)
    v = planes16.view(dt)
    want = torch.tensor(beta_c, dtype=torch.float32).to(dt)
    rest = torch.ones(v.shape[-1], dtype=torch.bool, device=v.device)
    for c in chans:
        assert bool((v[..., c] == want).all()) if bool(torch.isfinite(want)) else bool(torch.isinf(v[..., c]).all() and (v[..., c] > 0).all()), \
            f"{what}: channel {c} is not torch's cast of beta = {beta_c}"
        rest[c] = False
    assert bool(torch.isfinite(v[..., rest].float()).all()), f"{what}: a non-finite value outside the planted channels"


@pytest.mark.parametrize("prec,beta_c", NORM_VARIANTS)
@pytest.mark.parametrize("B,H,W,c1,c2,bmod", [(1, 4, 4, 32, 0, 0), (2, 20, 20, 96, 0, 0), (4, 20, 20, 64, 32, 2)])
def test_norm_gn_apply16(dev, B, H, W, c1, c2, bmod, prec, beta_c):
    """stedm_gn_apply16 with gamma (statistics from stedm_gn_stats): bit NORM, never CAST"""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    C = c1 + c2
    d1 = _randn((B, H, W, c1), 4, 1.7, 0.3).to(dev)
    d2 = _randn((bmod or B, H, W, c2), 5, 0.6, -0.2).to(dev) if c2 else None
    stats = torch.empty((B * ops.gn_nslab(C, H * W) * 32 * 2,), dtype=torch.float64, device=dev)
    ops.gn_stats(d1, d2, stats, 32, bmod)
    for c in (0, C - 1):
        gamma = _randn((C,), 6, 0.1, 1.0); beta = _randn((C,), 7, 0.1)
        gamma[c] = 0.0; beta[c] = beta_c
        hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
        with _Guard({RG.NORM: torch.tensor([beta_c])}, prec, f"gn_apply16 gamma, channel {c}") as g:
            ops.gn_apply16(d1, d2, hi, None, pr, gamma.to(dev), beta.to(dev), 1e-5, 32, 0, stats, bmod)
        _check_norm_planes(g, hi, prec, [c], beta_c, f"gn_apply16 gamma, channel {c}")


# ================================================================================================ S2D
@pytest.mark.parametrize("prec,value", VARIANTS)
def test_s2d(dev, prec, value):
    """stedm_space_to_depth16, (3, 8, 8, 32): pixel (2y + py, 2x + px) lands in channel block py * 2 + px; one planted pixel per block
    (each of the four parities), and the last pixel of the last sample"""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    B, H, W, C = 3, 8, 8, 32
    x0 = _randn((B, H, W, C), 8, 3.0)
    fold = lambda t: t.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)
    for idx in [(0, 0, 0, 0), (1, 2, 5, 7), (1, 5, 2, 31), (0, 3, 3, 16), (B - 1, H - 1, W - 1, C - 1)]:
        x = x0.clone()
        x[idx] = value
        ref = fold(x)
        hi = torch.full((B, H // 2, W // 2, 4 * C), FILL16, dtype=torch.int16, device=dev)
        with _Guard({RG.S2D: ref}, prec, f"space_to_depth16 {list(idx)}") as g:
            ops.space_to_depth16(x.to(dev), hi, None, pr)
        g.plane(hi, ref.to(dev))
        b, y, xx, c = idx      # the planted word sits in block (y % 2) * 2 + (x % 2) of low-res pixel (y / 2, x / 2)
        assert int(hi[b, y // 2, xx // 2, ((y % 2) * 2 + xx % 2) * C + c]) == int(_cast16(torch.tensor([value]), prec)[0])


# ================================================================================================ RAW and NORM: stedm_gn_apply16c
# (id, B, H, W, c1, c2, bmod, form). The form each shape takes, by the rules of gn_apply16c_launch (gn.hip):
GN16C = [
    # c1 = 36 is no multiple of 8 -> the quad kernel (gn_apply16c_kernel); cpg = 2: the per-element group lookup
    ("quad", 2, 8, 8, 36, 28, 0, "f32"),
    # C = 640, c1 = 512: multiples of 8, table 7.5 KiB -> the 8-wide kernel; B * C / t >= 768 for no run t -> cb = 0, pixel runs (1 pixel per block)
    ("v8_pixel", 2, 16, 16, 512, 128, 0, "f32"),
    # HW = 64 <= 256, C = 512, cpg = 16: t = 128 gives 200 * 4 = 800 >= 768 blocks -> cb = 128: four channel-run blocks of 8 groups per sample
    ("v8_chan", 200, 8, 8, 256, 256, 0, "f32"),
    ("v8_chan_bmod", 200, 8, 8, 256, 256, 100, "f32"),
    # hi + lo planes through the 8-wide kernel
    ("v8_hilo", 2, 16, 16, 512, 128, 0, "hilo"),
    # stedm_gn_apply16c_x16 -> the octet kernel. C = 2048, c1 = 1024 multiples of 16, HW = 64, cpg = 64: t = 128 gives 48 * 16 = 768 -> cb = 128, PAIR
    ("x16_pair_chan", 48, 8, 8, 1024, 1024, 24, "x16"),
    # HW = 1024 > 256 -> pixel runs; C = 256, c1 = 128 multiples of 16 -> PAIR
    ("x16_pair_pixel", 2, 32, 32, 128, 128, 0, "x16"),
    # c1 = 136 is a multiple of 8 but not of 16 -> no PAIR (C = 256 keeps 32 groups)
    ("x16_unpaired", 2, 8, 8, 136, 120, 0, "x16"),
]
GN16C_IDS = [c[0] for c in GN16C]


def _gn16c_setup(dev, case):
    from stedm_amd import ops
    name, B, H, W, c1, c2, bmod, form = case
    x1 = _randn((B, H, W, c1), 11, 1.7, 0.3)
    x2 = _randn((bmod or B, H, W, c2), 12, 0.6, -0.2)
    gamma = _randn((c1 + c2,), 13, 0.1, 1.0); beta = _randn((c1 + c2,), 14, 0.1)
    ns = ops.gn_chan_nslab(H * W)
    return x1, x2, gamma, beta, ns


def _gn16c_run(dev, case, prec, x1, x2, gamma, beta, act, planes, what):
    """partials from stedm_gn_chan_stats exactly as test_gn_chan_stats_apply16c builds them; the launch of the case's form under the protocol.
    planes: {site: reference} of this launch. Returns (guard, normalised plane, raw plane)."""
    from stedm_amd import ops
    name, B, H, W, c1, c2, bmod, form = case
    pr = ops.Precision(ops.Precision.parse(prec).mm_dtype, 3 if form == "hilo" else 1)
    C, ns = c1 + c2, ops.gn_chan_nslab(H * W)
    d1, d2 = x1.to(dev), x2.to(dev)
    cs1 = torch.full((B, ns, c1, 2), NAN, device=dev); ops.gn_chan_stats(d1, cs1)
    cs2 = torch.full((d2.shape[0], ns, c2, 2), NAN, device=dev); ops.gn_chan_stats(d2, cs2)
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
    raw = torch.full_like(hi, FILL16)
    lo = torch.full_like(hi, FILL16) if form == "hilo" else None
    rlo = torch.full_like(hi, FILL16) if form == "hilo" else None
    g_, b_ = gamma.to(dev), beta.to(dev)
    if form == "x16":      # the x1 half sits in the raw plane as the 16-bit values its producer stored (that launch's CONV_OUT16, not this one's)
        raw.view(_dt(prec))[..., :c1] = d1.to(_dt(prec))
    with _Guard(planes, prec, what) as g:
        if form == "x16":
            ops.gn_apply16c_x16(c1, cs1, d2, cs2, hi, raw, pr, g_, b_, 1e-5, 32, act, bmod)
        else:
            ops.gn_apply16c(d1, cs1, d2, cs2, hi, lo, pr, g_, b_, 1e-5, 32, act, bmod, raw=(raw, rlo))
    return g, hi, raw


def _gn16c_raw_positions(case):
    """(tensor, index): in x1 (first element: a group of the FIRST channel block), in x2 (last channel of the last pixel: a group of the LAST
    channel block), mid-tensor in both, and under bmod the last sample of x2, which the samples b = bmod - 1 (mod bmod) share.
    X16: x2 only - the x1 half was rounded by its producer."""
    name, B, H, W, c1, c2, bmod, form = case
    B2 = bmod or B
    pos = [(2, (0, 0, 0, 0)), (2, (B2 - 1, H - 1, W - 1, c2 - 1)), (2, (B2 // 2, H // 2, 1, c2 // 2 + 1))]
    if form != "x16":
        pos += [(1, (0, 0, 0, 0)), (1, (B - 1, H - 1, W - 1, c1 - 1)), (1, (B // 2, 1, W // 2, c1 // 2 + 1))]
    return pos


@pytest.mark.parametrize("prec,value", VARIANTS + [pytest.param("f16", RG.SWITCH_ON_FINITE, id="switch_on_finite")])
@pytest.mark.parametrize("case", GN16C, ids=GN16C_IDS)
def test_gn_apply16c_raw(dev, case, prec, value):
    """the raw planes of stedm_gn_apply16c / _x16: bit RAW. The per-element test hides behind the block-uniform switch `maybe_over` (some
    channel partial of the block's groups has a sum of squares >= 4.0e9): a block that consults the wrong groups' or the wrong sample's
    partials misses the value. 63300 switches the test on (63300^2 > 4.0e9) and is finite in fp16: no bit. The normalised planes stay
    far inside the range (|x^| <= sqrt(n)), so the word is RAW alone."""
    name, B, H, W, c1, c2, bmod, form = case
    x1_0, x2_0, gamma, beta, _ = _gn16c_setup(dev, case)
    for which, idx in _gn16c_raw_positions(case):
        x1, x2 = x1_0.clone(), x2_0.clone()
        (x1 if which == 1 else x2)[idx] = value
        ref = _concat(x1, x2, bmod)
        if form == "x16":      # the x1 half of the raw plane is input: what this launch rounds is x2
            watched = _concat(x1[..., :0], x2, bmod)
            ref = torch.cat([x1.to(_dt(prec)).float(), watched], -1)
        else:
            watched = ref
        what = f"gn_apply16c {name} x{which}{list(idx)} = {value}"
        g, hi, raw = _gn16c_run(dev, case, prec, x1, x2, gamma, beta, 1, {RG.RAW: watched}, what)
        g.plane(raw, ref.to(dev))
        assert bool(torch.isfinite(hi.view(_dt(prec)).float()).all()), f"{what}: the normalised plane is not finite"
        if prec == "f16":
            assert g.expected == (RG.RAW if value == RG.OVER else 0)


@pytest.mark.parametrize("prec,beta_c", NORM_VARIANTS)
@pytest.mark.parametrize("case", GN16C, ids=GN16C_IDS)
def test_gn_apply16c_norm(dev, case, prec, beta_c):
    """the normalised planes of stedm_gn_apply16c / _x16: bit NORM, behind the switch `norm_over` (sqrt(n) |gamma| + |beta| >= 65504 for a
    channel of the block). gamma = 0 / beta on a channel of each half (the first and the last channel block)."""
    name, B, H, W, c1, c2, bmod, form = case
    x1, x2, gamma0, beta0, _ = _gn16c_setup(dev, case)
    for c in (1, c1 + c2 - 2):
        gamma, beta = gamma0.clone(), beta0.clone()
        gamma[c] = 0.0; beta[c] = beta_c
        what = f"gn_apply16c {name} gamma[{c}] = 0, beta = {beta_c}"
        g, hi, raw = _gn16c_run(dev, case, prec, x1, x2, gamma, beta, 0, {RG.NORM: torch.tensor([beta_c])}, what)
        _check_norm_planes(g, hi, prec, [c], beta_c, what)


@pytest.mark.parametrize("case", GN16C, ids=GN16C_IDS)
def test_gn_apply16c_norm_switch_on_nothing_to_flag(dev, case):
    """gamma[c] = 1.01 * 65504 / sqrt(cpg * HW) on normal data: the bound sqrt(n) |gamma| + |beta| passes 65504 and switches the per-element
    test on; the actual values (a few standard deviations times gamma) stay far below: no bit"""
    name, B, H, W, c1, c2, bmod, form = case
    x1, x2, gamma, beta, _ = _gn16c_setup(dev, case)
    cpg = (c1 + c2) // 32
    c = c1 + c2 - 2
    gamma[c] = 1.01 * 65504.0 / math.sqrt(cpg * H * W)
    assert math.sqrt(cpg * H * W) * float(gamma[c]) + abs(float(beta[c])) >= 65504.0
    # |x^| of normal data stays below 8 (8 standard deviations): the plane's values below 8 * gamma + 1 < 65504
    assert 8.0 * float(gamma[c]) + 1.0 < 65504.0
    g, hi, raw = _gn16c_run(dev, case, "f16", x1, x2, gamma, beta, 0, {}, f"gn_apply16c {name} bound on, values small")
    assert g.expected == 0
    assert bool(torch.isfinite(hi.view(torch.float16).float()).all())


# ================================================================================================ CONV_SRC: the fp32-source loader
# (B, H, W, c1, c2, cout, bmod): _conv_case-style launches of test_gpu_kernels.py (src1 / src2 fp32, no src16): only the flag word is asserted,
# the operand never leaves LDS
SRC_CASES = [(2, 8, 8, 64, 0, 64, 0), (4, 8, 8, 128, 128, 64, 2)]


def _src_launch(dev, pr, x1, x2, bmod, cout, scale=None, shift=None):
    from stedm_amd import ops
    B, H, W, c1 = x1.shape
    cin = c1 + (0 if x2 is None else x2.shape[-1])
    w = _randn((cout, cin, 3, 3), 21, 1.0 / math.sqrt(cin * 9)).to(dev)
    whi, wlo = ops.pack_conv_weight(w, pr)
    out = torch.full((B, H, W, cout), NAN, device=dev)
    ops.conv_igemm(x1.to(dev), whi, wlo, out, prec=pr, ks=3, src2=None if x2 is None else x2.to(dev), src2_bmod=bmod,
                   scale=None if scale is None else scale.to(dev), shift=None if shift is None else shift.to(dev),
                   bias=_randn((cout,), 22, 0.05).to(dev))
    return out


@pytest.mark.parametrize("prec,value", VARIANTS)
@pytest.mark.parametrize("B,H,W,c1,c2,cout,bmod", SRC_CASES)
def test_conv_src(dev, B, H, W, c1, c2, cout, bmod, prec, value):
    """the fp32-source loader (conv_igemm.hip): bit CONV_SRC for an interior pixel, a corner pixel, an src2 channel and the shared src2
    sample; with scale / shift, a SMALL source whose shift carries the operand over: the operand, not the input, is what is tested"""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    x1_0 = _randn((B, H, W, c1), 23)
    x2_0 = _randn((bmod or B, H, W, c2), 24) if c2 else None
    pos = [(1, (0, 3, 4, 5)), (1, (B - 1, H - 1, W - 1, c1 - 1)), (1, (B - 1, 0, 0, 0))]
    if c2:
        pos += [(2, (0, 2, 2, 1)), (2, (bmod - 1, H - 1, W - 1, c2 - 1))]
    for which, idx in pos:
        x1, x2 = x1_0.clone(), None if x2_0 is None else x2_0.clone()
        (x1 if which == 1 else x2)[idx] = value
        with _Guard({RG.CONV_SRC: _concat(x1, x2, bmod)}, prec, f"conv fp32 source x{which}{list(idx)}") as g:
            out = _src_launch(dev, pr, x1, x2, bmod, cout)
        assert g.expected == (RG.CONV_SRC if (prec, value) == ("f16", RG.OVER) else 0)
        assert g.expected != 0 or bool(torch.isfinite(out).all()), "output elements left unwritten"
    # scale / shift: channel c of sample b is zero in the source, the operand is fma(0, scale, shift) = shift exactly
    C = c1 + c2
    for b, c in [(0, 3), (B - 1, C - 1)]:
        x1, x2 = x1_0.clone(), None if x2_0 is None else x2_0.clone()
        if c < c1:
            x1[b, :, :, c] = 0.0
        else:
            x2[b % bmod if bmod else b, :, :, c - c1] = 0.0
        scale = _randn((B, C), 25, 0.2, 1.0); shift = _randn((B, C), 26, 0.2)
        shift[b, c] = value
        operand = _concat(x1, x2, bmod) * scale[:, None, None, :] + shift[:, None, None, :]
        operand[b, :, :, c] = value      # exactly: 0 * scale + shift
        with _Guard({RG.CONV_SRC: operand}, prec, f"conv fp32 source, shift[{b}][{c}] = {value}") as g:
            _src_launch(dev, pr, x1, x2, bmod, cout, scale, shift)
        assert g.expected == (RG.CONV_SRC if (prec, value) == ("f16", RG.OVER) else 0)


# ================================================================================================ CONV_OUT16: the 16-bit output epilogues
def _base(name, *a, **k):
    return dict(CE.case(name, *a, **k).values[0])


def _ends(B, Ho, Wo, N):
    """first element; the last valid row of the (ragged) last M tile in the last column of the (masked) last N tile; an interior element"""
    return [(0, 0, 0, 0), (B - 1, Ho - 1, Wo - 1, N - 1), (B // 2, 1, 2, N // 2 + 1)]


def _parities(B, Ho, Wo, N):
    """one element per output parity (py, px) of the sub-pixel scatter, the last one in the last row of the last sample"""
    return [(0, 0, 0, 0), (1, 2, 5, 7), (B // 2, 5, 2, N // 2), (B - 1, Ho - 1, Wo - 1, N - 1)]


# (id, base case of test_gpu_conv_exact.py (same shapes), form, positions). form: side = fp32 output + 16-bit side output; only = the 16-bit
# output alone (statistics still written); wide = alone, into channels [0, cout) of a plane 32 channels wider (out16_stride)
CONV16 = [
    ("lds_1x1-side", _base("lds_1x1", 3, 4, 4, 128, 96, ks=1, pack="", rs=False), "side", _ends),
    ("lds_3x3_partial_tile-side", _base("lds_3x3_partial_tile", 3, 8, 8, 64, 96, pack="", rs=False), "side", _ends),
    ("rs3x3_ragged-side", _base("rs3x3_ragged", 771, 8, 8, 32, 96), "side", _ends),
    ("rs3x3_ragged-only", _base("rs3x3_ragged", 771, 8, 8, 32, 96), "only", _ends),
    ("rs3x3_ragged-wide", _base("rs3x3_ragged", 771, 8, 8, 32, 96), "wide", _ends),
    # cout = 94: the last lane of a row owns channels 92, 93 only (nv = 2): the scalar tail of the generic row loop
    ("rs3x3_tail-side", _base("rs3x3_tail", 771, 8, 8, 32, 94), "side", lambda B, Ho, Wo, N: _ends(B, Ho, Wo, N) + [(B - 1, Ho - 1, Wo - 1, N - 2)]),
    ("sub_full-side", _base("sub_full", 193, 8, 8, 32, 96, mode="up2", stats="parity"), "side", _parities),
    ("sub_full-only", _base("sub_full", 193, 8, 8, 32, 96, mode="up2", stats="parity"), "only", _parities),
    ("splitk3x3_b2-side", _base("splitk3x3_b2", 2, 8, 8, 1024, 1024, ws=True), "side", _ends),
    ("splitk3x3_b2-only", _base("splitk3x3_b2", 2, 8, 8, 1024, 1024, ws=True), "only", _ends),
]
CONV16_IDS = [c[0] for c in CONV16]


def conv16_reference(c, o):
    """(exact fp64 reference without the residual, the residual) of a dyadic case, on the device of the operands"""
    if "ref_wo" not in o:      # computed once per case, shared by its positions and variants, never changed
        conv = (lambda a_, w_: RC.conv_ref(a_, w_, "up", 3)) if c["mode"] == "up2" else CE._conv_fn(c)
        o["ref_wo"] = CE._reference(c, o["a"].double(), RC.otc(o["w"]).double(), conv, dict(o, res=None))
    return o["ref_wo"], o["res"]


def conv16_planted(c, o, positions, value):
    """the residual with `value` planted at every position, and the exact reference of the launch that uses it"""
    ref_wo, res = conv16_reference(c, o)
    res_p = RG.plant_residual(ref_wo, res, positions, value)
    return res_p, ref_wo + res_p.double()


def _conv16_launch(dev, c, prec, o, res, form):
    """the launch of test_gpu_conv_exact._launch, for one form of the 16-bit output. Returns (fp32 out or None, 16-bit plane [.., cout])"""
    from stedm_amd import ops
    from stedm_amd._lib import CONV_S1, CONV_UP_SUBPIXEL
    pr = ops.Precision.parse(prec)
    B, H, W, cin, cout, ks, mode, pack = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["ks"], c["mode"], c["pack"]
    Ho, Wo = RC.out_hw(H, W, {"up2": "up"}.get(mode, mode))
    hi = torch.empty((B, H, W, cin), dtype=torch.int16, device=dev)
    ops.gn_apply16(o["a"], None, hi, None, pr)
    if mode == "up2":
        whi, wlo = ops.pack_conv_weight_up(o["w"], pr)
        wf = ops.pack_conv_weight_up_frag(o["w"], pr) if "f" in pack else None
        nslab = 4 * ops.gn_chan_nslab(H * W)
    else:
        whi, wlo = ops.pack_conv_weight(o["w"], pr)
        wf = ops.pack_conv_weight_frag(o["w"], pr) if "f" in pack else None
        nslab = ops.gn_chan_nslab(Ho * Wo)
    out = torch.full((B, Ho, Wo, cout), NAN, device=dev) if form == "side" else None
    wide = cout + (32 if form == "wide" else 0)
    o16 = torch.full((B, Ho, Wo, wide), FILL16, dtype=torch.int16, device=dev)
    k = dict(prec=pr, ks=ks, mode=CONV_UP_SUBPIXEL if mode == "up2" else CONV_S1, src16=(hi, None), bias=o["bias"], emb=o["emb"],
             emb_offset=EMB_OFF if o["emb"] is not None else 0, emb_bstride=0 if o["emb"] is None else o["emb"].shape[1], res=res, w_frag=wf,
             chan_stats=torch.full((B, nslab, cout, 2), NAN, device=dev) if c["stats"] else None,
             ws=torch.full((16 * B * Ho * Wo * cout,), NAN, device=dev) if c["ws"] else None, out16=(o16, None))
    if form == "wide":
        k.update(out16_stride=wide, cout=cout)
    assert ops.conv_igemm(None, whi, wlo, out, query_rs=True, **k) == c["rs"], f"register-streamed kernel expected: {c['rs']}"
    ops.conv_igemm(None, whi, wlo, out, **k)
    assert k["ws"] is None or not bool(torch.isnan(k["ws"]).all()), "the K split did not run: the workspace is untouched"
    if form == "wide":
        assert bool((o16[..., cout:] == FILL16).all()), "the other channels of the wide plane were written"
    return out, o16[..., :cout]


@pytest.mark.parametrize("prec,value", VARIANTS)
@pytest.mark.parametrize("case", CONV16, ids=CONV16_IDS)
def test_conv_out16(dev, case, prec, value):
    """every 16-bit output epilogue of stedm_conv_igemm that a residual can steer: bit CONV_OUT16, the plane torch's cast of the exact value"""
    name, c, form, posfn = case
    o = CE._operands(dev, c, 1)
    RC.dyadic_ok(4 * c["cin"] + 3, wmax=4.0) if c["mode"] == "up2" else RC.dyadic_ok(c["ks"] ** 2 * c["cin"] + 4)
    Ho, Wo = RC.out_hw(c["H"], c["W"], {"up2": "up"}.get(c["mode"], c["mode"]))
    for p in posfn(c["B"], Ho, Wo, c["cout"]):
        res, ref = conv16_planted(c, o, [p], value)
        assert RG.plant_ok(ref) and float(ref[p]) == value
        with _Guard({RG.CONV_OUT16: ref}, prec, f"conv {name} {list(p)}") as g:
            out, o16 = _conv16_launch(dev, c, prec, o, res, form)
        g.plane(o16.contiguous(), ref)
        assert out is None or torch.equal(out.double(), ref)
        if prec == "f16":
            assert g.expected == (RG.CONV_OUT16 if value == RG.OVER else 0)


@pytest.mark.parametrize("prec,value", VARIANTS)
def test_conv_out16_finish(dev, prec, value):
    """stedm_conv_finish on its own, after conv_igemm(partials=True): the reduce pass writes the 16-bit output"""
    from stedm_amd import ops
    c = _base("splitk3x3_b2", 2, 8, 8, 1024, 1024, ws=True)
    o = CE._operands(dev, c, 1)
    pr = ops.Precision.parse(prec)
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    hi = torch.empty((B, H, W, cin), dtype=torch.int16, device=dev)
    ops.gn_apply16(o["a"], None, hi, None, pr)
    whi, _ = ops.pack_conv_weight(o["w"], pr)
    wf = ops.pack_conv_weight_frag(o["w"], pr)
    ws = torch.full((16 * B * H * W * cout,), NAN, device=dev)
    shape = torch.empty((B, H, W, cout), device=dev)
    n = ops.conv_igemm(None, whi, None, shape, prec=pr, src16=(hi, None), ws=ws, partials=True, w_frag=wf)
    assert n >= 2, f"the dispatcher left {n} partial(s)"
    for p in _ends(B, H, W, cout):
        res, ref = conv16_planted(c, o, [p], value)
        assert RG.plant_ok(ref)
        out = torch.full((B, H, W, cout), NAN, device=dev)
        o16 = torch.full((B, H, W, cout), FILL16, dtype=torch.int16, device=dev)
        with _Guard({RG.CONV_OUT16: ref}, prec, f"conv_finish {list(p)}") as g:
            ops.conv_finish(ws, n, out, prec=pr, bias=o["bias"], emb=o["emb"], emb_offset=EMB_OFF, emb_bstride=o["emb"].shape[1], res=res, out16=(o16, None))
        g.plane(o16, ref)
        assert torch.equal(out.double(), ref)


# ---- flat GEMMs whose epilogue admits no residual: the value goes through the bias. Row r of the input is sign(w[n]), so that out[r][n] =
# sum |w[n]| is the largest value channel n can take, and bias[n] = target - sum |w[n]| puts exactly `target` there and nothing above it
def _flat_operands(dev, M, K, N, plants, value, scales=None):
    """plants: [(row, channel)]. Returns x [M][K], w [N][K][1][1], bias [N] (dyadic, fp32, on `dev`) and the exact fp64 x w^T + bias"""
    x = RC.dyadic((M, K), 31); w = RC.dyadic((N, K), 32); bias = RC.dyadic((N,), 33)
    for r, n in plants:
        x[r] = torch.sign(w[n])
        bias[n] = value / (1.0 if scales is None else scales(n)) - float(w[n].abs().sum())
    x, w, bias = x.to(dev), w.to(dev), bias.to(dev)
    ref = x.double() @ w.double().t() + bias.double()
    for r, n in plants:
        assert float(ref[r, n]) == float(ref[:, n].max())
    return x, w.view(N, K, 1, 1), bias, ref


def _no_npers(flag):
    class _Env:
        def __enter__(self):
            if flag:
                os.environ["STEDM_CONV_NO_NPERS"] = "1"

        def __exit__(self, *a):
            os.environ.pop("STEDM_CONV_NO_NPERS", None)
    return _Env()


@pytest.mark.parametrize("prec,value", VARIANTS)
@pytest.mark.parametrize("name,B,H,W,K,N", [("lean_tiled", 493, 10, 10, 128, 200), ("lean_npers", 1, 1, 49300, 128, 200)])
def test_conv_out16_flat(dev, name, B, H, W, K, N, prec, value):
    """the 16-bit-only output without statistics (shapes of rs1x1_two_n_tiles and rs1x1n_flat, test_gpu_conv_exact.py): the lean 8-channel
    loop of the tiled 1x1 and the accumulator store of the N-persistent form (the flat shape meets its admission rule; run a second time
    with STEDM_CONV_NO_NPERS, which sends it to the tiled kernel: either form is held to the same word and plane)"""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    M = B * H * W
    # the last valid row of the ragged last M tile (49300 = 192 * 256 + 148) in the last column of the masked last N tile; the first element
    for plant in [(M - 1, N - 1), (0, 0), (M // 2 + 7, N // 2 + 3)]:
        x, w, bias, ref = _flat_operands(dev, M, K, N, [plant], value)
        assert RG.plant_ok(ref) and float(ref[plant]) == value
        x16 = x.to(_dt(prec)).view(torch.int16).view(B, H, W, K)
        assert torch.equal(x16.view(_dt(prec)).float().view(M, K), x)
        whi, wlo = ops.pack_conv_weight(w, pr); wf = ops.pack_conv_weight_frag(w, pr)
        for no_npers in ([False, True] if name == "lean_npers" else [False]):
            o16 = torch.full((B, H, W, N), FILL16, dtype=torch.int16, device=dev)
            k = dict(prec=pr, ks=1, src16=(x16, None), w_frag=wf, bias=bias, out16=(o16, None))
            assert ops.conv_igemm(None, whi, wlo, None, query_rs=True, **k)
            with _Guard({RG.CONV_OUT16: ref}, prec, f"{name} {plant} no_npers={no_npers}") as g, _no_npers(no_npers):
                ops.conv_igemm(None, whi, wlo, None, **k)
            g.plane(o16.view(M, N), ref)


@pytest.mark.parametrize("prec,value", VARIANTS)
@pytest.mark.parametrize("name,nb,T,heads,dim", [("qkv_tiled", 11, 514, 4, 128), ("qkv_npers", 13, 4098, 2, 128)])
def test_conv_out16_qkv(dev, name, nb, T, heads, dim, prec, value):
    """the qkv epilogue (qkv_planes; shapes of test_to_qkv_epilogue_writes_the_attention_planes): a q, a k and a v element planted through
    the bias, one launch each. q is stored as (out + bias) * qscale with qscale = 1/2: exact in fp32, the planted q bias is 2 * target - max.
    The second shape has the M tiles of the N-persistent form and runs a second time with STEDM_CONV_NO_NPERS (the tiled epilogue)."""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    dt = _dt(prec)
    M, HD, Tp = nb * T, heads * 64, (T + 127) // 128 * 128
    N = 3 * HD
    qs = 0.5
    scales = lambda n: qs if n < HD else 1.0
    # q in the first row, k in a row of a tile that straddles two samples, v in the last valid row of the ragged last tile
    for sec, plant in [("q", (0, 3)), ("k", (T + 1, HD + HD - 1)), ("v", (M - 1, 2 * HD + HD - 2)), ("v", (M - 2, 2 * HD))]:
        x, w, bias, ref = _flat_operands(dev, M, dim, N, [plant], value, scales)
        assert RG.plant_ok(ref)      # before the scale; the product with 1/2 is exact in fp32
        ref = ref.clone()
        ref[:, :HD] *= qs
        assert float(ref[plant]) == value
        x16 = x.to(dt).view(torch.int16).view(1, 1, M, dim)
        whi, wlo = ops.pack_conv_weight(w, pr); wf = ops.pack_conv_weight_frag(w, pr)
        r5 = ref.view(nb, T, 3, heads, 64)
        want = [r5[:, :, s_].permute(0, 2, 1, 3).reshape(nb * heads, T, 64) for s_ in range(3)]
        for no_npers in ([False, True] if name == "qkv_npers" else [False]):
            q, k_ = (torch.full((nb * heads, Tp, 64), FILL16, dtype=torch.int16, device=dev) for _ in range(2))
            vt = torch.full((nb * heads, 64, Tp), FILL16, dtype=torch.int16, device=dev)
            kw = dict(prec=pr, ks=1, src16=(x16, None), w_frag=wf, bias=bias, qkv_planes=(q, k_, vt, T, Tp, heads, qs))
            assert ops.conv_igemm(None, whi, wlo, None, query_rs=True, **kw)
            with _Guard({RG.CONV_OUT16: ref}, prec, f"{name} {sec} {plant} no_npers={no_npers}") as g, _no_npers(no_npers):
                ops.conv_igemm(None, whi, wlo, None, **kw)
            g.plane(q[:, :T].contiguous(), want[0])
            g.plane(k_[:, :T].contiguous(), want[1])
            g.plane(vt[:, :, :T].contiguous(), want[2].transpose(1, 2))
            assert bool((q[:, T:] == FILL16).all()) and bool((k_[:, T:] == FILL16).all()) and bool((vt[:, :, T:] == FILL16).all())


# ================================================================================================ NORM from the convolution epilogues
@pytest.mark.parametrize("prec,beta_c", NORM_VARIANTS)
def test_norm_layernorm_epilogue(dev, prec, beta_c):
    """ln_after (shape of test_gemm_with_layernorm_epilogue: M = 33333, K = 64, N = 96, ragged last M tile): the 16-bit output of the
    LayerNorm epilogue carries bit NORM"""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    M, K, N = 33333, 64, 96
    x16 = (_randn((M, K), 41, 0.7)).to(dev).to(_dt(prec)).view(torch.int16)
    w = _randn((N, K, 1, 1), 42, 1.0 / math.sqrt(K)).to(dev)
    bs = _randn((N,), 43, 0.3).to(dev)
    whi, wlo = ops.pack_conv_weight(w, pr); wf = ops.pack_conv_weight_frag(w, pr)
    v4 = lambda t: t.view(1, 1, M, -1)
    for c in (0, N - 1):
        gamma = _randn((N,), 44, 0.2, 1.0); beta = _randn((N,), 45, 0.1)
        gamma[c] = 0.0; beta[c] = beta_c
        h16 = torch.full((M, N), FILL16, dtype=torch.int16, device=dev)
        y = torch.full((M, N), NAN, device=dev)
        kw = dict(prec=pr, ks=1, src16=(v4(x16), None), w_frag=wf, bias=bs, out16=(v4(h16), None), ln_after=(gamma.to(dev), beta.to(dev), 1e-5, None))
        assert ops.conv_igemm(None, whi, wlo, v4(y), query_rs=True, **kw)
        with _Guard({RG.NORM: torch.tensor([beta_c])}, prec, f"LayerNorm epilogue, channel {c}") as g:
            ops.conv_igemm(None, whi, wlo, v4(y), **kw)
        _check_norm_planes(g, h16, prec, [c], beta_c, f"LayerNorm epilogue, channel {c}")
        assert bool((y[:, c] == beta_c).all())


# (id, B, H, W, cin, cout): in_tile - the (126, 8, 8, 256, 128) shape of test_conv_with_the_consumers_groupnorm (four samples per tile, a
# last tile of two samples and two masked ones) at the smallest batch that keeps gn_tile: the dispatcher runs the register-streamed kernel
# without a K split from 3/4 of the chip's 256 CUs in tiles, 192 tiles = 766 samples of 64 pixels; coop - the ("f16", 64, 32, 32) case of
# test_conv_group_norm_epilogue_across_the_tiles_of_a_sample; splitk - the batch-1 CFG step's shape, the GroupNorm rides on the reduce pass
RIDING = [("in_tile", 766, 8, 8, 256, 128), ("coop", 64, 32, 32, 128, 128), ("splitk", 2, 8, 8, 1024, 1024)]


@pytest.mark.parametrize("prec,beta_c", NORM_VARIANTS)
@pytest.mark.parametrize("name,B,H,W,cin,cout", RIDING, ids=[r[0] for r in RIDING])
def test_norm_riding_groupnorm(dev, name, B, H, W, cin, cout, prec, beta_c):
    """gn_next: the consumer's GroupNorm written by the convolution's own launch, in its three forms. gamma = 0 / beta on one channel:
    bit NORM (whichever form runs: where the epilogue form is not taken, the dispatcher's stedm_gn_apply16c pass writes the planes)."""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    x = _randn((B, H, W, cin), 51).to(dev)
    w = _randn((cout, cin, 3, 3), 52, 1.0 / math.sqrt(cin * 9)).to(dev)
    bias = _randn((cout,), 53).to(dev); emb = _randn((B, cout), 54).to(dev)
    h16 = torch.empty((B, H, W, cin), dtype=torch.int16, device=dev)
    ops.gn_apply16(x, None, h16, None, pr)
    whi, wlo = ops.pack_conv_weight(w, pr); wf = ops.pack_conv_weight_frag(w, pr)
    wf16 = ops.pack_conv_weight_frag16(w, pr) if cin >= 256 else None
    kw = dict(prec=pr, src16=(h16, None), bias=bias, emb=emb, emb_offset=0, emb_bstride=cout, w_frag=wf, w_frag16=wf16)
    ns = ops.gn_chan_nslab(H * W)
    cw = ops.coop_words_new() if name == "coop" else None
    words = torch.zeros((B, 4, 128, 2), dtype=torch.int64, device=dev) if name == "coop" else None
    for c in (2, cout - 1):
        gamma = _randn((cout,), 55, 0.3, 1.0); beta = _randn((cout,), 56, 0.2)
        gamma[c] = 0.0; beta[c] = beta_c
        out = torch.full((B, H, W, cout), NAN, device=dev); cs = torch.full((B, ns, cout, 2), NAN, device=dev)
        planes = torch.full((B, H, W, cout), FILL16, dtype=torch.int16, device=dev)
        k = dict(kw, chan_stats=cs, gn_next=(gamma.to(dev), beta.to(dev), 1e-5, 32, 0, planes, None, name == "coop"))
        if name == "coop":
            ops.step_advance(cw, 1)
            k["coop"] = (words, cw)
        if name == "splitk":
            k["ws"] = torch.full((16 * out.numel(),), NAN, device=dev)
        with _Guard({RG.NORM: torch.tensor([beta_c])}, prec, f"riding GroupNorm {name}, channel {c}") as g:
            ops.conv_igemm(None, whi, wlo, out, **k)
        _check_norm_planes(g, planes, prec, [c], beta_c, f"riding GroupNorm {name}, channel {c}")
        assert bool(torch.isfinite(cs).all()), "statistics slots left unwritten"
        if name == "coop":
            assert bool(torch.isnan(out).all()), "the epilogue form did not run (it stores no fp32 tensor: gn_only)"
        if name == "splitk":
            assert not bool(torch.isnan(k["ws"]).all()), "the K split did not run: the workspace is untouched"
    if name == "coop":
        assert int(cw[1].item()) == 0
        ops.coop_check("test")


# ================================================================================================ composite: the real pipeline
@pytest.mark.parametrize("prec,value", VARIANTS)
def test_composite_conv_statistics_switch_the_raw_test_on(dev, prec, value):
    """A dyadic split-K convolution (splitk3x3_b2) with chan_stats whose fp32 output has one element at the value; stedm_gn_apply16c reads
    that output and THE EPILOGUE'S partials (no stedm_gn_chan_stats in between) and writes the raw planes: the RAW bit must come up from
    them. The convolution itself writes no 16-bit output: the word is RAW alone."""
    from stedm_amd import ops
    c = _base("splitk3x3_b2", 2, 8, 8, 1024, 1024, ws=True)
    o = CE._operands(dev, c, 1)
    pr = ops.Precision.parse(prec)
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    hi = torch.empty((B, H, W, cin), dtype=torch.int16, device=dev)
    ops.gn_apply16(o["a"], None, hi, None, pr)
    whi, wlo = ops.pack_conv_weight(o["w"], pr); wf = ops.pack_conv_weight_frag(o["w"], pr)
    gamma = _randn((cout,), 61, 0.1, 1.0).to(dev); beta = _randn((cout,), 62, 0.1).to(dev)
    for p in [(0, 0, 0, 0), (B - 1, H - 1, W - 1, cout - 1)]:
        res, ref = conv16_planted(c, o, [p], value)
        out = torch.full((B, H, W, cout), NAN, device=dev); cs = torch.full((B, ops.gn_chan_nslab(H * W), cout, 2), NAN, device=dev)
        nrm = torch.full((B, H, W, cout), FILL16, dtype=torch.int16, device=dev); raw = torch.full_like(nrm, FILL16)
        with _Guard({RG.RAW: ref}, prec, f"conv -> gn_apply16c(raw) {list(p)}") as g:
            ops.conv_igemm(None, whi, wlo, out, prec=pr, src16=(hi, None), bias=o["bias"], emb=o["emb"], emb_offset=EMB_OFF, emb_bstride=o["emb"].shape[1],
                           res=res, w_frag=wf, chan_stats=cs, ws=torch.full((16 * out.numel(),), NAN, device=dev))
            ops.gn_apply16c(out, cs, None, None, nrm, None, pr, gamma, beta, 1e-5, 32, 1, raw=(raw, None))
        assert torch.equal(out.double(), ref)
        g.plane(raw, ref)
        assert bool(torch.isfinite(nrm.view(_dt(prec)).float()).all())
        if prec == "f16":
            assert g.expected == (RG.RAW if value == RG.OVER else 0)
