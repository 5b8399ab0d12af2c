"""GPU tier (-m gpu): every weight-pack entry (stedm_pack_*) and stedm_space_to_depth16, in f16 and bf16, word for word against the plain
references of tests/refs_pack.py. A pack is index arithmetic and one rounding, so the comparison is torch.equal on the int16 words: a wrong
kofs, tap map, fold order or lo rounding fails at its cause, not in a convolution far from it. Every output is filled with a word no pack of
these inputs produces (0x7fff, a NaN) where the caller hands the buffer over; the others are allocated by the wrapper and compared whole.

Shapes are the smallest that reach each branch: a ragged second 128-row tile, cin a multiple of 16 but not of 32, both kofs rules, the
16-byte and the scalar gather on full tiles, a transposed + flipped source, s2d channel counts at which a 16- or 32-channel chunk straddles
two parity blocks. Values are at the scale 1 / sqrt(cin * taps) of an initialised filter, where most f16 lo words are subnormal, plus one case
at unit scale."""
import math

import pytest
import torch

from tests import refs_conv as RC
from tests import refs_pack as RP

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

PRECS = ["f16", "bf16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from stedm_amd import ops as o
    return o


def _w(shape, seed, unit=False):
    taps_cin = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1)
    return RC.normal(shape, seed, "pack.w", std=1.0 if unit else 1.0 / math.sqrt(taps_cin))


def _prec(ops, prec, lo):
    return ops.Precision.parse({("f16", False): "f16", ("bf16", False): "bf16", ("f16", True): "parity", ("bf16", True): "parity_bf16"}[(prec, lo)])


def _eq(got, want):
    assert got.dtype == torch.int16 and tuple(got.shape) == tuple(want.shape), (got.dtype, tuple(got.shape), tuple(want.shape))
    assert torch.equal(got.cpu(), want)


def _eq_hl(got, v, prec):
    """got: [2] + layout, the hi stream then the lo stream"""
    hi, lo = RP.hi_lo(v, prec)
    _eq(got, torch.stack([hi, lo]))


# ------------------------------------------------------------------------------------------------ planes
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("ks", [3, 1])
def test_planes(dev, ops, prec, lo, ks):
    cout, cin = 40, 24
    w = _w((cout, cin, ks, ks), 21)
    hi, l = ops.pack_conv_weight(w.to(dev), _prec(ops, prec, lo))
    whi, wlo = RP.hi_lo(RP.planes(RP.oihw(w)), prec)
    _eq(hi, whi)
    assert (l is None) == (not lo)
    if lo:
        _eq(l, wlo)


def test_planes_conv1d_weight(dev, ops):
    w = _w((40, 24, 1), 22)
    hi, _ = ops.pack_conv_weight(w.to(dev), _prec(ops, "f16", False))
    _eq(hi, RP.words(RP.planes(RP.oihw(w)), "f16"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("lo", [False, True])
def test_planes_up(dev, ops, prec, lo):
    w = _w((40, 24, 3, 3), 23)
    hi, l = ops.pack_conv_weight_up(w.to(dev), _prec(ops, prec, lo))
    whi, wlo = RP.hi_lo(RP.up_planes(w), prec)
    _eq(hi, whi)
    assert (l is None) == (not lo)
    if lo:
        _eq(l, wlo)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("lo", [False, True])
@pytest.mark.parametrize("ks", [3, 1])
def test_planes_strided_transposed_flipped(dev, ops, prec, lo, ks):
    co, ci, taps = 40, 24, ks * ks                  # forward shape; the pack's rows are the forward input channels
    w = _w((co, ci, ks, ks), 24)
    hi, l, frag = ops.pack_conv_weight_strided(w.to(dev), taps, ci * taps, True, ci, co, ks, _prec(ops, prec, lo), want_hi=True)
    L = RP.oihw(w.flip(2, 3).transpose(0, 1).contiguous())
    whi, wlo = RP.hi_lo(RP.planes(L), prec)
    _eq(hi, whi)
    assert frag is None and (l is None) == (not lo)
    if lo:
        _eq(l, wlo)


# ------------------------------------------------------------------------------------------------ 32x32x16 order
def test_pack_conv_weight_frag_layout(dev):
    from stedm_amd import ops
    from stedm_amd.utils import prng
    prec = ops.Precision.parse("f16")
    cout, cin = 160, 48
    w = prng.normal(3, "wf.w", (cout, cin, 3, 3))
    got = ops.pack_conv_weight_frag(w.to(dev), prec).cpu().view(torch.float16).float()      # [tn][chunk][tap][q][lane][8]
    tn, ch, tap, q, lane, e = torch.meshgrid(*[torch.arange(n) for n in got.shape], indexing="ij")
    n = tn * 128 + (q // 2) * 64 + (q % 2) * 32 + (lane % 32)
    ci = ch * 16 + (lane // 32) * 8 + e
    wp = torch.cat([w, torch.zeros(256 - cout, cin, 3, 3)]).reshape(256, cin, 9)
    want = wp[n, ci, tap].half().float()
    assert torch.equal(got, want)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout,cin,ks,unit", [(160, 48, 3, False), (128, 16, 1, False), (160, 48, 3, True)])
def test_frag32(dev, ops, prec, cout, cin, ks, unit):
    w = _w((cout, cin, ks, ks), 25, unit)
    want = RP.words(RP.frag32(RP.oihw(w)), prec)
    _eq(ops.pack_conv_weight_frag(w.to(dev), _prec(ops, prec, False)), want)
    taps = ks * ks
    frag = ops.pack_conv_weight_strided(w.to(dev), cin * taps, taps, False, cout, cin, ks, _prec(ops, prec, False), want_hi=False, want_frag=True)[2]
    _eq(frag, want)


@pytest.mark.parametrize("prec", PRECS)
def test_frag32_dgrad_source(dev, ops, prec):
    """transposed, flipped, sn = taps, sc = cin * taps at forward shape (96, 160, 3): the n-fast 16-byte gather on a full tile and the
    scalar gather on the ragged one"""
    co, ci = 96, 160
    w = _w((co, ci, 3, 3), 26)
    hi, lo, frag = ops.pack_conv_weight_strided(w.to(dev), 9, ci * 9, True, ci, co, 3, _prec(ops, prec, False), want_hi=False, want_frag=True)
    assert hi is None and lo is None
    _eq(frag, RP.words(RP.frag32(RP.oihw(w.flip(2, 3).transpose(0, 1).contiguous())), prec))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ks", [3, 1])
def test_frag32_source_offset_by_one_float(dev, ops, prec, ks):
    """a source that is not 16-byte aligned: the 16-byte gather is refused and the scalar gather runs on full tiles"""
    cout, cin = 128, 32
    w = _w((cout, cin, ks, ks), 27)
    buf = torch.zeros(w.numel() + 1, device=dev)
    buf[1:] = w.flatten().to(dev)
    wd = buf[1:].view(w.shape)
    assert wd.data_ptr() % 16 == 4 and wd.is_contiguous()
    _eq(ops.pack_conv_weight_frag(wd, _prec(ops, prec, False)), RP.words(RP.frag32(RP.oihw(w)), prec))


# ------------------------------------------------------------------------------------------------ 16x16x32 order
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout,cin,ks", [(160, 64, 3), (160, 32, 1)])
def test_frag16(dev, ops, prec, cout, cin, ks):
    """the two kofs rules; the hi + lo entries (_hl for a 3x3, _hl1 for a 1x1); the hi stream of those equals the plain entry"""
    w = _w((cout, cin, ks, ks), 28)
    v = RP.frag16(RP.oihw(w))
    one = ops.pack_conv_weight_frag16(w.to(dev), _prec(ops, prec, False))
    _eq(one, RP.words(v, prec))
    two = ops.pack_conv_weight_frag16(w.to(dev), _prec(ops, prec, True))
    _eq_hl(two, v, prec)
    assert torch.equal(two[0], one)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("co,ci,ks", [(64, 160, 3), (32, 160, 1)])
def test_frag16_transposed_flipped(dev, ops, prec, co, ci, ks):
    taps = ks * ks
    w = _w((co, ci, ks, ks), 29)
    v = RP.frag16(RP.oihw(w.flip(2, 3).transpose(0, 1).contiguous()))
    kw = dict(sn=taps, sc=ci * taps, flip=True, cout=ci, cin=co, ks=ks)
    _eq(ops.pack_conv_weight_frag16(w.to(dev), _prec(ops, prec, False), **kw), RP.words(v, prec))
    _eq_hl(ops.pack_conv_weight_frag16(w.to(dev), _prec(ops, prec, True), **kw), v, prec)


def test_frag16_unit_scale(dev, ops):
    w = _w((160, 64, 3, 3), 30, unit=True)
    _eq_hl(ops.pack_conv_weight_frag16(w.to(dev), _prec(ops, "f16", True)), RP.frag16(RP.oihw(w)), "f16")


# ------------------------------------------------------------------------------------------------ derived filters
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout,cin", [(160, 32), (96, 64)])
def test_up_frag(dev, ops, prec, cout, cin):
    w = _w((cout, cin, 3, 3), 31)
    _eq(ops.pack_conv_weight_up_frag(w.to(dev), _prec(ops, prec, False)), RP.words(RP.up_frag(w, RP.frag32), prec))
    _eq_hl(ops.pack_conv_weight_up_frag16_hl(w.to(dev), _prec(ops, prec, True)), RP.up_frag(w, RP.frag16), prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pad_br", [False, True])
@pytest.mark.parametrize("cin", [8, 24])
def test_s2d_frag(dev, ops, prec, cin, pad_br):
    cout = 160
    w = _w((cout, cin, 3, 3), 32)
    L = RP.s2d(w, pad_br)
    _eq(ops.pack_conv_weight_s2d_frag(w.to(dev), _prec(ops, prec, False), pad_br=pad_br), RP.words(RP.frag32(L), prec))
    _eq_hl(ops.pack_conv_weight_s2d_frag16_hl(w.to(dev), _prec(ops, prec, True), pad_br=pad_br), RP.frag16(L), prec)


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("lo", [False, True])
def test_space_to_depth16(dev, ops, prec, lo):
    B, H, W, C = 2, 4, 6, 8
    x = RC.normal((B, H, W, C), 33, "pack.x", std=1.0 / 64)
    hi = torch.full((B, H // 2, W // 2, 4 * C), 0x7FFF, dtype=torch.int16, device=dev)
    l = torch.full_like(hi, 0x7FFF) if lo else None
    ops.space_to_depth16(x.to(dev), hi, l, _prec(ops, prec, lo))
    whi, wlo = RP.hi_lo(RP.space_to_depth(x), prec)
    _eq(hi, whi)
    if lo:
        _eq(l, wlo)


# ------------------------------------------------------------------------------------------------ many tensors, one launch
@pytest.mark.parametrize("prec", PRECS)
def test_pack_frag_multi_table_of_the_four_forms(dev, ops, prec):
    """one stedm_pack_frag_multi table holding the four forms above (both orders, plain and transposed + flipped, 3x3 and 1x1) writes what
    the single packs wrote, also after the weights changed"""
    pr = _prec(ops, prec, False)
    plan = ops.PackPlan(pr)
    ws = [_w(s, 34 + i).to(dev) for i, s in enumerate([(160, 64, 3, 3), (128, 32, 1, 1), (96, 160, 3, 3)])]
    outs, want = [], []

    def refs():
        r = []
        for w in ws:
            wc = w.cpu()
            L, Lt = RP.oihw(wc), RP.oihw(wc.flip(2, 3).transpose(0, 1).contiguous())
            r += [RP.words(RP.frag32(L), prec), RP.words(RP.frag16(L), prec), RP.words(RP.frag32(Lt), prec), RP.words(RP.frag16(Lt), prec)]
        return r

    for w in ws:
        co, ci, ks, _ = w.shape
        taps = ks * ks
        outs += [plan.frag_oihw(w, False), plan.frag_oihw(w, True), plan.frag(w, taps, ci * taps, True, ci, co, ks, False),
                 plan.frag(w, taps, ci * taps, True, ci, co, ks, True)]
    for a, b in zip(outs, refs()):
        _eq(a, b)
    for i, w in enumerate(ws):                      # an "optimizer step": same storage, new values
        w.copy_(_w(tuple(w.shape), 40 + i))
    for o in outs:
        o.fill_(0x7FFF)
    plan.run()
    for a, b in zip(outs, refs()):
        _eq(a, b)
