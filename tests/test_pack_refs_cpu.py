"""CPU tier of the pack references (tests/refs_pack.py): every layout function is an index gather written from the header's formula; here each
is held against an independent statement of the same layout. A fragment order is undone with a reshape and a permute (no index tensors) and
must give back refs_conv.otc of the filter; the sub-pixel fold must equal refs_conv.subpixel_fold bit for bit; the space-to-depth filter
must reproduce, through the 2x2 convolution that reads it, the stride-2 3x3 convolution of refs_conv.conv_ref exactly (dyadic operands in
fp64, both paddings)."""
import pytest
import torch

from tests import refs_conv as RC
from tests import refs_pack as RP

torch.set_grad_enabled(False)


def _unfrag32(f, cout):
    """[tn][chunk][tap][q][lane = h * 32 + r][e] -> [n = tn * 128 + q * 32 + r][tap][c = chunk * 16 + h * 8 + e]"""
    tn, nch, taps = f.shape[:3]
    return f.reshape(tn, nch, taps, 4, 2, 32, 8).permute(0, 3, 5, 2, 1, 4, 6).reshape(tn * 128, taps, nch * 16)[:cout]


def _unfrag16(f, cout):
    """[tn][chunk][tap][c][lane = g * 16 + r][e] -> [n = tn * 128 + c * 16 + r][tap][ci]; a 1x1 has ci = chunk * 32 + g * 8 + e, a filter with
    taps splits g = g1 * 2 + g0 and has ci = chunk * 32 + g0 * 16 + g1 * 8 + e"""
    tn, nch, taps = f.shape[:3]
    if taps == 1:
        return f.reshape(tn, nch, taps, 8, 4, 16, 8).permute(0, 3, 5, 2, 1, 4, 6).reshape(tn * 128, taps, nch * 32)[:cout]
    return f.reshape(tn, nch, taps, 8, 2, 2, 16, 8).permute(0, 3, 6, 2, 1, 5, 4, 7).reshape(tn * 128, taps, nch * 32)[:cout]


@pytest.mark.parametrize("cout,cin,ks", [(160, 48, 3), (128, 16, 1), (96, 32, 3)])
def test_frag32_unpermutes_to_the_planes(cout, cin, ks):
    w = RC.normal((cout, cin, ks, ks), 11, "pk.w32")
    f = RP.frag32(RP.oihw(w))
    assert torch.equal(_unfrag32(f, cout), RC.otc(w))
    assert torch.equal(_unfrag32(f, 1 << 30)[cout:], torch.zeros(f.shape[0] * 128 - cout, ks * ks, cin))
    assert torch.equal(RP.planes(RP.oihw(w)), RC.otc(w))


@pytest.mark.parametrize("cout,cin,ks", [(160, 64, 3), (160, 32, 1), (96, 96, 3)])
def test_frag16_unpermutes_to_the_planes(cout, cin, ks):
    w = RC.normal((cout, cin, ks, ks), 12, "pk.w16")
    f = RP.frag16(RP.oihw(w))
    assert torch.equal(_unfrag16(f, cout), RC.otc(w))
    assert torch.equal(_unfrag16(f, 1 << 30)[cout:], torch.zeros(f.shape[0] * 128 - cout, ks * ks, cin))


def test_logical_restates_the_transposed_flipped_source():
    """the dgrad source: n = forward cin, c = forward cout, taps reversed, read straight from the OIHW parameter"""
    co, ci = 24, 40
    w = RC.normal((co, ci, 3, 3), 13, "pk.wt")
    L = RP.logical(w, 9, ci * 9, True, ci, co, 9)
    assert torch.equal(L, RP.oihw(w.flip(2, 3).transpose(0, 1).contiguous()))
    assert torch.equal(RP.logical(w, ci * 9, 9, False, co, ci, 9), RP.oihw(w))


def test_hi_lo_words_split_the_value():
    v = torch.cat([RC.normal((4096,), 14, "pk.v", std=1.0 / 64), RC.normal((4096,), 15, "pk.v1")])
    for prec in ("f16", "bf16"):
        hi, lo = RP.hi_lo(v, prec)
        h, l = hi.view(RP.DT[prec]).float(), lo.view(RP.DT[prec]).float()
        assert torch.equal(hi, RP.words(v, prec))
        assert torch.equal(l, (v - h).to(RP.DT[prec]).float())
    hi, lo = RP.hi_lo(v[:4096], "f16")
    assert bool(((lo.view(torch.float16).abs() < 2.0 ** -14) & (lo != 0)).any())      # at the 1 / sqrt(K) scale f16 lo words are subnormal


def test_subpixel_layouts_equal_the_fold():
    w = RC.normal((40, 32, 3, 3), 16, "pk.wu")
    fold = RC.subpixel_fold(w)                                  # [4][O][4 taps][I]
    assert torch.equal(RP.subpixel(w).permute(0, 1, 3, 2), fold)
    assert torch.equal(RP.up_planes(w), fold.reshape(4 * 40, 4, 32))
    f32, f16 = RP.up_frag(w, RP.frag32), RP.up_frag(w, RP.frag16)
    for par in range(4):
        assert torch.equal(_unfrag32(f32[par], 40), fold[par])
        assert torch.equal(_unfrag16(f16[par], 40), fold[par])


def test_space_to_depth_is_pixel_unshuffle():
    x = RC.normal((2, 4, 6, 8), 17, "pk.x")
    ref = torch.nn.functional.pixel_unshuffle(x.permute(0, 3, 1, 2), 2)             # NCHW, channel = c * 4 + py * 2 + px
    ref = ref.reshape(2, 8, 4, 2, 3).permute(0, 3, 4, 2, 1).reshape(2, 2, 3, 32)
    assert torch.equal(RP.space_to_depth(x), ref)


@pytest.mark.parametrize("pad_br", [False, True])
@pytest.mark.parametrize("cin", [8, 24])
def test_s2d_filter_reproduces_the_stride2_convolution(cin, pad_br):
    B, H, W, cout = 2, 6, 8, 12
    x = RC.dyadic((B, H, W, cin), 18).double()
    w = RC.dyadic((cout, cin, 3, 3), 19).double()
    got = RP.conv2x2_ref(RP.space_to_depth(x), RP.s2d(w, pad_br), pad_br)
    assert torch.equal(got, RC.conv_ref(x, RC.otc(w), "down", 3, pad_br=pad_br))
    L = RP.s2d(w, pad_br)               # 4 * cin channels: a 16- or 32-channel chunk straddles two parity blocks
    assert torch.equal(_unfrag32(RP.frag32(L), cout), RP.planes(L))
    assert torch.equal(_unfrag16(RP.frag16(L), cout), RP.planes(L))
