"""CPU tier: pins the references of tests/refs_conv.py themselves, where there is no GPU. conv_ref / conv_ref_subpixel equal F.conv2d in
fp64 for every geometry the GPU file uses; the dyadic exactness that tests/test_gpu_conv_exact.py's bit-for-bit tier rests on holds for
torch's own fp32 convolution and for split / permuted accumulations at the largest K any GPU case reaches; and the growth factor of a plain
fp32 accumulation (the yardstick of the operand-exact tier) is measured, printed and held against refs_conv.G_PLAIN."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import refs_conv as RC

torch.set_grad_enabled(False)

K_MAX = 9 * 2048 + 2048 + 4          # the largest sum of a GPU case: 3x3 at 2048 channels + a fused 2048-channel 1x1 + two biases, embedding, residual


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


otc = RC.otc


def torch_conv(a_nchw, w, mode, pad_br=False):
    ks = w.shape[-1]
    if mode == "s1":
        return F.conv2d(a_nchw, w, padding=ks // 2)
    if mode == "down":
        return F.conv2d(F.pad(a_nchw, (0, 1, 0, 1)), w, stride=2) if pad_br else F.conv2d(a_nchw, w, stride=2, padding=1)
    return F.conv2d(F.interpolate(a_nchw, scale_factor=2, mode="nearest"), w, padding=1)


def _close64(got, ref, tol=1e-13):
    assert got.shape == ref.shape and got.dtype == torch.float64
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= tol * scale, float((got - ref).abs().max()) / scale


@pytest.mark.parametrize("mode,ks,pad_br", [("s1", 3, False), ("s1", 1, False), ("down", 3, False), ("down", 3, True), ("up", 3, False)])
@pytest.mark.parametrize("B,H,W,cin,cout", [(3, 6, 10, 40, 96), (1, 2, 2, 8, 5), (2, 8, 4, 16, 7)])
def test_conv_ref_is_conv2d(mode, ks, pad_br, B, H, W, cin, cout):
    a = RC.normal((B, cin, H, W), 1, "a").double()
    w = RC.normal((cout, cin, ks, ks), 2, "w").double()
    got = RC.conv_ref(nhwc(a), otc(w), mode, ks, pad_br)
    _close64(got, nhwc(torch_conv(a, w, mode, pad_br)))
    assert tuple(got.shape[1:3]) == RC.out_hw(H, W, mode)


def test_conv_ref_batch_chunks(monkeypatch):
    a = RC.normal((5, 4, 6, 8), 3, "a").double()
    w = RC.normal((7, 9, 8), 4, "w").double()
    whole = RC.conv_ref(a, w, "s1", 3)
    monkeypatch.setattr(RC, "MAX_F64_BYTES", 2 * 6 * 8 * 8 * 8 + 1)          # two padded samples per chunk, a last chunk of one
    assert torch.equal(RC.conv_ref(a, w, "s1", 3), whole)


@pytest.mark.parametrize("B,H,W,cin,cout", [(3, 5, 7, 24, 96), (1, 1, 1, 8, 3), (2, 4, 4, 32, 32)])
def test_subpixel_fold_is_nearest_upsample_then_conv(B, H, W, cin, cout):
    a = RC.normal((B, cin, H, W), 5, "a").double()
    w = RC.normal((cout, cin, 3, 3), 6, "w").double()
    w_eff = RC.subpixel_fold(w)
    assert tuple(w_eff.shape) == (4, cout, 4, cin)
    ref = nhwc(torch_conv(a, w, "up"))
    _close64(RC.conv_ref_subpixel(nhwc(a), w_eff), ref)
    _close64(RC.conv_ref(nhwc(a), otc(w), "up", 3), ref)
    assert torch.equal(w_eff.sum((0, 2)), 4 * w.sum((2, 3)))          # every 3x3 tap lands in exactly one tap of every parity


def test_epilogue_and_slab_stats():
    ref = RC.normal((3, 4, 6, 10), 7, "r").double()
    bias, emb, res = RC.normal((10,), 8, "b").double(), RC.normal((3, 20), 9, "e").double(), RC.normal((3, 4, 6, 10), 10, "s").double()
    got = RC.epilogue(ref, bias, emb, 4, res)
    assert torch.equal(got, ref + bias[None, None, None, :] + emb[:, 4:14][:, None, None, :] + res)
    assert RC.epilogue(ref) is ref
    s, q = RC.slab_stats(got.float(), 8)
    flat = got.float().double().view(3, 3, 8, 10)
    _close64(s, flat.sum(2)); _close64(q, (flat * flat).sum(2))
    # sub-pixel slots: one per output parity (and 256-pixel run of the low-res grid)
    up = RC.normal((2, 8, 12, 5), 11, "u").double()
    s, q = RC.slab_stats(up, RC.slot_parity(4, 6))
    for py in range(2):
        for px in range(2):
            _close64(s[:, py * 2 + px], up[:, py::2, px::2].sum((1, 2))); _close64(q[:, py * 2 + px], (up[:, py::2, px::2] ** 2).sum((1, 2)))
    idx = RC.slot_parity(32, 16)               # 512 low-res pixels: two runs of 256 = 16 rows each
    assert int(idx.max()) == 7 and int(idx.view(64, 32)[31, 0]) == 2 and int(idx.view(64, 32)[32, 1]) == 4 + 1


def test_as_f64_and_three_products():
    x = RC.normal((1000,), 12, "x")
    for label, dt in (("f16", torch.float16), ("bf16", torch.bfloat16), ("f16x3", torch.float16), ("bf16x3", torch.bfloat16)):
        assert torch.equal(RC.as_f64(x.to(dt).view(torch.int16), label), x.to(dt).double())
    a = RC.normal((2, 4, 4, 8), 13, "a").double(); w = RC.normal((6, 9, 8), 14, "w").double()
    ah, wh = a.half().double(), w.half().double()
    al, wl = (a - ah).half().double(), (w - wh).half().double()
    conv = lambda p, q: RC.conv_ref(p, q, "s1", 3)
    got = RC.three_products(ah, al, wh, wl, conv)
    _close64(got, conv(ah + al, wh + wl) - conv(al, wl), 1e-12)
    S = RC.abs_sum(a, w, conv, bias=-torch.ones(6, dtype=torch.float64))
    assert torch.equal(S, conv(a.abs(), w.abs()) + 1.0) and bool((S >= conv(a, w).abs()).all())


def test_dyadic_ok_states_the_fp32_limit():
    RC.dyadic_ok(K_MAX)
    RC.dyadic_ok(4 * 2048, wmax=4.0)
    with pytest.raises(AssertionError):
        RC.dyadic_ok(1 << 18)


def test_dyadic_convolution_is_exact_in_fp32_at_the_largest_k():
    """3x3 at 2048 channels + a 2048-channel 1x1 + bias, embedding row, residual on dyadic data: torch's fp32 convolution, a 16-way channel
    split summed afterwards and a permuted channel order all equal the fp64 result bit for bit."""
    B, H, W, cin, cb, cout = 2, 4, 4, 2048, 2048, 24
    RC.dyadic_ok(9 * cin + cb + 4)
    a, x = RC.dyadic((B, H, W, cin), 1), RC.dyadic((B, H, W, cb), 2)
    w3, w1 = RC.dyadic((cout, 9, cin), 3), RC.dyadic((cout, 1, cb), 4)
    bias, emb, res = RC.dyadic((cout,), 5), RC.dyadic((B, cout + 24), 6), RC.dyadic((B, H, W, cout), 7)
    full = lambda a_, x_, w3_, w1_: RC.conv_ref(a_, w3_, "s1", 3) + RC.conv_ref(x_, w1_, "s1", 1)
    ref = RC.epilogue(full(a.double(), x.double(), w3.double(), w1.double()), bias.double(), emb.double(), 8, res.double())
    assert float(ref.abs().max()) > 64.0
    got = RC.epilogue(full(a, x, w3, w1), bias, emb, 8, res)
    assert got.dtype == torch.float32 and torch.equal(got.double(), ref)
    w_oihw = w3.view(cout, 3, 3, cin).permute(0, 3, 1, 2).contiguous()
    t = F.conv2d(a.permute(0, 3, 1, 2), w_oihw, padding=1) + F.conv2d(x.permute(0, 3, 1, 2), w1.view(cout, cb, 1, 1))
    assert torch.equal(RC.epilogue(nhwc(t), bias, emb, 8, res).double(), ref)
    parts = None                                                          # a K split: 16 channel shares, each rounded to fp32, added in order
    for s in range(16):
        sl = slice(s * cin // 16, (s + 1) * cin // 16); sb = slice(s * cb // 16, (s + 1) * cb // 16)
        p = full(a[..., sl], x[..., sb], w3[..., sl], w1[..., sb])
        parts = p if parts is None else parts + p
    assert torch.equal(RC.epilogue(parts, bias, emb, 8, res).double(), ref)
    perm = torch.randperm(cin, generator=torch.Generator().manual_seed(1))
    assert torch.equal(RC.epilogue(full(a[..., perm], x[..., perm], w3[..., perm], w1[..., perm]), bias, emb, 8, res).double(), ref)


def test_dyadic_subpixel_fold_is_exact_in_both_16_bit_types():
    """the pre-summed taps of dyadic weights reach |4| in steps of 1/8: exact in f16 and bf16, and the folded fp32 convolution equals
    nearest-2x + 3x3 in fp64 bit for bit"""
    B, H, W, cin, cout = 2, 4, 4, 1024, 24
    RC.dyadic_ok(4 * cin, wmax=4.0)
    a = RC.dyadic((B, H, W, cin), 8)
    w = RC.dyadic((cout, cin, 3, 3), 9)
    w_eff = RC.subpixel_fold(w)
    assert float(w_eff.abs().max()) == 4.0
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(w_eff.to(dt).float(), w_eff) and torch.equal(a.to(dt).float(), a)
    ref = RC.conv_ref(a.double(), otc(w).double(), "up", 3)
    got = RC.conv_ref_subpixel(a, w_eff)
    assert got.dtype == torch.float32 and torch.equal(got.double(), ref)


@pytest.mark.parametrize("mode,pad_br", [("down", False), ("down", True)])
def test_dyadic_downsample_is_exact(mode, pad_br):
    a = RC.dyadic((2, 8, 8, 64), 10); w = RC.dyadic((24, 9, 64), 11)
    assert torch.equal(RC.conv_ref(a, w, mode, 3, pad_br).double(), RC.conv_ref(a.double(), w.double(), mode, 3, pad_br))


def test_growth_factor_of_a_plain_fp32_accumulation(capsys):
    """max |fp32 conv of the 16-bit-rounded operands - fp64 conv of the same operands| / (u * S) with S the convolution of the magnitudes,
    for torch's CPU convolution at K = 2304 and K = 18432 in both 16-bit types, on the GPU tier's operand distributions (silu(1.3 x + 0.1)
    activations, 1 / sqrt(K) weights). A maximum over a few thousand outputs scatters with the sample (0.37 .. 0.68 over the four cases here,
    the larger values at the shorter K), so refs_conv.G_PLAIN = 0.5 is held to within a factor of two of the largest of the four, both ways:
    the GPU tier's bound G = 16 * G_PLAIN comes from this property of fp32, not from a kernel."""
    worst = 0.0
    for cin in (256, 2048):
        a = F.silu(RC.normal((2, cin, 8, 8), 20 + cin, "a") * 1.3 + 0.1)
        w = RC.normal((32, cin, 3, 3), 21 + cin, "w", std=1.0 / math.sqrt(9 * cin))
        for dt in (torch.float16, torch.bfloat16):
            ar, wr = a.to(dt).float(), w.to(dt).float()
            got = F.conv2d(ar, wr, padding=1).double()
            ref = F.conv2d(ar.double(), wr.double(), padding=1)
            S = F.conv2d(ar.double().abs(), wr.double().abs(), padding=1)
            g = float(((got - ref).abs() / (RC.U * S)).max())
            with capsys.disabled():
                print(f"\n  growth factor, K = {9 * cin}, {dt}: {g:.3f}", end="")
            worst = max(worst, g)
    with capsys.disabled():
        print(f"\n  largest: {worst:.3f} (G_PLAIN = {RC.G_PLAIN}, G = {RC.G})")
    assert RC.G_PLAIN / 2 <= worst <= 2 * RC.G_PLAIN
    assert RC.G == 16 * RC.G_PLAIN
