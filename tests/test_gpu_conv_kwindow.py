"""GPU tier (-m gpu): the K window (stedm_conv_args.src16_cstride / k_chan0 / w_cin) and res_bmod of the register-streamed 3x3 kinds,
in the form the U-Net uses them under classifier-free guidance (UNetModel._in_conv): a convolution over C channels at batch 2 Bs whose
channels [seam, C) carry the same values in samples b and b + Bs runs as

  shared launch  batch Bs, channels [seam, C) of the plane, the matching chunks of the FULL filter's fragment pack, no epilogue extra
                 -> fp32 partial P [Bs][H][W][cout]
  2B launch      batch 2 Bs, channels [0, seam), bias / embedding / statistics / the riding GroupNorm, res = P, res_bmod = Bs

and the pair is held against ONE fp64 convolution over the full K at batch 2 Bs, in the two tiers of tests/test_gpu_conv_exact.py (whose
references, generators and constants are those of tests/refs_conv.py):

  tier 1, bit-exact: dyadic operands, refs_conv.dyadic_ok on the FULL K (+ bias, embedding row and the partial): every fp32 partial sum is
    exact in every order, so the pair must equal the fp64 convolution: torch.equal. A second pair gives equal bits. A window that starts
    at the wrong chunk, a wrong row stride, a partial read from the wrong sample: each changes a term and fails.
  tier 2, operand-exact: normal data, operands read back from the planes, |out - ref64| <= G u S with the file's own G = 8. S is the same
    convolution and epilogue on the magnitudes over the full K: the pair adds no term a single launch would not have (P is one more fp32
    rounding of a partial sum, inside the margin G holds for the split-K partials).
  statistics against refs_conv.slab_stats of the stored output; the riding GroupNorm's planes against GroupNorm + SiLU of the stored output
    in fp64 (bound in _check_gn).

Output, partial, statistics, GroupNorm planes and workspaces are NaN- (or sentinel-) filled before every call. Which kernel runs is pinned
by what the case packs ('f': w_frag only, the 32x32x16 kind; 'm': w_frag16 only, the 16x16x32 kind, which the dispatcher takes from a
WINDOW width of 256 channels) and by query_rs; a launch whose grid is under 3/4 of the chip must have written its NaN-filled workspace.

Cases (Bs = res_bmod):
  a  98 x 16x16, C 576 = [0, 320) + [320, 576) (10 + 8 chunks of 32), 'm', cout 160: two N tiles, masked N; the shared launch has 98 tiles
     and takes the K split; the 2B launch is unsplit, with embedding, statistics and the riding GroupNorm
  b  772 x 8x8, C 512 = [0, 288) + [288, 512), 'f', cout 96: 16-channel chunks, four samples per tile, a ragged last tile (386 = 96 x 4 + 2)
  c  2 x 8x8, C 2048 = [0, 1024) + [1024, 2048), 'm', cout 1024: both launches split; res_bmod and the GroupNorm in the reduce pass
  d  8 x 32x32, C 256 = [0, 128) + [128, 256), 'f', cout 128: the 32 x 32 level, run with the gn_coop words
and, on case b, the 16-bit-only form of the 2B launch into a wider plane (out == NULL, out16_hi + out16_stride).

Measured on an MI355X, max over the output of |out - ref64| / (u S), f16 / bf16 (G = 8):  a 1.49 / 1.58   b 2.03 / 1.43   c 0.26 / 0.25
d 0.57 / 0.52  (the K-split forms stay under 1, as in tests/test_gpu_conv_exact.py; the file prints the figures with pytest -s)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import refs_conv as RC

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
U = RC.U
G = RC.G
EMB_OFF, EMB_PAD = 8, 24
GROUPS = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def case(name, B, bmod, H, W, C, seam, pack, cout, coop=False):
    return pytest.param(dict(name=name, B=B, bmod=bmod, H=H, W=W, C=C, seam=seam, pack=pack, cout=cout, coop=coop), id=name)


CASES = [
    case("a", 98, 49, 16, 16, 576, 320, "m", 160),
    case("b", 772, 386, 8, 8, 512, 288, "f", 96),
    case("c", 2, 1, 8, 8, 2048, 1024, "m", 1024),
    case("d", 8, 4, 32, 32, 256, 128, "f", 128, coop=True),
]
CASE_B = CASES[1].values[0]

_OPERANDS = {}          # one entry: the operands (and the tier-1 reference) of the case at hand, shared by its f16 / bf16 runs


def _operands(dev, c, tier):
    """fp32 operands on the device: a NHWC [B][H][W][C] whose channels [seam, C) repeat with period bmod over the batch, w OIHW, bias,
    emb [B][cout + EMB_PAD], GroupNorm gamma / beta"""
    key = (c["name"], tier)
    if key in _OPERANDS:
        return _OPERANDS[key]
    _OPERANDS.clear()
    B, Bs, H, W, C, cout, seam = c["B"], c["bmod"], c["H"], c["W"], c["C"], c["cout"], c["seam"]
    seed = 7000 + sum(ord(ch) for ch in c["name"])
    if tier == 1:
        gen = lambda shape, i, std=1.0: RC.dyadic(shape, 100 * seed + i)
        act = lambda t: t
    else:
        gen = lambda shape, i, std=1.0: RC.normal(shape, 100 * seed + i, "kw", std=std)
        act = lambda t: F.silu(t * 1.3 + 0.1)
    a = act(gen((B, H, W, C), 0))
    for r in range(1, B // Bs):
        a[r * Bs:(r + 1) * Bs, :, :, seam:] = a[:Bs, :, :, seam:]
    o = dict(a=a, w=gen((cout, C, 3, 3), 1, 1.0 / math.sqrt(C * 9)), bias=gen((cout,), 2, 0.05), emb=gen((B, cout + EMB_PAD), 3),
             gamma=RC.normal((cout,), seed + 11, "kw.g", std=0.2, mean=1.0), beta=RC.normal((cout,), seed + 12, "kw.b", std=0.2))
    o = {k: v.to(dev) for k, v in o.items()}
    _OPERANDS[key] = o
    return o


def _split_expected(ops, B, H, W, cout):
    """conv_rs_pick: a grid of fewer 256-row x 128-channel tiles than 3/4 of the chip runs only with a K split"""
    tiles = ((B * H * W + 255) // 256 if H * W >= 256 else (B + 256 // (H * W) - 1) // (256 // (H * W))) * ((cout + 127) // 128)
    return tiles * 4 < ops.device_cus() * 3


def _launch_pair(dev, c, prec_name, o, only16=False, nruns=2):
    """planes, packs and `nruns` identical (shared launch, 2B launch) pairs into NaN-filled buffers.
    only16: the 2B launch writes 16-bit values only, into channels [0, cout) of a plane of cout + 32 channels (no GroupNorm: it has no fp32 tensor)."""
    from stedm_amd import ops
    pr = ops.Precision.parse(prec_name)
    B, Bs, H, W, C, cout, seam, pack = c["B"], c["bmod"], c["H"], c["W"], c["C"], c["cout"], c["seam"], c["pack"]
    hi = torch.empty((B, H, W, C), dtype=torch.int16, device=dev)
    ops.gn_apply16(o["a"], None, hi, None, pr)
    whi, _ = ops.pack_conv_weight(o["w"], pr)
    pl = dict(ah=RC.as_f64(hi, pr.label), wh=RC.as_f64(whi, pr.label))
    wf = ops.pack_conv_weight_frag(o["w"], pr) if "f" in pack else None
    wf16 = ops.pack_conv_weight_frag16(o["w"], pr) if "m" in pack else None
    nslab = ops.gn_chan_nslab(H * W)
    runs = []
    for _ in range(nruns):
        P = torch.full((Bs, H, W, cout), NAN, device=dev)
        ws1 = torch.full((16 * Bs * H * W * cout,), NAN, device=dev)
        ws2 = torch.full((16 * B * H * W * cout,), NAN, device=dev)
        out = None if only16 else torch.full((B, H, W, cout), NAN, device=dev)
        cs = torch.full((B, nslab, cout, 2), NAN, device=dev)
        g16 = None if only16 else torch.full((B, H, W, cout), 0x7e7e, dtype=torch.int16, device=dev)
        k1 = dict(prec=pr, src16=(hi[:Bs, :, :, seam:], None), w_frag=wf, w_frag16=wf16, ws=ws1)
        k2 = dict(prec=pr, src16=(hi[:, :, :, :seam], None), w_frag=wf, w_frag16=wf16, ws=ws2, bias=o["bias"], emb=o["emb"], emb_offset=EMB_OFF,
                  emb_bstride=o["emb"].shape[1], res=P, res_bmod=Bs, chan_stats=cs)
        o16 = None
        if only16:
            o16 = torch.full((B, H, W, cout + 32), 0x7e7e, dtype=torch.int16, device=dev)
            k2.update(out16=(o16, None), out16_stride=cout + 32, cout=cout)
        else:
            k2.update(gn_next=(o["gamma"], o["beta"], 1e-5, GROUPS, 1, g16))
            if c["coop"]:
                words = ops.coop_words_new()
                ops.step_advance(words, 1)        # the epoch of this "forward" (never 0)
                k2.update(coop=(torch.zeros((B, 4, 128, 2), dtype=torch.int64, device=dev), words))
        assert ops.conv_igemm(None, whi, None, P, query_rs=True, **k1), "the register-streamed kernel was expected to run the shared launch"
        assert ops.conv_igemm(None, whi, None, out, query_rs=True, **k2), "the register-streamed kernel was expected to run the 2B launch"
        ops.conv_igemm(None, whi, None, P, **k1)
        ops.conv_igemm(None, whi, None, out, **k2)
        for ws_, b_, what in ((ws1, Bs, "shared"), (ws2, B, "2B")):
            if _split_expected(ops, b_, H, W, cout):
                assert not bool(torch.isnan(ws_).all()), f"the K split of the {what} launch did not run: its workspace is untouched"
        assert bool(torch.isfinite(P).all()), "elements of the partial left unwritten"
        runs.append((out, cs, g16, o16, P))
    torch.cuda.synchronize()
    if c["coop"] and not only16:
        ops.coop_check("test_gpu_conv_kwindow")
    return pr, pl, runs


def _reference(o, a, w):
    return RC.epilogue(RC.conv_ref(a, w, "s1", 3), o["bias"].double(), o["emb"].double(), EMB_OFF)


def _check_stats(cs, out):
    """both planes of every slot against the sums of the stored output (the bounds of tests/test_gpu_conv_exact.py)"""
    B, Ho, Wo, cout = out.shape
    nslab = cs.shape[1]
    idx = RC.slot_runs(Ho * Wo, 256 if nslab == (Ho * Wo + 255) // 256 else Ho * Wo // nslab, out.device)
    s, q = RC.slab_stats(out, idx)
    sa, _ = RC.slab_stats(out.abs(), idx)
    n = torch.bincount(idx, minlength=nslab).double()[None, :, None]
    assert s.shape[1] == nslab and bool(torch.isfinite(cs).all()), "statistics slots left unwritten"
    e0 = (cs[..., 0].double() - s).abs(); e1 = (cs[..., 1].double() - q).abs()
    assert bool((e0 <= n * U * sa).all()), f"sum: worst error / bound {float((e0 / (n * U * sa).clamp_min(1e-300)).max()):.3g}"
    assert bool((e1 <= (n + 1) * U * q).all()), f"sum of squares: worst error / bound {float((e1 / ((n + 1) * U * q).clamp_min(1e-300)).max()):.3g}"


def _check_gn(o, out, g16, label):
    """the riding GroupNorm + SiLU of the stored output, in fp64. The kernel computes y = (v - mean) * (rstd * gamma) + beta in fp32 from
    mean / rstd folded in double out of fp32 channel sums (each within n u sum|v| of its exact value, n <= 1024 pixels: a relative 6e-5 of
    the sample's scale at worst), then SiLU (slope <= 1.1) and ONE rounding to the 16-bit type (relative u16 = 2^-11 / 2^-8). Bound:
    |got - ref| <= u16 |ref| + 1e-4 (1 + |y|)."""
    B, H, W, C = out.shape
    v = out.double().view(B, H * W, GROUPS, C // GROUPS)
    mean = v.mean(dim=(1, 3), keepdim=True)
    var = (v * v).mean(dim=(1, 3), keepdim=True) - mean * mean
    y = ((v - mean) / torch.sqrt(var.clamp_min(0) + 1e-5)).view(B, H, W, C) * o["gamma"].double() + o["beta"].double()
    ref = y * torch.sigmoid(y)
    f16 = label.startswith("f16")
    got = g16.view(torch.float16 if f16 else torch.bfloat16).double()
    assert bool(torch.isfinite(got).all()), "GroupNorm plane elements left unwritten"
    u16 = 2.0 ** -11 if f16 else 2.0 ** -8
    err = (got - ref).abs()
    bound = u16 * ref.abs() + 1e-4 * (1 + y.abs())
    assert bool((err <= bound).all()), f"riding GroupNorm: worst error / bound {float((err / bound).max()):.3g}"


def _where(bad):
    i = bad.nonzero()
    return f"{int(bad.sum())} of {bad.numel()} elements differ, first at [b, y, x, n] = {i[0].tolist()}, last at {i[-1].tolist()}"


# ================================================================================================ tier 1: bit-exact
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("c", CASES)
def test_kwindow_pair_bit_exact_on_dyadic_operands(dev, c, prec):
    o = _operands(dev, c, 1)
    RC.dyadic_ok(9 * c["C"] + 4)
    if "ref" not in o:
        o["ref"] = _reference(o, o["a"].double(), RC.otc(o["w"]).double())
        assert bool((o["ref"] * 64 == (o["ref"] * 64).round()).all()) and float(o["ref"].abs().max()) * 64 < 2 ** 24
    ref = o["ref"]
    pr, pl, runs = _launch_pair(dev, c, prec, o)
    out, cs, g16, _, P = runs[0]
    bad = out.double() != ref
    assert not bool(bad.any()), _where(bad)
    assert torch.equal(out.double(), ref)
    # the partial alone: the fp64 convolution of the shared channels at batch bmod
    refP = RC.conv_ref(o["a"][:c["bmod"], :, :, c["seam"]:].double(), RC.otc(o["w"][:, c["seam"]:]).double(), "s1", 3)
    assert torch.equal(P.double(), refP), "the shared launch's partial is not the convolution of channels [seam, C)"
    o2, cs2, g2, _, P2 = runs[1]
    assert torch.equal(o2, out) and torch.equal(cs2, cs) and torch.equal(g2, g16) and torch.equal(P2, P), "the second run differs from the first"
    _check_stats(cs, out)
    _check_gn(o, out, g16, pr.label)


# ================================================================================================ tier 2: operand-exact
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("c", CASES)
def test_kwindow_pair_operand_exact(dev, c, prec):
    o = _operands(dev, c, 2)
    pr, pl, runs = _launch_pair(dev, c, prec, o)
    out, cs, g16, _, P = runs[0]
    ref = _reference(o, pl["ah"], pl["wh"])
    conv = lambda a_, w_: RC.conv_ref(a_, w_, "s1", 3)
    S = RC.abs_sum(pl["ah"], pl["wh"], conv, o["bias"].double().abs(), o["emb"].double().abs(), EMB_OFF)
    assert bool(torch.isfinite(out).all()), "output elements left unwritten"
    g = (out.double() - ref).abs() / (U * S)
    print(f"\n  MEASURED kwindow {c['name']:4s} {prec:6s} max err / (u S) = {float(g.max()):.3f}   (err / std(ref) = {float((out.double() - ref).abs().max() / ref.std()):.2e})", end="")
    bad = g > G
    assert not bool(bad.any()), f"max err / (u S) = {float(g.max()):.3f} > G = {G}: " + _where(bad)
    o2, cs2, g2, _, P2 = runs[1]
    assert torch.equal(o2, out) and torch.equal(cs2, cs) and torch.equal(g2, g16) and torch.equal(P2, P), "the second run differs from the first"
    _check_stats(cs, out)
    _check_gn(o, out, g16, pr.label)


# ================================================================================================ 16-bit-only output into a wider plane
@pytest.mark.parametrize("prec", ["f16", "bf16"])
def test_kwindow_pair_16bit_only_strided_output(dev, prec):
    c = CASE_B
    o = _operands(dev, c, 1)
    RC.dyadic_ok(9 * c["C"] + 4)
    if "ref" not in o:
        o["ref"] = _reference(o, o["a"].double(), RC.otc(o["w"]).double())
    ref = o["ref"]
    pr, pl, runs = _launch_pair(dev, c, prec, o, only16=True)
    _, cs, _, o16, _ = runs[0]
    dt = torch.float16 if pr.label.startswith("f16") else torch.bfloat16
    cout = c["cout"]
    assert torch.equal(o16[..., :cout].contiguous().view(dt), ref.float().to(dt)), "the 16-bit output is not torch's conversion of the exact value"
    assert bool((o16[..., cout:] == 0x7e7e).all()), "channels beyond cout of the wider plane were written"
    assert torch.equal(runs[1][3], o16) and torch.equal(runs[1][1], cs), "the second run differs from the first"
    _check_stats(cs, ref.float())        # the statistics are those of the fp32 values before their rounding (exact here)


# ================================================================================================ everything else refuses
def test_kwindow_and_res_bmod_are_refused_elsewhere(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    B, H, W, C, cout, seam = 8, 8, 8, 512, 128, 256
    a = RC.dyadic((B, H, W, C), 1).to(dev)
    w3 = RC.dyadic((cout, C, 3, 3), 2).to(dev)
    w1 = RC.dyadic((cout, C, 1, 1), 3).to(dev)
    out = torch.zeros((B, H, W, cout), device=dev)
    P = torch.zeros((B // 2, H, W, cout), device=dev)
    ws = torch.zeros((16 * B * H * W * cout,), device=dev)      # (a grid this small runs with a K split only: never refused for want of a workspace)

    def refused(w_hi, w_lo, **kw):
        assert ops.conv_igemm(None, w_hi, w_lo, out, query_rs=True, ws=ws, **kw) is False
        with pytest.raises(StedmHipError):
            ops.conv_igemm(None, w_hi, w_lo, out, ws=ws, **kw)

    pr = ops.Precision.parse("f16")
    hi = torch.empty((B, H, W, C), dtype=torch.int16, device=dev)
    ops.gn_apply16(a, None, hi, None, pr)
    win = (hi[:, :, :, :seam], None)
    whi3, _ = ops.pack_conv_weight(w3, pr)
    whi1, _ = ops.pack_conv_weight(w1, pr)
    wf3, wf1 = ops.pack_conv_weight_frag(w3, pr), ops.pack_conv_weight_frag(w1, pr)
    # the plain form runs (so that what follows is refused for the reason named)
    assert ops.conv_igemm(None, whi3, None, out, query_rs=True, prec=pr, src16=win, w_frag=wf3, ws=ws)
    assert ops.conv_igemm(None, whi3, None, out, query_rs=True, prec=pr, src16=(hi, None), w_frag=wf3, res=P, res_bmod=B // 2, ws=ws)
    # a window with ks = 1; res_bmod with ks = 1
    refused(whi1, None, prec=pr, ks=1, src16=win, w_frag=wf1)
    refused(whi1, None, prec=pr, ks=1, src16=(hi, None), w_frag=wf1, res=P, res_bmod=B // 2)
    # a window with the fused skip phase
    x16 = torch.empty((B, H, W, 64), dtype=torch.int16, device=dev)
    ops.gn_apply16(RC.dyadic((B, H, W, 64), 4).to(dev), None, x16, None, pr)
    wsk = RC.dyadic((cout, 64, 1, 1), 5).to(dev)
    skip = (x16, ops.pack_conv_weight_frag(wsk, pr), None)
    assert ops.conv_igemm(None, whi3, None, out, query_fused=True, prec=pr, src16=win, w_frag=wf3, skip=skip, ws=ws) is False
    with pytest.raises(StedmHipError):
        ops.conv_igemm(None, whi3, None, out, prec=pr, src16=win, w_frag=wf3, skip=skip, ws=ws)
    # a window with no fragment pack (the LDS-operand kernels); res_bmod there
    refused(whi3, None, prec=pr, src16=win)
    refused(whi3, None, prec=pr, src16=(hi, None), res=P, res_bmod=B // 2)
    # a window in a 3-product mode
    p3 = ops.Precision.parse("parity")
    hi3, lo3 = torch.empty_like(hi), torch.empty_like(hi)
    ops.gn_apply16(a, None, hi3, lo3, p3)
    wh, wl = ops.pack_conv_weight(w3, p3)
    refused(wh, wl, prec=p3, src16=(hi3[:, :, :, :seam], lo3[:, :, :, :seam]), w_frag16=ops.pack_conv_weight_frag16(w3, p3))
    refused(wh, wl, prec=p3, src16=(hi3, lo3), w_frag16=ops.pack_conv_weight_frag16(w3, p3), res=P, res_bmod=B // 2)
    torch.cuda.synchronize()
