"""GPU tier (-m gpu): every form of the implicit-GEMM convolution that conv_rs_pick, conv_rs3_pick and the 128-row launchers behind
stedm_conv_igemm choose between, held against the plain references of tests/refs_conv.py in two tiers that leave the kernel no slack.

  tier 1, bit-exact: dyadic activations, weights, bias, embedding row and residual (refs_bwd.dyadic). Every product is a multiple of 1/64,
    every fp32 partial sum is exact in every order (refs_conv.dyadic_ok states the condition per case), so whatever MFMA shape, chunk order,
    K split or tap fold a form uses, its output must equal the fp64 convolution of the ORIGINAL tensors: torch.equal, no tolerance. One
    missing, doubled or misplaced term fails; so does a pack that rounds. A second, identical launch must give the same bits. On three cases
    (epilogue, split-K reduce, sub-pixel scatter) two more launches produce the 16-bit output: as a side output next to the fp32 one, and as
    the ONLY output (out == NULL, statistics still written); both must be torch's own conversion of the exact value.
  tier 2, operand-exact: normal data (silu(1.3 x + 0.1) activations, 1 / sqrt(K) weights). The operands are read back from the 16-bit planes
    the kernel reads (stedm_gn_apply16 / stedm_space_to_depth16 planes, the [O][taps][I] planes of stedm_pack_conv_weight and
    stedm_pack_conv_weight_up) and convolved in fp64: a reference of the same operation, with the kernel's fp32 accumulation alone between the
    two. Asserted elementwise: |out - ref64| <= G u S, S the same convolution and epilogue on the magnitudes, u = 2^-24,
    G = 16 G_PLAIN = 8 (refs_conv.py: G_PLAIN = 0.5 is the nominal growth factor of a plain fp32 accumulation; torch's CPU convolution
    measures 0.37 .. 0.68 on the CPU tier, so G is below 16 x the largest measurement; neither figure is taken from a kernel). A fragment pack whose rounding differs from the hi planes fails here. The split-product modes run against
    refs_conv.three_products (hi.hi + hi.lo + lo.hi).
  statistics: wherever chan_stats is requested, both planes of every slot against refs_conv.slab_stats of the STORED output:
    |sum - ref| <= n u sum|v|, |sum of squares - ref| <= (n + 1) u sum v^2, n the slot's pixel count.

Every output and statistics buffer is filled with NaN before the call. Which kernel family runs is pinned by what the case packs (only
w_frag: the 32x32x16 kinds; only w_frag16: the 16x16x32 kinds; neither: the LDS-operand 128-row kernels) and asserted through the
capability queries (query_rs / query_fused): that the register-streamed / fused kernel runs, or that it does not. The queries answer with
one bit, so two distinctions rest on something else. A K split: every case that hands over a workspace has a grid the dispatcher admits
only with a split, and the NaN-filled workspace must have been written. RS_1X1N against RS_1X1: rs1x1n_flat meets the N-persistent form's
admission rule as conv_rs_try states it (a flat GEMM, cin <= 256, two N tiles, cout % 8 == 0, M tiles for 3/4 of the chip, no embedding,
no statistics) and is run a second time with STEDM_CONV_NO_NPERS set, which sends it to RS_1X1: both launches must give the same bits,
so either form is held to the exact reference whichever of them the first launch took.

Measured on an MI355X, max over the output of |out - ref64| / (u S), f16 / bf16 (G = 8, G_PLAIN = 0.5):

  lds_3x3_partial_tile   1.69 / 1.59      subm_full              3.07 / 2.50
  lds_3x3_rows           1.42 / 1.68      s2d_a                  1.51 / 1.55
  lds_1x1                1.24 / 1.13      s2d_a_ws               0.83 / 0.81
  lds_down               0.90 / 1.41      s2d_a_br               2.08 / 1.42
  lds_up                 1.53 / 1.31      s2d_a_br_ws            1.13 / 0.92
  lds_up_subpixel        1.94 / 1.75      s2d_b                  1.18 / 1.10
  rs3x3_ragged           2.58 / 2.48      s2d_b_ws               0.82 / 0.80
  rs3x3_two_n_tiles      2.35 / 2.58      s2d_b_br               1.21 / 1.42
  rs3x3m_ragged          2.63 / 2.48      s2d_b_br_ws            1.00 / 0.70
  rs3x3m_16_per_tile     2.24 / 2.90      fused                  1.89 / 2.13
  rs3x3m_odd_chunks      2.89 / 3.01      fused_noemb            2.09 / 1.88
  splitk3x3_b2           0.42 / 0.43      fused_m                2.14 / 2.58
  splitk3x3m_b2          0.36 / 0.43      fused_m_noemb          2.04 / 2.35
  splitk3x3_one_tile     0.38 / 0.39      fused_splitk           0.31 / 0.26
  splitk3x3m_one_tile    0.44 / 0.40      fused_splitk_noemb     0.31 / 0.32
  splitk3x3_k18432       0.35 / 0.38      fused_m_splitk         0.37 / 0.28
  splitk3x3m_k18432      0.33 / 0.36      fused_m_splitk_noemb   0.29 / 0.47
  rs1x1_partial_tile     2.73 / 2.59      wide_rows              2.26 / 2.21
  rs1x1_two_n_tiles      2.62 / 2.58      p3_rs3x3m              4.42 / 4.10
  rs1x1n_flat            2.91 / 2.59      p3_rs1x1m              3.46 / 3.43
  splitk1x1              0.58 / 0.64      p3_subm                4.61 / 4.27
  sub_full               2.66 / 2.44      p3_lds_3x3             2.35 / 2.75
  sub_splitk             0.73 / 0.70      p3_lds_1x1             2.08 / 2.09

(p3_*: the split-product modes, parity / parity_bf16. The largest single-product figure is 3.07, the largest of all 4.61: the K-split forms
stay under 1 because each share's partial sum is short; no form comes near G.)
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import refs_conv as RC

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
U = RC.U
G = RC.G
EMB_OFF, EMB_PAD = 8, 24          # the embedding row sits at an offset inside a wider row (offset + batch stride), as the U-Net passes it


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def case(name, B, H, W, cin, cout, mode="s1", ks=3, pack="f", ws=False, emb=True, res=True, stats="runs", rs=True, pad_br=False, cb=0, o16=False):
    """mode: s1 | down (CONV_DOWN) | up (CONV_UP) | up2 (CONV_UP_SUBPIXEL) | s2d (CONV_S2D). pack: 'f' = w_frag only (32x32x16 kinds),
    'm' = w_frag16 only (16x16x32 kinds), '' = no fragment pack (LDS-operand kernels). stats: None | 'runs' (row-major runs: 256 pixels,
    or the caller's partition) | 'parity' (the sub-pixel epilogue's (run, output parity) slots). rs: what the capability query must say.
    cb: channels of the fused skip_connection's 1x1 (0: none)."""
    return pytest.param(dict(name=name, B=B, H=H, W=W, cin=cin, cout=cout, mode=mode, ks=ks, pack=pack, ws=ws, emb=emb, res=res, stats=stats,
                             rs=rs, pad_br=pad_br, cb=cb, o16=o16), id=name)


SINGLE = [
    # ---- LDS-operand 128-row kernels: no fragment pack
    case("lds_3x3_partial_tile", 3, 8, 8, 64, 96, pack="", rs=False),
    case("lds_3x3_rows", 1, 32, 32, 32, 32, pack="", rs=False),
    case("lds_1x1", 3, 4, 4, 128, 96, ks=1, pack="", rs=False),
    case("lds_down", 3, 8, 8, 32, 32, mode="down", pack="", rs=False),
    case("lds_up", 3, 4, 4, 32, 32, mode="up", pack="", rs=False),
    case("lds_up_subpixel", 3, 4, 4, 32, 32, mode="up2", pack="", rs=False),
    # ---- RS_3X3 on a full grid: 4 samples per tile + ragged last tile + masked N; two N tiles with rows inside a sample
    case("rs3x3_ragged", 771, 8, 8, 32, 96, o16=True),
    case("rs3x3_two_n_tiles", 25, 32, 32, 32, 160),
    # ---- RS_3X3M (cin >= 256, only w_frag16 packed): 4 and 16 samples per tile, an odd chunk count
    case("rs3x3m_ragged", 771, 8, 8, 256, 96, pack="m"),
    case("rs3x3m_16_per_tile", 3089, 4, 4, 256, 32, pack="m"),
    case("rs3x3m_odd_chunks", 97, 16, 16, 288, 160, pack="m"),
    # ---- split-K 3x3 with the reduce pass's statistics, both MFMA kinds
    case("splitk3x3_b2", 2, 8, 8, 1024, 1024, ws=True, o16=True),
    case("splitk3x3m_b2", 2, 8, 8, 1024, 1024, pack="m", ws=True),
    case("splitk3x3_one_tile", 1, 16, 16, 512, 128, ws=True),
    case("splitk3x3m_one_tile", 1, 16, 16, 512, 128, pack="m", ws=True),
    case("splitk3x3_k18432", 4, 8, 8, 2048, 1024, ws=True),
    case("splitk3x3m_k18432", 4, 8, 8, 2048, 1024, pack="m", ws=True),
    # ---- 1x1: tiled (M = 49300, partial last tile), two N tiles, the N-persistent form (a flat GEMM: B = 1; no embedding, no statistics), split K
    case("rs1x1_partial_tile", 493, 10, 10, 64, 96, ks=1),
    case("rs1x1_two_n_tiles", 493, 10, 10, 128, 200, ks=1, emb=False, stats=None),
    case("rs1x1n_flat", 1, 1, 49300, 128, 200, ks=1, emb=False, stats=None),
    case("splitk1x1", 2, 8, 8, 2048, 1024, ks=1, ws=True),
    # ---- sub-pixel Upsample: RS_SUB on a full grid (4 parities x 49 tiles) and split K; RS_SUBM when only the 16x16x32 order is packed
    case("sub_full", 193, 8, 8, 32, 96, mode="up2", stats="parity", o16=True),
    case("sub_splitk", 2, 8, 8, 1024, 1024, mode="up2", ws=True),
    case("subm_full", 193, 8, 8, 32, 96, mode="up2", pack="m", stats="parity"),
    # ---- space-to-depth Downsample, both paddings, with and without the workspace
    case("s2d_a", 5, 16, 16, 64, 96, mode="s2d"),
    case("s2d_a_ws", 5, 16, 16, 64, 96, mode="s2d", ws=True),
    case("s2d_a_br", 5, 16, 16, 64, 96, mode="s2d", pad_br=True),
    case("s2d_a_br_ws", 5, 16, 16, 64, 96, mode="s2d", pad_br=True, ws=True),
    case("s2d_b", 3, 8, 8, 32, 32, mode="s2d"),
    case("s2d_b_ws", 3, 8, 8, 32, 32, mode="s2d", ws=True),
    case("s2d_b_br", 3, 8, 8, 32, 32, mode="s2d", pad_br=True),
    case("s2d_b_br_ws", 3, 8, 8, 32, 32, mode="s2d", pad_br=True, ws=True),
    # ---- fused skip_connection phase: 32x32x16, 16x16x32, split K (both), each with and without the embedding row
    case("fused", 771, 8, 8, 32, 96, cb=64, res=False),
    case("fused_noemb", 771, 8, 8, 32, 96, cb=64, res=False, emb=False),
    case("fused_m", 771, 8, 8, 256, 96, cb=128, pack="m", res=False),
    case("fused_m_noemb", 771, 8, 8, 256, 96, cb=128, pack="m", res=False, emb=False),
    case("fused_splitk", 2, 8, 8, 1024, 1024, cb=2048, ws=True, res=False),
    case("fused_splitk_noemb", 2, 8, 8, 1024, 1024, cb=2048, ws=True, res=False, emb=False),
    case("fused_m_splitk", 2, 8, 8, 1024, 1024, cb=2048, pack="m", ws=True, res=False),
    case("fused_m_splitk_noemb", 2, 8, 8, 1024, 1024, cb=2048, pack="m", ws=True, res=False, emb=False),
    # ---- rows wider than the tile: 192 row-run tiles
    case("wide_rows", 1, 96, 512, 32, 32),
]

THREE = [   # the split-product modes: RS_3X3M / RS_1X1M / RS_SUBM with hi + lo streams (only w_frag16 packed), and the LDS-operand 3-product kernel
    case("p3_rs3x3m", 771, 8, 8, 256, 96, pack="m"),
    case("p3_rs1x1m", 493, 10, 10, 64, 96, ks=1, pack="m"),
    case("p3_subm", 193, 8, 8, 128, 96, mode="up2", pack="m", stats="parity"),
    case("p3_lds_3x3", 3, 8, 8, 64, 96, pack="", rs=False),
    case("p3_lds_1x1", 3, 4, 4, 128, 96, ks=1, pack="", rs=False),
]


otc = RC.otc


_OPERANDS = {}          # one entry: the operands (and the tier-1 reference) of the case at hand, shared by its f16 / bf16 runs


def _operands(dev, c, tier):
    """fp32 operands on the device: a NHWC, w OIHW, bias, emb [B][cout + EMB_PAD], res NHWC, and of the fused 1x1: x NHWC, w1 OIHW, b1"""
    key = (c["name"], tier)
    if key in _OPERANDS:
        return _OPERANDS[key]
    _OPERANDS.clear()
    B, H, W, cin, cout, ks, cb = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["ks"], c["cb"]
    Ho, Wo = RC.out_hw(H, W, {"s2d": "down", "up2": "up"}.get(c["mode"], c["mode"]))
    seed = sum(ord(ch) for ch in c["name"])
    if tier == 1:
        gen = lambda shape, i, std=1.0: RC.dyadic(shape, 100 * seed + i)
        act = lambda t: t
    else:
        gen = lambda shape, i, std=1.0: RC.normal(shape, 100 * seed + i, "cx", std=std)
        act = lambda t: F.silu(t * 1.3 + 0.1)                      # stands for the normalised + activated activation
    o = dict(a=act(gen((B, H, W, cin), 0)), w=gen((cout, cin, ks, ks), 1, 1.0 / math.sqrt(cin * ks * ks)), bias=gen((cout,), 2, 0.05),
             emb=gen((B, cout + EMB_PAD), 3) if c["emb"] else None, res=gen((B, Ho, Wo, cout), 4) if c["res"] else None)
    if cb:
        o.update(x=gen((B, H, W, cb), 5), w1=gen((cout, cb, 1, 1), 6, 1.0 / math.sqrt(cb)), b1=gen((cout,), 7, 0.05))
    o = {k: (None if v is None else v.to(dev)) for k, v in o.items()}
    _OPERANDS[key] = o
    return o


def _conv_fn(c):
    """the case's convolution as a function of (activations NHWC, weights [O][taps][I] or, sub-pixel, [4][O][4][I])"""
    if c["mode"] == "up2":
        return RC.conv_ref_subpixel
    mode = {"s2d": "down"}.get(c["mode"], c["mode"])
    return lambda a_, w_: RC.conv_ref(a_, w_, mode, c["ks"], c["pad_br"])


def _launch(dev, c, prec_name, o, extra=False):
    """packs, planes and two identical launches into NaN-filled buffers. extra: further launches of the same problem - the 16-bit output as
    a side output and as the only output (o16 cases), the tiled twin of the N-persistent 1x1. Returns (out, chan_stats, out16) of every
    launch and the planes the kernel read."""
    from stedm_amd import ops
    from stedm_amd._lib import CONV_DOWN, CONV_S1, CONV_S2D, CONV_UP, CONV_UP_SUBPIXEL
    pr = ops.Precision.parse(prec_name)
    p3 = pr.npass == 3
    B, H, W, cin, cout, ks, cb, mode, pack = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["ks"], c["cb"], c["mode"], c["pack"]
    Ho, Wo = RC.out_hw(H, W, {"s2d": "down", "up2": "up"}.get(mode, mode))
    a, w = o["a"], o["w"]
    pl = dict()
    if mode == "s2d":
        hi = torch.empty((B, H // 2, W // 2, 4 * cin), dtype=torch.int16, device=dev); lo = torch.empty_like(hi) if p3 else None
        ops.space_to_depth16(a, hi, lo, pr)
        # the planes hold pixel (2y + py, 2x + px) in channel block py * 2 + px
        unfold = lambda t: t.view(B, H // 2, W // 2, 2, 2, cin).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, cin)
        pl["ah"] = unfold(RC.as_f64(hi, pr.label)); pl["al"] = unfold(RC.as_f64(lo, pr.label)) if p3 else None
    else:
        hi = torch.empty((B, H, W, cin), dtype=torch.int16, device=dev); lo = torch.empty_like(hi) if p3 else None
        ops.gn_apply16(a, None, hi, lo, pr)
        pl["ah"] = RC.as_f64(hi, pr.label); pl["al"] = RC.as_f64(lo, pr.label) if p3 else None
    if mode == "up2":
        whi, wlo = ops.pack_conv_weight_up(w, pr)
        pl["wh"] = RC.as_f64(whi, pr.label).view(4, cout, 4, cin); pl["wl"] = RC.as_f64(wlo, pr.label).view(4, cout, 4, cin) if p3 else None
    else:
        whi, wlo = ops.pack_conv_weight(w, pr)
        pl["wh"] = RC.as_f64(whi, pr.label); pl["wl"] = RC.as_f64(wlo, pr.label) if p3 else None
    wf = wf16 = None
    if "f" in pack:
        wf = {"up2": ops.pack_conv_weight_up_frag, "s2d": lambda w_, p_: ops.pack_conv_weight_s2d_frag(w_, p_, c["pad_br"])}.get(mode, ops.pack_conv_weight_frag)(w, pr)
    if "m" in pack:
        wf16 = {"up2": ops.pack_conv_weight_up_frag16_hl, "s2d": lambda w_, p_: ops.pack_conv_weight_s2d_frag16_hl(w_, p_, c["pad_br"])}.get(mode, ops.pack_conv_weight_frag16)(w, pr)
    m = {"s1": CONV_S1, "down": CONV_DOWN, "up": CONV_UP, "up2": CONV_UP_SUBPIXEL, "s2d": CONV_S2D}[mode]
    # stride-2 patches can exceed LDS in the 128-row DMA kernel: the fp32 source lets the dispatcher fall back. It holds the plane's values, so
    # that either kernel multiplies the same operands
    src1 = pl["ah"].float().contiguous() if mode == "down" else None
    kw = dict(prec=pr, ks=ks, mode=m, src16=(hi, lo), bias=o["bias"], emb=o["emb"], emb_offset=EMB_OFF if o["emb"] is not None else 0,
              emb_bstride=0 if o["emb"] is None else o["emb"].shape[1], res=o["res"], w_frag=wf, w_frag16=wf16, pad_br=c["pad_br"])
    if mode == "s2d":
        whi = wlo = None
    if cb:
        x16 = torch.empty((B, H, W, cb), dtype=torch.int16, device=dev)
        ops.gn_apply16(o["x"], None, x16, None, pr)
        pl["xh"] = RC.as_f64(x16, pr.label); pl["w1h"] = RC.as_f64(ops.pack_conv_weight(o["w1"], pr)[0], pr.label)
        kw["skip"] = (x16, ops.pack_conv_weight_frag(o["w1"], pr), o["b1"]) + ((ops.pack_conv_weight_frag16(o["w1"], pr),) if "m" in pack else ())
    if c["stats"]:
        nslab = 4 * ops.gn_chan_nslab(H * W) if mode == "up2" else ops.gn_chan_nslab(Ho * Wo)
    kinds = ["plain", "plain"] + (["side16", "only16"] if extra and c["o16"] else []) + (["no_npers"] if extra and c["name"] == "rs1x1n_flat" else [])
    runs = []
    for kind in kinds:
        out = torch.full((B, Ho, Wo, cout), NAN, device=dev) if kind != "only16" else None
        cs = torch.full((B, nslab, cout, 2), NAN, device=dev) if c["stats"] else None
        ws = torch.full((16 * B * Ho * Wo * cout,), NAN, device=dev) if c["ws"] else None
        k = dict(kw, chan_stats=cs, ws=ws)
        o16 = None
        if kind in ("side16", "only16"):
            o16 = torch.full((B, Ho, Wo, cout), 0x7e7e, dtype=torch.int16, device=dev)
            k["out16"] = (o16, None)
        # the intended kernel family must (not) be the one that runs
        if cb:
            assert ops.conv_igemm(src1, whi, wlo, out, query_fused=True, **k), "the fused skip phase was expected to run as one kernel"
        else:
            assert ops.conv_igemm(src1, whi, wlo, out, query_rs=True, **k) == c["rs"], f"register-streamed kernel expected: {c['rs']}"
        if kind == "no_npers":
            os.environ["STEDM_CONV_NO_NPERS"] = "1"
        try:
            ops.conv_igemm(src1, whi, wlo, out, **k)
        finally:
            os.environ.pop("STEDM_CONV_NO_NPERS", None)
        # every case that hands over a workspace is sized for the K split: the partial tiles must have landed in it
        assert ws is None or not bool(torch.isnan(ws).all()), "the K split did not run: the workspace is untouched"
        runs.append((out, cs, o16))
    torch.cuda.synchronize()
    return pr, pl, runs


def _check_stats(c, cs, out):
    """both planes of every slot against the sums of the stored output"""
    if cs is None:
        return
    B, Ho, Wo, cout = out.shape
    HWo = Ho * Wo
    nslab = cs.shape[1]
    if c["stats"] == "parity":
        idx = RC.slot_parity(c["H"], c["W"], out.device)
    else:
        idx = RC.slot_runs(HWo, 256 if nslab == (HWo + 255) // 256 else HWo // nslab, out.device)
    s, q = RC.slab_stats(out, idx)
    sa, _ = RC.slab_stats(out.abs(), idx)
    n = torch.bincount(idx, minlength=nslab).double()[None, :, None]
    assert s.shape[1] == nslab and bool(torch.isfinite(cs).all()), "statistics slots left unwritten"
    e0 = (cs[..., 0].double() - s).abs(); e1 = (cs[..., 1].double() - q).abs()
    assert bool((e0 <= n * U * sa).all()), f"sum: worst error / bound {float((e0 / (n * U * sa).clamp_min(1e-300)).max()):.3g}"
    assert bool((e1 <= (n + 1) * U * q).all()), f"sum of squares: worst error / bound {float((e1 / ((n + 1) * U * q).clamp_min(1e-300)).max()):.3g}"


def _reference(c, a, w, conv, o, x=None, w1=None):
    ref = conv(a, w)
    if c["cb"]:
        ref = ref + RC.conv_ref(x, w1, "s1", 1) + o["b1"].double()
    return RC.epilogue(ref, o["bias"].double(), None if o["emb"] is None else o["emb"].double(), EMB_OFF, None if o["res"] is None else o["res"].double())


def _where(out, bad):
    i = bad.nonzero()
    return f"{int(bad.sum())} of {bad.numel()} elements differ, first at [b, y, x, n] = {i[0].tolist()}, last at {i[-1].tolist()}"


# ================================================================================================ tier 1: bit-exact
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("c", SINGLE)
def test_conv_bit_exact_on_dyadic_operands(dev, c, prec):
    o = _operands(dev, c, 1)
    if c["mode"] == "up2":      # the pre-summed taps reach |4|; the reference is nearest-2x + 3x3 on the unfolded filter
        RC.dyadic_ok(4 * c["cin"] + 3, wmax=4.0)
    else:
        RC.dyadic_ok(c["ks"] ** 2 * c["cin"] + c["cb"] + 4)
    if "ref" not in o:
        conv = (lambda a_, w_: RC.conv_ref(a_, w_, "up", 3)) if c["mode"] == "up2" else _conv_fn(c)
        o["ref"] = _reference(c, o["a"].double(), otc(o["w"]).double(), conv, o,
                              None if not c["cb"] else o["x"].double(), None if not c["cb"] else otc(o["w1"]).double())
        assert bool((o["ref"] * 64 == (o["ref"] * 64).round()).all()) and float(o["ref"].abs().max()) * 64 < 2 ** 24
    ref = o["ref"]
    pr, pl, runs = _launch(dev, c, prec, o, extra=True)
    out, cs, _ = runs[0]
    bad = out.double() != ref
    assert not bool(bad.any()), _where(out, bad)
    assert torch.equal(out.double(), ref)
    assert torch.equal(runs[1][0], out) and (cs is None or torch.equal(runs[1][1], cs)), "the second run differs from the first"
    _check_stats(c, cs, out)
    dt = torch.float16 if pr.label.startswith("f16") else torch.bfloat16
    for o2, cs2, o16 in runs[2:]:      # the 16-bit output beside the fp32 one, then alone; the tiled twin of the N-persistent 1x1
        assert o2 is None or torch.equal(o2, out)
        assert cs is None or torch.equal(cs2, cs), "the statistics differ from the plain launch's"
        assert o16 is None or torch.equal(o16.view(dt), ref.float().to(dt))
    assert len(runs) == 2 + (2 if c["o16"] else 0) + (1 if c["name"] == "rs1x1n_flat" else 0)


# ================================================================================================ tier 2: operand-exact
def _operand_exact(dev, c, prec):
    o = _operands(dev, c, 2)
    pr, pl, runs = _launch(dev, c, prec, o)
    out, cs, _ = runs[0]
    conv = _conv_fn(c)
    if pr.npass == 3:
        ref = _reference(c, None, None, lambda *_: RC.three_products(pl["ah"], pl["al"], pl["wh"], pl["wl"], conv), o)
        am, wm = pl["ah"].abs() + pl["al"].abs(), pl["wh"].abs() + pl["wl"].abs()
    else:
        ref = _reference(c, pl["ah"], pl["wh"], conv, o, pl.get("xh"), pl.get("w1h"))
        am, wm = pl["ah"], pl["wh"]
    ab = lambda t: None if t is None else t.double().abs()
    S = RC.abs_sum(am, wm, conv, ab(o["bias"]), ab(o["emb"]), EMB_OFF, ab(o["res"]))
    if c["cb"]:
        S = S + RC.conv_ref(pl["xh"].abs(), pl["w1h"].abs(), "s1", 1) + o["b1"].double().abs()
    assert bool(torch.isfinite(out).all()), "output elements left unwritten"
    g = (out.double() - ref).abs() / (U * S)
    print(f"\n  MEASURED {c['name']:24s} {prec:12s} max err / (u S) = {float(g.max()):.3f}   (err / std(ref) = {float((out.double() - ref).abs().max() / ref.std()):.2e})", end="")
    bad = g > G
    assert not bool(bad.any()), f"max err / (u S) = {float(g.max()):.3f} > G = {G}: " + _where(out, bad)
    assert torch.equal(runs[1][0], out) and (cs is None or torch.equal(runs[1][1], cs)), "the second run differs from the first"
    _check_stats(c, cs, out)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("c", SINGLE)
def test_conv_operand_exact_single_product(dev, c, prec):
    _operand_exact(dev, c, prec)


@pytest.mark.parametrize("prec", ["parity", "parity_bf16"])
@pytest.mark.parametrize("c", THREE)
def test_conv_operand_exact_three_products(dev, c, prec):
    _operand_exact(dev, c, prec)
