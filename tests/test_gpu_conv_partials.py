"""GPU tier (-m gpu): the two halves of a split-K call as calls of their own (stedm_conv_partials / stedm_conv_finish, ABI 24), the
finish pass's ws_bmod, and the second residual res2 of the plain 3x3 kinds - through the C ABI (stedm_amd.ops), against the fp64
references of tests/refs_conv.py, in the two tiers of tests/test_gpu_conv_exact.py / test_gpu_conv_kwindow.py.

Finish pass with ws_bmod: a plain 3x3 convolution at partial batch Bp = 2 leaves its partials; the finish pass writes output batch 4,
sample b from the partial rows of sample b % 2, with bias, the embedding row of sample b, statistics and (with / without) the riding
GroupNorm + SiLU. Shapes (8 x 8 and 16 x 16 pixels; 16 x 16 is one full 256-pixel slab), which form they reach and why:
  two   C 96, w_frag only (16-channel chunks: 6 of them), cout 160: the grid is 2 tiles, far under 3/4 of the chip, so the dispatcher
        splits; 6 chunks halve but do not quarter -> 2 shares, the KSMAX = 2 form of the reduce kernel
  many  C 256, w_frag16 only (32-channel chunks: 8), cout 160: 8 shares, the KSMAX = 16 form
  one   C 32, w_frag, cout = 128 x ceil(3 CUs / 4 / M-tiles): the dispatcher splits a grid of fewer 256-row x 128-channel tiles than 3/4 of
        the chip and refuses it when it cannot, so the smallest grid it runs WITHOUT a split is ceil(3 CUs / 4) tiles (192 on 256 CUs):
        one M-tile (8 x 8: 2 samples of 4 per tile) or two (16 x 16) times that many N-tiles. The launch writes the raw tile sums as
        the one partial; the finish pass runs the KSMAX = 16 form with one plane.
Checked per shape and operand type, for embedding rows None / different in b and b + 2 / equal in b and b + 2, with and without the
riding GroupNorm:
  tier 1 (dyadic operands, every fp32 sum exact): the output equals the fp64 convolution + bias + that row's embedding, torch.equal;
  tier 2 (normal data, operands read back from the planes): |out - ref64| <= G u S, G = refs_conv.G = 8 (the bound of test_gpu_conv_kwindow.py);
  rows b and b + 2 with equal embedding rows carry equal bits (output, statistics, planes);
  rows 0, 1 carry the bits of the ordinary split-K call at batch 2 with the same arguments and workspace size (split forms; the one-partial
    form has no split-K call to compare with: there the rows are held to the ordinary call in tier 1, where every order gives the same bits);
  against a plain call at batch 4 on the duplicated input: equal bits in output, statistics and planes when that call takes the same split
    (asked of the dispatcher), otherwise (another split, or the one-partial form, whose plain call sums in its epilogue) statistics
    and planes are held to the stored output with the bounds of test_gpu_conv_kwindow.py (_check_stats, _check_gn).

res2: the K-window pair at decoder batch 4 (shared batch 2). The route (2B launch with res = p0, res2 = p1) must equal the route through the
reduced P = p0 + p1 (2B launch with res = P) bit for bit, output, statistics and planes:
  split  8 x 8, C 2048 = [0, 1024) + [1024, 2048), w_frag16, cout 1024 (test_gpu_conv_kwindow.py's case c at batch 4): the shared launch
         leaves 2 partials (workspace of two planes), the 2B launch splits K too: res2 in the reduce kernel
  epi    8 x 8, C 96 = [0, 32) + [32, 64) + [64, 96), w_frag, cout as in `one`: nothing splits; p0 / p1 are the partials-only launches of the two
         upper windows, P their finish pass; the 2B launch adds them in its epilogue row loop
and res2 is refused (stedm_conv_rs_ok 0, the call raises) by a fused-skip kind, a 1x1 kind and a 3-product kind."""
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
BP, BO = 2, 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def _unsplit_cout(ops, B, H, W):
    """channels of the smallest grid conv_rs_pick runs without a K split: tiles_m x tiles_n >= 3/4 of the chip"""
    tiles_m = (B * H * W + 255) // 256 if H * W >= 256 else (B + 256 // (H * W) - 1) // (256 // (H * W))
    need = (3 * ops.device_cus() + 3) // 4
    return 128 * ((need + tiles_m - 1) // tiles_m)


SHAPES = [pytest.param(dict(form=f, H=h, W=h), id=f"{f}-{h}x{h}") for f in ("two", "many", "one") for h in (8, 16)]
_OPERANDS = {}


def _shape(ops, c):
    if c["form"] == "two":
        return 96, "f", 160
    if c["form"] == "many":
        return 256, "m", 160
    return 32, "f", _unsplit_cout(ops, BP, c["H"], c["W"])


def _operands(dev, ops, c, tier):
    key = (c["form"], c["H"], tier)
    if key in _OPERANDS:
        return _OPERANDS[key]
    _OPERANDS.clear()
    C, pack, cout = _shape(ops, c)
    H, W = c["H"], c["W"]
    seed = 9100 + 7 * H + sum(ord(ch) for ch in c["form"])
    if tier == 1:
        gen = lambda shape, i, std=1.0: RC.dyadic(shape, 100 * seed + i)
        act = lambda t: t
    else:
        gen = lambda shape, i, std=1.0: RC.normal(shape, 100 * seed + i, "pt", std=std)
        act = lambda t: F.silu(t * 1.3 + 0.1)
    emb = gen((BO, cout + EMB_PAD), 3)
    emb_eq = emb.clone()
    emb_eq[BP:] = emb_eq[:BP]
    o = dict(a=act(gen((BP, H, W, C), 0)), w=gen((cout, C, 3, 3), 1, 1.0 / math.sqrt(C * 9)), bias=gen((cout,), 2, 0.05), emb=emb, emb_eq=emb_eq,
             gamma=RC.normal((cout,), seed + 11, "pt.g", std=0.2, mean=1.0), beta=RC.normal((cout,), seed + 12, "pt.b", std=0.2))
    o = {k: v.to(dev) for k, v in o.items()}
    o.update(C=C, pack=pack, cout=cout, groups=cout // 8)
    _OPERANDS[key] = o
    return o


def _check_stats(cs, out):
    """both planes of every slot against the sums of the stored output (the bounds of tests/test_gpu_conv_kwindow.py)"""
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
    """the riding GroupNorm + SiLU of the stored output in fp64, bound |got - ref| <= u16 |ref| + 1e-4 (1 + |y|) (test_gpu_conv_kwindow.py: _check_gn)"""
    B, H, W, C = out.shape
    groups = o["groups"]
    v = out.double().view(B, H * W, groups, C // groups)
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


def _run_finish_cases(dev, c, prec, tier):
    from stedm_amd import ops
    o = _operands(dev, ops, c, tier)
    pr = ops.Precision.parse(prec)
    H, W, C, cout, pack, groups = c["H"], c["W"], o["C"], o["cout"], o["pack"], o["groups"]
    if tier == 1:
        RC.dyadic_ok(9 * C + 4)
    hi = torch.empty((BP, H, W, C), dtype=torch.int16, device=dev)
    ops.gn_apply16(o["a"], None, hi, None, pr)
    hi4 = torch.cat([hi, hi]).contiguous()
    whi, _ = ops.pack_conv_weight(o["w"], pr)
    wf = ops.pack_conv_weight_frag(o["w"], pr) if "f" in pack else None
    wf16 = ops.pack_conv_weight_frag16(o["w"], pr) if "m" in pack else None
    nslab = ops.gn_chan_nslab(H * W)
    plane = BP * H * W * cout
    shape2 = torch.empty((BP, H, W, cout), device=dev)
    kconv = dict(prec=pr, w_frag=wf, w_frag16=wf16)
    # ---- first half: the partials
    nws = 1 if c["form"] == "one" else 16          # planes of workspace (the one-partial shapes are wide: no room they cannot use)
    ws = torch.full((nws * plane,), NAN, device=dev)
    assert ops.conv_igemm(None, whi, None, shape2, src16=(hi, None), ws=ws, partials=True, query_rs=True, **kconv), "the partials-only launch was expected to run"
    n = ops.conv_igemm(None, whi, None, shape2, src16=(hi, None), ws=ws, partials=True, **kconv)
    assert {"two": n == 2, "many": n > 2, "one": n == 1}[c["form"]], f"form {c['form']}: the dispatcher left {n} partial(s)"
    assert bool(torch.isfinite(ws[:n * plane]).all()) and bool(torch.isnan(ws[n * plane:]).all()), "the partial planes are not exactly the first n of the workspace"
    # the split a plain call at batch 4 on the duplicated input would take (same workspace rule: that many planes of ITS output)
    ws4 = torch.full((nws * 2 * plane,), NAN, device=dev)
    n4 = ops.conv_igemm(None, whi, None, torch.empty((BO, H, W, cout), device=dev), src16=(hi4, None), ws=ws4, partials=True, query_rs=True, **kconv)
    a64 = RC.as_f64(hi, pr.label) if tier == 2 else o["a"].double()
    w64 = RC.as_f64(whi, pr.label) if tier == 2 else RC.otc(o["w"]).double()
    conv2 = RC.conv_ref(a64, w64, "s1", 3)
    conv4 = torch.cat([conv2, conv2])
    S4 = None
    if tier == 2:
        sabs = RC.conv_ref(a64.abs(), w64.abs(), "s1", 3)
        S4 = torch.cat([sabs, sabs])
    worst = 0.0
    for emb_name in (None, "emb", "emb_eq"):
        emb = None if emb_name is None else o[emb_name]
        for gn in (False, True):
            def bufs(B):
                return (torch.full((B, H, W, cout), NAN, device=dev), torch.full((B, nslab, cout, 2), NAN, device=dev),
                        torch.full((B, H, W, cout), 0x7e7e, dtype=torch.int16, device=dev) if gn else None)
            def epi(B, cs, g16):
                k = dict(bias=o["bias"], chan_stats=cs)
                if emb is not None:
                    k.update(emb=emb, emb_offset=EMB_OFF, emb_bstride=emb.shape[1])
                if gn:
                    k.update(gn_next=(o["gamma"], o["beta"], 1e-5, groups, 1, g16))
                return k
            out, cs, g16 = bufs(BO)
            ops.conv_finish(ws, n, out, prec=pr, ws_bmod=BP, **epi(BO, cs, g16))
            assert bool(torch.isfinite(out).all()), "output elements left unwritten"
            ref = RC.epilogue(conv4, o["bias"].double(), None if emb is None else emb.double(), EMB_OFF)
            if tier == 1:
                bad = out.double() != ref
                assert not bool(bad.any()), f"{emb_name} gn={gn}: " + _where(bad)
            else:
                S = RC.epilogue(S4, o["bias"].double().abs(), None if emb is None else emb.double().abs(), EMB_OFF)
                g = (out.double() - ref).abs() / (U * S)
                worst = max(worst, float(g.max()))
                bad = g > G
                assert not bool(bad.any()), f"{emb_name} gn={gn}: max err / (u S) = {float(g.max()):.3f} > G = {G}: " + _where(bad)
            _check_stats(cs, out)
            if gn:
                _check_gn(o, out, g16, pr.label)
            if emb_name != "emb":       # equal (or no) embedding rows: samples b and b + Bp are the same computation
                assert torch.equal(out[:BP], out[BP:]) and torch.equal(cs[:BP], cs[BP:]) and (not gn or torch.equal(g16[:BP], g16[BP:])), \
                    f"{emb_name} gn={gn}: rows b and b + {BP} differ"
            elif tier == 2:
                assert not torch.equal(out[:BP], out[BP:]), "different embedding rows left no trace: the finish pass read the wrong row"
            # rows 0 .. Bp - 1 against the ordinary call at batch Bp with the same arguments
            if n >= 2 or tier == 1:
                o2, cs2, g2 = bufs(BP)
                wsb = torch.full((nws * plane,), NAN, device=dev)
                ops.conv_igemm(None, whi, None, o2, src16=(hi, None), ws=wsb, **epi(BP, cs2, g2), **kconv)
                assert (n >= 2) == (not bool(torch.isnan(wsb).all())), "the ordinary call's split is not the partials-only launch's"
                assert torch.equal(out[:BP], o2), f"{emb_name} gn={gn}: rows 0 .. {BP - 1} are not the ordinary call's"
                if n >= 2:
                    assert torch.equal(cs[:BP], cs2) and (not gn or torch.equal(g16[:BP], g2)), f"{emb_name} gn={gn}: statistics / planes of rows 0 .. {BP - 1} are not the ordinary split-K call's"
            # a plain call at batch 4 on the duplicated input
            if n >= 2 and n4 == n:
                o4, cs4, g4 = bufs(BO)
                ws4.fill_(NAN)
                ops.conv_igemm(None, whi, None, o4, src16=(hi4, None), ws=ws4, **epi(BO, cs4, g4), **kconv)
                assert torch.equal(out, o4) and torch.equal(cs, cs4) and (not gn or torch.equal(g16, g4)), \
                    f"{emb_name} gn={gn}: the plain call at batch {BO} takes the same split ({n}) and gives other bits"
    torch.cuda.synchronize()
    if tier == 2:
        print(f"\n  MEASURED partials {c['form']:4s} {H}x{W} {prec:5s} n={n} (plain batch-4 split {n4}) max err / (u S) = {worst:.3f}", end="")


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("c", SHAPES)
def test_finish_pass_ws_bmod_bit_exact_on_dyadic_operands(dev, c, prec):
    _run_finish_cases(dev, c, prec, 1)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("c", SHAPES)
def test_finish_pass_ws_bmod_operand_exact(dev, c, prec):
    _run_finish_cases(dev, c, prec, 2)


# ================================================================================================ res2
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("form", ["split", "epi"])
def test_res2_route_equals_the_route_through_the_reduced_partial(dev, form, prec):
    from stedm_amd import ops
    pr = ops.Precision.parse(prec)
    H = W = 8
    if form == "split":
        C, seam, pack, cout = 2048, 1024, "m", 1024
        wins = [(seam, C)]
    else:
        C, seam, pack, cout = 96, 32, "f", _unsplit_cout(ops, BP, H, W)
        wins = [(32, 64), (64, 96)]
    groups = cout // 8
    seed = 9900 + (0 if form == "split" else 50)
    a = F.silu(RC.normal((BO, H, W, C), seed, "r2", std=1.0) * 1.3 + 0.1)
    a[BP:, :, :, seam:] = a[:BP, :, :, seam:]
    w = RC.normal((cout, C, 3, 3), seed + 1, "r2", std=1.0 / math.sqrt(C * 9)).to(dev)
    bias, emb = RC.normal((cout,), seed + 2, "r2", std=0.05).to(dev), RC.normal((BO, cout + EMB_PAD), seed + 3, "r2").to(dev)
    gamma, beta = RC.normal((cout,), seed + 4, "r2.g", std=0.2, mean=1.0).to(dev), RC.normal((cout,), seed + 5, "r2.b", std=0.2).to(dev)
    hi = torch.empty((BO, H, W, C), dtype=torch.int16, device=dev)
    ops.gn_apply16(a.to(dev), None, hi, None, pr)
    whi, _ = ops.pack_conv_weight(w, pr)
    wf = ops.pack_conv_weight_frag(w, pr) if "f" in pack else None
    wf16 = ops.pack_conv_weight_frag16(w, pr) if "m" in pack else None
    kconv = dict(prec=pr, w_frag=wf, w_frag16=wf16)
    plane = BP * H * W * cout
    P2 = torch.full((2, BP, H, W, cout), NAN, device=dev)
    P = torch.full((BP, H, W, cout), NAN, device=dev)
    if form == "split":
        # the shared launch with a workspace of two planes: two K shares, left where the kernel wrote them; P by the ordinary call (its reduce pass)
        n = ops.conv_igemm(None, whi, None, P, src16=(hi[:BP, :, :, seam:], None), ws=P2.view(-1), partials=True, **kconv)
        assert n == 2, n
        ops.conv_igemm(None, whi, None, P, src16=(hi[:BP, :, :, seam:], None), ws=torch.full((2 * plane,), NAN, device=dev), **kconv)
    else:
        for i, (k0, k1) in enumerate(wins):
            n = ops.conv_igemm(None, whi, None, P, src16=(hi[:BP, :, :, k0:k1], None), ws=P2[i].view(-1), partials=True, **kconv)
            assert n == 1, n
        ops.conv_finish(P2.view(-1), 2, P, prec=pr)
    assert bool(torch.isfinite(P2).all()) and bool(torch.isfinite(P).all())
    assert torch.equal(P, P2[0] + P2[1]), "the reduced partial is not p0 + p1"
    nslab = ops.gn_chan_nslab(H * W)
    res = []
    for route in ("P", "res2"):
        out = torch.full((BO, H, W, cout), NAN, device=dev)
        cs = torch.full((BO, nslab, cout, 2), NAN, device=dev)
        g16 = torch.full((BO, H, W, cout), 0x7e7e, dtype=torch.int16, device=dev)
        ws2 = torch.full((16 * 2 * plane,), NAN, device=dev) if form == "split" else None
        k2 = dict(src16=(hi[:, :, :, :seam], None), ws=ws2, bias=bias, emb=emb, emb_offset=EMB_OFF, emb_bstride=emb.shape[1], res_bmod=BP, chan_stats=cs,
                  gn_next=(gamma, beta, 1e-5, groups, 1, g16), **kconv)
        k2.update(dict(res=P) if route == "P" else dict(res=P2[0], res2=P2[1]))
        assert ops.conv_igemm(None, whi, None, out, query_rs=True, **k2), "the register-streamed kernel was expected to run the 2B launch"
        ops.conv_igemm(None, whi, None, out, **k2)
        if form == "split":
            assert not bool(torch.isnan(ws2).all()), "the 2B launch was expected to split K (res2 in the reduce kernel)"
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(cs).all())
        res.append((out, cs, g16))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]), _where(res[0][0] != res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    # and the route is the convolution over the full K: operand-exact against fp64
    a64, w64 = RC.as_f64(hi, pr.label), RC.as_f64(whi, pr.label)
    ref = RC.epilogue(RC.conv_ref(a64, w64, "s1", 3), bias.double(), emb.double(), EMB_OFF)
    S = RC.epilogue(RC.conv_ref(a64.abs(), w64.abs(), "s1", 3), bias.double().abs(), emb.double().abs(), EMB_OFF)
    g = (res[1][0].double() - ref).abs() / (U * S)
    print(f"\n  MEASURED res2 {form:5s} {prec:5s} max err / (u S) = {float(g.max()):.3f}", end="")
    assert not bool((g > G).any()), f"max err / (u S) = {float(g.max()):.3f} > G = {G}"


def test_res2_is_refused_elsewhere(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    B, H, W, C, cout = 8, 8, 8, 512, 128
    a = RC.dyadic((B, H, W, C), 1).to(dev)
    w3 = RC.dyadic((cout, C, 3, 3), 2).to(dev)
    w1 = RC.dyadic((cout, C, 1, 1), 3).to(dev)
    out = torch.zeros((B, H, W, cout), device=dev)
    P = torch.zeros((2, B // 2, H, W, cout), device=dev)
    ws = torch.zeros((16 * B * H * W * cout,), device=dev)
    rr = dict(res=P[0], res2=P[1], res_bmod=B // 2)

    def refused(w_hi, w_lo, **kw):
        assert ops.conv_igemm(None, w_hi, w_lo, out, query_rs=True, ws=ws, **kw) is False
        with pytest.raises(StedmHipError):
            ops.conv_igemm(None, w_hi, w_lo, out, ws=ws, **kw)

    pr = ops.Precision.parse("f16")
    hi = torch.empty((B, H, W, C), dtype=torch.int16, device=dev)
    ops.gn_apply16(a, None, hi, None, pr)
    whi3, _ = ops.pack_conv_weight(w3, pr)
    whi1, _ = ops.pack_conv_weight(w1, pr)
    wf3, wf1 = ops.pack_conv_weight_frag(w3, pr), ops.pack_conv_weight_frag(w1, pr)
    # the plain form takes it (so that what follows is refused for the reason named)
    assert ops.conv_igemm(None, whi3, None, out, query_rs=True, prec=pr, src16=(hi, None), w_frag=wf3, ws=ws, **rr)
    # a 1x1 kind
    refused(whi1, None, prec=pr, ks=1, src16=(hi, None), w_frag=wf1, **rr)
    # a fused-skip kind
    x16 = torch.empty((B, H, W, 64), dtype=torch.int16, device=dev)
    ops.gn_apply16(RC.dyadic((B, H, W, 64), 4).to(dev), None, x16, None, pr)
    skip = (x16, ops.pack_conv_weight_frag(RC.dyadic((cout, 64, 1, 1), 5).to(dev), pr), None)
    refused(whi3, None, prec=pr, src16=(hi, None), w_frag=wf3, skip=skip, **rr)
    # a 3-product kind
    p3 = ops.Precision.parse("parity")
    hi3, lo3 = torch.empty_like(hi), torch.empty_like(hi)
    ops.gn_apply16(a, None, hi3, lo3, p3)
    wh, wl = ops.pack_conv_weight(w3, p3)
    refused(wh, wl, prec=p3, src16=(hi3, lo3), w_frag16=ops.pack_conv_weight_frag16(w3, p3), **rr)
    torch.cuda.synchronize()
