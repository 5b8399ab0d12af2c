"""GPU tier (-m gpu): the attention kernels of attn.hip, svit.hip, attn_fp8.hip and swin.hip, called directly through their ops.* entries
and held against tests/refs_attn.py in two tiers (the style of tests/test_gpu_conv_exact.py; tests/test_attn_refs_cpu.py proves on the CPU
that both tiers reject a dropped / doubled / swapped key, an off-by-one key mask, a skipped rescale, a missing diagonal mask, a wrong
roll and an ignored region mask):

  tier 1, exact (every case): selector inputs (refs_attn.one_hot, refs_attn.group; for T > 64 refs_attn.late: the whole first key tile
    far below every target; for ch >= 32 refs_attn.below_zero: every logit negative, so a zero key row beyond T would take the row if the
    tail mask let it through) whose output is a known integer or quarter-integer.
    Expected-output rule: torch.equal for EVERY softmax kernel here. attn_legacy_kernel, attn64_mfma_kernel and lsa_flash_kernel subtract
    the row maximum, so the target's p is exp(0) = 1; attn_flash_kernel, lsa_flash64_kernel and lsa_flash64_mx8_kernel exponentiate
    relative to a reference (rounded to the operand type in the first two): the sign codes make every logit a multiple of 256 below 2^16,
    exactly representable in f16 and bf16, so the reference IS the row maximum and p = 1 there too (stricter than a 2 u_T |v| allowance,
    which the rounded reference would need for general logits). Every other key is >= 160 nats below: p = 0 exactly. l = 1, 2 or 4.
    Dropout at p = 0.5 scales by exactly 2: expected 0 or 2 v under the oracle's mask. Swin's cosine logits are bounded by the scale, so
    its tier 1 is `uniform` (q = 0, rpb = 0, v = the bits of the source token's (y, x, sample)): every output is the fraction of set bits
    among the keys of the query's window and shift region, asserted within 2 u_T (one wrong token moves a channel by >= 1 / 64).
  tier 2, per element (every case): random operands rounded as the kernel receives them, |out - ref64| <= refs_attn.bound (each kernel's
    own rounding points, no free factor). The worst err / bound is printed.

Outputs are pre-filled with NaN words; a second identical call must give the same bits; everything must be finite.

Measured on an MI355X, worst err / bound per kernel over its cases (the fp32 emulation of the CPU tier in brackets); no case failed
tier 2, and tier 1 failed only on `late` before the fix named below:

  attn_legacy fp32            0.022 (0.022)     lsa_flash<3> parity        0.007 (0.014)     swin f16                 0.444 (0.444)
  attn64_mfma f16, rows       0.380 (0.380)     lsa_flash<3> parity_bf16   0.034 (0.034)     swin bf16                0.573 (0.573)
  attn64_mfma f16, plane      0.380             lsa_flash64 f16            0.460 (0.460)     swin f16, int16 qkv      0.471 (0.471)
  attn64_mfma bf16, rows      0.488 (0.488)     lsa_flash64 bf16           0.449 (0.449)     swin bf16, int16 qkv     0.602 (0.602)
  attn64_mfma bf16, plane     0.488             lsa_flash64<drop> f16      0.498 (0.498)     swin parity              0.004 (0.006)
  attn_flash f16              0.502 (0.502)     lsa_flash64<drop> bf16     0.497 (0.497)     swin parity_bf16         0.031 (0.027)
  attn_flash bf16             0.596 (0.596)     lsa_flash<3, drop> parity  0.006 (0.009)     lsa_flash64_mx8          0.344 (0.344)

In e4m3 (lsa_flash64_mx8, u = 2^-4) tier 2 separates a dropped / doubled / swapped key and a missing diagonal mask by only 4 .. 21 times
the bound and does not separate an off-by-one tail mask at all (tests/test_attn_refs_cpu.py): tier 1 is the guard for that kernel.

(The one-product figures sit at half the bound and equal the emulation's to three digits: the bound is the two 16-bit roundings and
little else, and those are deterministic. The three-product bounds are dominated by the lo.lo terms the modes drop by design.)

Found by `late`: attn_flash_kernel, lsa_flash64_kernel and lsa_flash64_mx8_kernel rescaled their still-empty l and O by
exp2(-reference) when they set the reference on the first tile; a first tile more than 128 log2 units below zero made the factor inf
and every output of the row 0 * inf = NaN (all rows of the `late` cases, f16 and bf16). The factor is finite on the first tile now.
"""

import pytest
import torch

from tests import refs_attn as R

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NANW = 0x7FFF              # a NaN in f16 and in bf16
I16 = torch.int16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def _prec(name):
    from stedm_amd import ops
    pr = ops.Precision.parse(name)
    want = {"f16": (ops.F16, 1), "bf16": (ops.BF16, 1), "parity": (ops.F16, 3), "parity_bf16": (ops.BF16, 3), "fp8": (ops.BF16, 1)}[name]
    assert (pr.mm_dtype, pr.npass) == want                   # the instantiation the entry will pick
    return pr


def _twice(run):
    """the result of a call, after a second identical call gave the same bits and everything was finite"""
    a, b = run(), run()
    bad = (~torch.isfinite(a)).any(-1).nonzero()
    assert bad.numel() == 0, f"NaN / inf (or an output element that was never written) in {bad.shape[0]} rows, first {bad[0].tolist()}"
    assert torch.equal(a, b), "two identical calls differ"
    return a


def _check(tag, run, ref_fn, bound_fn, sel_cases, t2_case):
    """tier 1 on every selector case (name, q, k, v, expected), tier 2 on (q, k, v); returns the worst err / bound"""
    for name, q, k, v, ex in sel_cases:
        got = _twice(lambda: run(q, k, v))
        bad = (got != ex).any(-1).nonzero()
        assert bad.numel() == 0, f"{tag} {name}: {bad.shape[0]} wrong rows, first (problem, query) {bad[0].tolist()}, key tile of the query {int(bad[0][1]) // 64}"
    q, k, v = t2_case
    r = ref_fn(q, k, v)
    R.assert_spread(r)
    got = _twice(lambda: run(q, k, v))
    ratio = float(((got - r["out"]).abs() / bound_fn(r, q, k, v)).max())
    print(f"[{tag}] tier 1 exact; tier 2 worst err / bound {ratio:.3f} (logit spread {r['spread']:.1f} log2 units)")
    assert ratio <= 1.0, ratio
    return ratio


def _selectors(P, T, ch, diag=False):
    q, k, v, ex, _ = R.one_hot(P, T, ch, seed=T + ch)
    assert torch.equal(ex, R.selector_expected(q, k, v, diag))
    q2, k2, v2, ex2, _ = R.group(P, T, ch, seed=T + ch, diag=diag)
    assert torch.equal(ex2, R.selector_expected(q2, k2, v2, diag))
    sel = [("one_hot", q, k, v, ex), ("group", q2, k2, v2, ex2)]
    if T > 64:                                     # the first key tile far below every target: a first-tile reference must not produce 0 * inf
        q3, k3, v3, ex3, _ = R.late(P, T, ch, seed=T + ch, diag=diag)
        assert torch.equal(ex3, R.selector_expected(q3, k3, v3, diag))
        sel.append(("late", q3, k3, v3, ex3))
    if ch >= 32:                                   # every logit negative: a zero key row beyond T must not outrank the real keys
        q4, k4, v4, ex4, _ = R.below_zero(P, T, ch, seed=T + ch, diag=diag)
        assert torch.equal(ex4, R.selector_expected(q4, k4, v4, diag))
        sel.append(("below_zero", q4, k4, v4, ex4))
    return sel


# ------------------------------------------------------------------------------------------------ QKVAttentionLegacy
@pytest.mark.parametrize("B,T,heads,ch", R.CASES["attn_legacy"])
def test_attn_legacy_fp32(dev, B, T, heads, ch):
    from stedm_amd import ops

    def run(q, k, v):
        qkv = R.legacy_pack(q, k, v, B, heads).float().to(dev)
        out = torch.full((B, T, heads * ch), float("nan"), device=dev)
        ops.attn_legacy(qkv, out, heads)
        return R.legacy_unpack(out.cpu().double(), B, heads)
    _check(f"attn_legacy fp32 B{B} T{T} h{heads} ch{ch}", run, R.legacy_ref,
           lambda r, q, k, v: R.tier2_bound("attn_legacy", "fp32", r, q, k, v, T, ch), _selectors(B * heads, T, ch),
           R.tier2_inputs("attn_legacy", "fp32", B * heads, T, ch, seed=7 * T + ch))


def _run_legacy16(dev, B, T, heads, ch, precision, plane):
    from stedm_amd import ops
    pr, dt = _prec(precision), R.DTYPES[precision]

    def run(q, k, v):
        qkv = R.legacy_pack(q, k, v, B, heads)
        assert torch.equal(qkv.to(dt).double(), qkv)         # the operands are exact in the type: both input forms carry the same values
        src = qkv.to(dt).view(I16).to(dev) if plane else qkv.float().to(dev)
        out = torch.full((B, T, heads * ch), NANW, dtype=I16, device=dev)
        ops.attn_legacy16(src, out, heads, pr)
        return R.legacy_unpack(out.cpu().view(dt).double(), B, heads)
    return run


@pytest.mark.parametrize("plane", [False, True], ids=["fp32rows", "int16plane"])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("B,T,heads,ch", R.CASES["attn64"])
def test_attn64_mfma(dev, B, T, heads, ch, precision, plane):
    assert T == 64 and ch in (32, 64, 128) and (B * heads) % 4 != 0         # attn64_mfma_kernel<T, ch, plane>, a workgroup with dead waves
    _check(f"attn64_mfma {precision} ch{ch} {'int16 plane' if plane else 'fp32 rows'}", _run_legacy16(dev, B, T, heads, ch, precision, plane),
           R.legacy_ref, lambda r, q, k, v: R.tier2_bound("attn64", precision, r, q, k, v, T, ch), _selectors(B * heads, T, ch),
           R.tier2_inputs("attn64", precision, B * heads, T, ch, seed=7 * T + ch))


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("B,T,heads,ch", R.CASES["attn_flash"])
def test_attn_flash_four_wave_form(dev, B, T, heads, ch, precision):
    assert T != 64 and not (T >= 1024 and ch == 128)                          # attn_flash_kernel<T, ch, 4, 2>
    _check(f"attn_flash {precision} B{B} T{T} h{heads} ch{ch}", _run_legacy16(dev, B, T, heads, ch, precision, True),
           R.legacy_ref, lambda r, q, k, v: R.tier2_bound("attn_flash", precision, r, q, k, v, T, ch), _selectors(B * heads, T, ch),
           R.tier2_inputs("attn_flash", precision, B * heads, T, ch, seed=7 * T + ch))


# ------------------------------------------------------------------------------------------------ LSA
def _run_lsa(dev, B, T, heads, precision, drop=None):
    from stedm_amd import ops
    pr, dt = _prec(precision), R.DTYPES[precision]
    Tp = (T + 127) // 128 * 128
    lo = pr.npass == 3

    def run(q, k, v):
        planes = R.lsa_planes(q, k, v, Tp, dt, lo=lo)
        for (hi, l_), x, tr in zip(planes, (q, k, v), (False, False, True)):       # the planes hold the problem's values exactly
            back = hi.view(dt).double() + (l_.view(dt).double() if lo else 0)
            back = back.transpose(1, 2) if tr else back
            assert torch.equal(back[:, :T], x)
        qd, kd, vd = (tuple(None if t is None else t.to(dev) for t in pl) for pl in planes)
        od = (torch.full((B, T, heads * 64), NANW, dtype=I16, device=dev), torch.full((B, T, heads * 64), NANW, dtype=I16, device=dev) if lo else None)
        if drop is None:
            ops.lsa_flash(qd, kd, vd, od, B, T, Tp, heads, pr)
        else:
            ops.lsa_flash_drop(qd, kd, vd, od, B, T, Tp, heads, pr, *drop)
        out = od[0].cpu().view(dt).double() + (od[1].cpu().view(dt).double() if lo else 0)
        return R.legacy_unpack(out, B, heads)
    return run


@pytest.mark.parametrize("precision", ["parity", "parity_bf16", "f16", "bf16"])
@pytest.mark.parametrize("B,T,heads,ch", R.CASES["lsa64"])
def test_lsa_flash(dev, B, T, heads, ch, precision):
    """parity / parity_bf16: lsa_flash_kernel<T, 3> (hi + lo planes); f16 / bf16: lsa_flash64_kernel<T>"""
    kernel = "lsa_parity" if precision.startswith("parity") else "lsa64"
    _check(f"{kernel} {precision} B{B} T{T} h{heads}", _run_lsa(dev, B, T, heads, precision), R.lsa_ref,
           lambda r, q, k, v: R.tier2_bound(kernel, precision, r, q, k, v, T, ch), _selectors(B * heads, T, ch, diag=True),
           R.tier2_inputs(kernel, precision, B * heads, T, ch, seed=7 * T + ch))


@pytest.mark.parametrize("precision", ["parity", "f16", "bf16"])
def test_lsa_flash_drop(dev, precision):
    """lsa_flash64_kernel<T, true> / lsa_flash_kernel<T, 3, true> at p = 0.5: 1 / (1 - p) = 2 exactly"""
    from oracle import dropmask
    (B, T, heads, ch), p, seed, site = R.CASES["lsa_drop"][0], 0.5, 0xC0FFEE1234, 25
    P = B * heads
    kernel = "lsa_parity" if precision.startswith("parity") else "lsa64"
    keep = torch.from_numpy(dropmask.keep_attention(P, T, p, seed, site))
    sel = []
    for name, q, k, v, _ in _selectors(P, T, ch, diag=True):
        ex = R.selector_expected(q, k, v, True, keep, 2.0)
        assert bool(((ex == 0).all(-1)).any()) and bool(((ex != 0).any(-1)).any())
        sel.append((name, q, k, v, ex))
    _check(f"{kernel} dropout {precision} B{B} T{T} h{heads}", _run_lsa(dev, B, T, heads, precision, (p, seed, site)),
           lambda q, k, v: R.lsa_ref(q, k, v, keep=keep, p=p), lambda r, q, k, v: R.tier2_bound(kernel, precision, r, q, k, v, T, ch), sel,
           R.tier2_inputs(kernel, precision, P, T, ch, seed=11))


@pytest.mark.parametrize("B,T,heads,ch", R.CASES["lsa_mx8"])
def test_lsa_flash_mx8(dev, B, T, heads, ch):
    """lsa_flash64_mx8_kernel<bf16> behind qkv_pack_mx8 (scale 1): the selectors are exact in e4m3 under any block scale, so the pack
    changes nothing; tier 2 is held against the attention on the operands the planes stand for, with u = 2^-4 for the e4m3 P."""
    from stedm_amd import ops
    pr = _prec("fp8")
    assert pr.attn_fp8
    P, Tp, u8 = B * heads, (T + 127) // 128 * 128, torch.uint8
    deq = {}

    def run(q, k, v):
        qkv = R.lsa_qkv_rows(q, k, v, B, heads).float().to(dev)
        q8 = torch.zeros((P, Tp, 64), dtype=u8, device=dev); k8 = torch.zeros_like(q8); v8 = torch.zeros((P, 64, Tp), dtype=u8, device=dev)
        qs = torch.zeros((P, Tp, 2), dtype=u8, device=dev); ks = torch.zeros_like(qs); vs = torch.zeros((P, Tp // 32, 64), dtype=u8, device=dev)
        out = torch.full((B, T, heads * 64), NANW, dtype=I16, device=dev)
        ops.qkv_pack_mx8(qkv, 1.0, q8, qs, k8, ks, v8, vs, B, T, Tp, heads, pr)
        ops.lsa_flash_mx8(q8, qs, k8, ks, v8, vs, out, B, T, Tp, heads, pr)
        deq["ops"] = R.mx_problem_operands(*(t.cpu() for t in (q8, qs, k8, ks, v8, vs)), T)
        return R.legacy_unpack(out.cpu().view(torch.bfloat16).double(), B, heads)

    sel = []
    q, k, _, _, pi = R.one_hot(P, T, ch, seed=T + ch)
    v = R.mx_one_hot_v(T, ch).expand(P, T, ch).contiguous()
    sel.append(("one_hot", q, k, v, R.selector_expected(q, k, v, True)))
    q2, k2, v2, ex2, _ = R.group(P, T, ch, seed=T + ch, diag=True)
    sel.append(("group", q2, k2, v2, ex2))
    q3, k3, _, _, _ = R.late(P, T, ch, seed=T + ch, diag=True)
    sel.append(("late", q3, k3, v, R.selector_expected(q3, k3, v, True)))
    q4, k4, _, _, _ = R.below_zero(P, T, ch, seed=T + ch, diag=True)
    sel.append(("below_zero", q4, k4, v, R.selector_expected(q4, k4, v, True)))
    for name, a, b, c, ex in sel:
        got = _twice(lambda: run(a, b, c))
        assert all(torch.equal(x, y) for x, y in zip(deq["ops"], (a, b, c))), "the MX planes do not hold the selectors exactly"
        bad = (got != ex).any(-1).nonzero()
        assert bad.numel() == 0, f"lsa_mx8 {name}: {bad.shape[0]} wrong rows, first (problem, query) {bad[0].tolist()}"
    q, k, v = R.random_qkv(P, T, ch, None, seed=7 * T + ch, logit_std=1.5, base2=True)
    got = _twice(lambda: run(q, k, v))
    r = R.lsa_ref(*deq["ops"])
    R.assert_spread(r)
    ratio = float(((got - r["out"]).abs() / R.bound(r, T, ch, torch.float8_e4m3fn, out_dtype=torch.bfloat16)).max())
    print(f"[lsa_flash64_mx8 B{B} T{T} h{heads}] tier 1 exact; tier 2 worst err / bound {ratio:.3f} (u = 2^-4)")
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------ Swin-V2 window attention
SWIN_FORMS = [("parity", False), ("parity_bf16", False), ("f16", False), ("bf16", False), ("f16", True), ("bf16", True)]


@pytest.mark.parametrize("precision,in16", SWIN_FORMS, ids=[f"{p}{'-in16' if i else ''}" for p, i in SWIN_FORMS])
@pytest.mark.parametrize("H,W,shift", R.SWIN_CASES)
def test_swin_window_attn(dev, H, W, shift, precision, in16):
    """swin_window_attn_kernel<T, npass, in16>: all six instantiations, picked by Precision (npass, dtype) and the dtype of qkv"""
    from stedm_amd import ops
    pr, dt = _prec(precision), R.DTYPES[precision]
    N, heads = R.SWIN_N, R.SWIN_HEADS
    C, rows, lo = heads * 32, N * H * W, pr.npass == 3
    assert not (in16 and lo)
    uT = R.u_of(dt)[0]

    def run(qkv, bias, scale, rpb):
        src = qkv.to(dt).view(I16).to(dev) if in16 else qkv.to(dev)
        assert not in16 or torch.equal(qkv.to(dt).float(), qkv)
        hi = torch.full((rows, C), NANW, dtype=I16, device=dev)
        l_ = torch.full((rows, C), NANW, dtype=I16, device=dev) if lo else None
        ops.swin_window_attn(src, bias.to(dev), scale.float().to(dev), rpb.float().contiguous().to(dev), hi, l_, N, H, W, heads, shift, pr)
        out = hi.cpu().view(dt).double() + (l_.cpu().view(dt).double() if lo else 0)
        return out.view(N, H * W, heads, 32)

    scale = torch.tensor([2.0, 4.0, 6.0], dtype=torch.float64)
    # tier 1: uniform
    qkv, bias, ops_, pad = R.swin_uniform(N, H, W, heads)
    rpb0 = torch.zeros(heads, 64, 64, dtype=torch.float64)
    want = R.swin_attention(*ops_, pad, scale, rpb0, H, W, shift)["out"]
    got = _twice(lambda: run(qkv, bias, scale, rpb0))
    d = (got - want).abs()
    bad = (d > 2 * uT).any(-1).nonzero()
    assert bad.numel() == 0, f"uniform: {bad.shape[0]} wrong (sample, token, head), first {bad[0].tolist()} = (y, x) {divmod(int(bad[0][1]), W)}, max {float(d.max()):.4f}"
    # tier 2
    qkv, bias, ops2, pad2 = R.swin_operands(N, H, W, heads, dt, pr.npass, seed=H * 100 + W, in16=in16)
    rpb = torch.rand(heads, 64, 64, generator=torch.Generator().manual_seed(H + W)).double() * 2.0
    r = R.swin_attention(*ops2, pad2, scale, rpb, H, W, shift)
    assert r["spread"] < 20.0, r["spread"]
    got = _twice(lambda: run(qkv, bias, scale, rpb))
    ratio = float(((got - r["out"]).abs() / R.swin_bound(r, dt, pr.npass)).max())
    print(f"[swin_window_attn {precision}{' int16 qkv' if in16 else ''} H{H} W{W} shift{shift}] tier 1 max {float(d.max()) / uT:.2f} u_T; tier 2 worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
