"""CPU tier of the attention reference tests (no GPU): pins tests/refs_attn.py and proves that the two tiers of
tests/test_gpu_attn_exact.py reject wrong kernels.

  * every reference against its oracle on unrounded random inputs (oracle.unet.qkv_attention_legacy, the attention core of
    oracle.style.lsa with and without a drop mask, oracle.swin.window_attention with an identity proj);
  * the generators' obligations (exact logits, >= 160 nats between the matching key and every other one, exact expected values, the
    asserted logit spread) for every shape of the GPU file;
  * an fp32 emulation of each kernel's arithmetic (refs_attn.emulate: fp32 products and sums, the kernel's rounding points, tile-by-tile
    online softmax or the rounded-reference rule) stays inside tier 1 (bit-exact) and tier 2 (err / bound <= 1) on every GPU case;
  * the same emulation with one defect at a time is rejected.

Worst err / bound of the honest emulation over the GPU cases (tier 2; the one-product bounds are the two 16-bit roundings and little else):
  attn_legacy fp32 0.022 | attn64 f16 0.380, bf16 0.488 | attn_flash f16 0.502, bf16 0.596 | lsa_flash<3> parity 0.014, parity_bf16 0.034
  lsa_flash64 f16 0.460, bf16 0.449 | lsa_flash64<drop> f16 0.498, bf16 0.497 | lsa_flash<3, drop> parity 0.009
  lsa_flash64_mx8 (e4m3 P, u = 2^-4, operands = what refs_attn.mx_quantise makes of the inputs) 0.344
  swin one product f16 0.471, bf16 0.602 (fp32 rows and int16 qkv rows), three products f16 0.006, bf16 0.027

Defects (refs_attn.MUTANTS and the two Swin ones). Tier 1: the pattern that rejects it - asserted for every kernel the defect applies to,
lsa_flash64_mx8 included. Tier 2: worst err / bound over the cases, the smallest over the kernels of a type, f16 / bf16 / e4m3 (e4m3 is
lsa_flash64_mx8 alone); asserted > 1 in f16 (and fp32, parity) for the first five rows, reported otherwise:
  defect             tier 1                              tier 2 f16 / bf16 / e4m3   note
  drop_last          one_hot (the query of key T - 1)    430 / 60 / 4.2             the last valid key is masked
  double_key         group (a member counted twice)      410 / 55 / 4.7             in l and in O
  swap_v             one_hot                             1100 / 160 / 21            two keys of one tile swapped in the V order only
  no_diag            group (own group of 2)              830 / 115 / 6.9
  mask_off_by_one    group in attn_flash (its pad row    9.2 / 1.5 / 0.34           LSA's, the MX planes' and the fp32 kernel's pad rows are zero
                     re-reads key T - 1, which is in a                              (logit 0, v 0): one_hot / group cannot see them; below_zero
                     group); below_zero everywhere else                             makes every real logit negative, so a visible pad key takes
                                                                                    the row. In e4m3 tier 2 does NOT separate it (0.34 = the
                                                                                    honest figure): tier 1 is the only guard there
  skip_rescale       one_hot, late                       0.45 / 0.45 / 1.3          with a first-tile reference random logits seldom move it:
                                                                                    tier 1 is the guard (online forms 7000+)
  first_rescale      late                                0.46 / 0.45 / 0.34         the still-empty sums rescaled by exp2(-first reference): 0 inf
                                                                                    = NaN when the first tile is far down; tier 1 is the guard
  swin roll shift-1  uniform                             5600 / 580                 (three products 30000 / 5300)
  swin mask visible  uniform                             5700 / 700                 (three products 24000 / 5600)
So in e4m3 tier 2 still separates the key-set defects (4 .. 21 times the bound) but with little room, and not the off-by-one mask.
The measured ratios are printed by the tests (-s) and asserted where the table says so.
"""
import math

import pytest
import torch

from tests import refs_attn as R

torch.set_grad_enabled(False)

KP = [("attn_legacy", "fp32"), ("attn64", "f16"), ("attn64", "bf16"), ("attn_flash", "f16"), ("attn_flash", "bf16"),
      ("lsa_parity", "parity"), ("lsa_parity", "parity_bf16"), ("lsa64", "f16"), ("lsa64", "bf16"), ("lsa_mx8", "fp8")]
DIAG = ("lsa_parity", "lsa64", "lsa_mx8")


def _sel_cases(kernel, P, T, ch):
    """the selector cases (name, q, k, v, expected) of a kernel's shape; MX-fp8: v exact in e4m3, and the pack must change nothing"""
    diag = kernel in DIAG
    q, k, v, ex, _ = R.one_hot(P, T, ch, seed=T + ch)
    if kernel == "lsa_mx8":
        v = R.mx_one_hot_v(T, ch).expand(P, T, ch).contiguous()
        ex = R.selector_expected(q, k, v, diag)
    out = [("one_hot", q, k, v, ex)]
    q2, k2, v2, ex2, _ = R.group(P, T, ch, seed=T + ch, diag=diag)
    out.append(("group", q2, k2, v2, ex2))
    if T > 64:
        q3, k3, v3, ex3, _ = R.late(P, T, ch, seed=T + ch, diag=diag)
        if kernel == "lsa_mx8":
            v3, ex3 = v, R.selector_expected(q3, k3, v, diag)
        out.append(("late", q3, k3, v3, ex3))
    if ch >= 32:
        q4, k4, v4, ex4, _ = R.below_zero(P, T, ch, seed=T + ch, diag=diag)
        R.check_selector(q4, k4, math.log(2.0) if diag else 1.0 / math.sqrt(ch), diag)
        if kernel == "lsa_mx8":
            v4, ex4 = v, R.selector_expected(q4, k4, v, diag)
        out.append(("below_zero", q4, k4, v4, ex4))
    if kernel == "lsa_mx8":
        for _, a, b, c, _ in out:
            assert all(torch.equal(x, y) for x, y in zip(R.mx_quantise(a, b, c), (a, b, c)))
    return out


def _emu(kernel, prec, q, k, v, **kw):
    ek, _, _ = R.spec(kernel, prec, q.shape[-1])
    if kernel == "attn64":
        ek = dict(ek, tile=64)
    return R.emulate(q, k, v, **ek, **kw)


def _ratio(kernel, prec, got, q, k, v, keep=None, p=0.0):
    _, _, ref = R.spec(kernel, prec, q.shape[-1])
    r = ref(q, k, v) if keep is None else ref(q, k, v, keep=keep, p=p)
    R.assert_spread(r)
    b = R.tier2_bound(kernel, prec, r, q, k, v, q.shape[1], q.shape[2])
    return float(((got - r["out"]).abs() / b).max())


# ------------------------------------------------------------------------------------------------ references against the oracles
def test_legacy_reference_vs_oracle():
    from oracle.unet import qkv_attention_legacy
    g = torch.Generator().manual_seed(3)
    for B, T, heads, ch in [(2, 36, 2, 16), (1, 100, 3, 64)]:
        q, k, v = (torch.randn(B * heads, T, ch, generator=g, dtype=torch.float64) for _ in range(3))
        qkv = R.legacy_pack(q, k, v, B, heads)                                   # [B][T][heads 3 ch]
        want = qkv_attention_legacy(qkv.transpose(1, 2).contiguous(), heads)     # [B][heads ch][T]
        got = R.legacy_ref(q, k, v)["out"]
        assert float((R.legacy_unpack(want.transpose(1, 2), B, heads) - got).abs().max()) < 2e-6      # the oracle's softmax is fp32


@pytest.mark.parametrize("drop", [False, True])
def test_lsa_reference_vs_oracle(drop):
    from oracle import dropmask, style
    g = torch.Generator().manual_seed(4)
    B, T, heads = 2, 70, 3
    inner = heads * 64
    x = torch.randn(B, T, 3 * inner, generator=g, dtype=torch.float64)
    tau = math.exp(math.log(64 ** -0.5) + 0.1)
    P = {"a.to_qkv.weight": torch.eye(3 * inner, dtype=torch.float64), "a.temperature": torch.tensor(math.log(tau), dtype=torch.float64),
         "a.to_out.0.weight": torch.eye(inner, dtype=torch.float64), "a.to_out.0.bias": torch.zeros(inner, dtype=torch.float64)}
    p, seed, layer = 0.25, 0xABCDEF12345, 2
    want = style.lsa(P, "a.", x, heads, (p, seed, layer) if drop else None)
    q, k, v = (t.reshape(B, T, heads, 64).permute(0, 2, 1, 3).reshape(B * heads, T, 64) for t in x.chunk(3, dim=-1))
    keep = None
    if drop:
        keep = torch.from_numpy(dropmask.keep_attention(B * heads, T, p, seed, 8 * layer + style.SITE_ATTN))
    got = R.lsa_ref(q * (tau * R.LOG2E), k, v, keep=keep, p=p)["out"].reshape(B, heads, T, 64).permute(0, 2, 1, 3).reshape(B, T, inner)
    if drop:                                      # the oracle also drops elements after to_out: compare what it kept
        kept = want != 0
        assert float(kept.double().mean()) > 0.6
        want, got = want * (1.0 - p), torch.where(kept, got, torch.zeros_like(got))
    assert float((want - got).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("kernel", sorted(R.CASES))
def test_generator_conditions(kernel):
    diag = kernel in ("lsa_parity", "lsa64", "lsa_drop", "lsa_mx8")
    for B, T, heads, ch in R.CASES[kernel]:
        P = B * heads
        sn = math.log(2.0) if diag else 1.0 / math.sqrt(ch)
        q, k, v, ex, pi = R.one_hot(P, T, ch, seed=T + ch)
        gap = R.check_selector(q, k, sn, diag)
        assert bool((pi != torch.arange(T)).all()) and bool((v.to(torch.bfloat16).double() == v).all())
        nt = (T + 63) // 64
        if nt > 1:                                # targets before, inside and after the query's own tile, and in the last tile
            qt, tt = torch.arange(T)[None, :] // 64, pi // 64
            assert bool((tt < qt).any()) and bool((tt == qt).any()) and bool((tt > qt).any()) and bool((tt == nt - 1).any())
        if T > 64:
            ql, kl, _, _, first = R.late(P, T, ch, seed=T + ch, diag=diag)
            gap3 = R.check_selector(ql, kl, sn, diag)
            assert first * sn * R.LOG2E <= -150.0, (first, gap3)          # exp2(-first) overflows fp32: the reference of the first tile is far below
        assert bool((v[0][:, None, :] != v[0][None, :, :]).all(-1)[~torch.eye(T, dtype=torch.bool)].all())      # any two keys differ in every channel
        q, k, v, ex, groups = R.group(P, T, ch, seed=T + ch, diag=diag)
        gap2 = R.check_selector(q, k, sn, diag)
        assert any(T - 1 in grp for grp in groups) and {len(grp) for grp in groups} == {2, 4}
        assert bool((ex.to(torch.bfloat16).double() == ex).all())
        if nt >= 4:
            assert any(len({s // 64 for s in grp}) == len(grp) for grp in groups if len(grp) == 4)
        print(f"[{kernel} T{T} ch{ch}] gaps {gap:.0f} / {gap2:.0f} nats, groups {groups}")


# ------------------------------------------------------------------------------------------------ honest emulation: inside both tiers
@pytest.mark.parametrize("kernel,prec", KP)
def test_honest_emulation_is_inside_both_tiers(kernel, prec):
    worst = 0.0
    diag = kernel in DIAG
    for B, T, heads, ch in R.CASES[kernel]:
        P = B * heads
        for name, q, k, v, ex in _sel_cases(kernel, P, T, ch):
            assert torch.equal(_emu(kernel, prec, q, k, v), ex), name
        q, k, v = R.tier2_inputs(kernel, prec, P, T, ch, seed=7 * T + ch)
        worst = max(worst, _ratio(kernel, prec, _emu(kernel, prec, q, k, v), q, k, v))
    print(f"[emulation {kernel} {prec}] worst err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("kernel,prec", [("lsa64", "f16"), ("lsa64", "bf16"), ("lsa_parity", "parity")])
def test_honest_dropout_emulation_is_inside_both_tiers(kernel, prec):
    from oracle import dropmask
    (B, T, heads, ch), p = R.CASES["lsa_drop"][0], 0.5
    P = B * heads
    keep = torch.from_numpy(dropmask.keep_attention(P, T, p, 0xC0FFEE1234, 25))
    q, k, v, ex, pi = R.one_hot(P, T, ch, seed=T + ch)
    want = torch.where(torch.gather(keep, 2, pi[:, :, None]), 2 * ex, torch.zeros_like(ex))
    assert torch.equal(_emu(kernel, prec, q, k, v, keep=keep, inv_keep=2.0), want)
    assert 0.3 < float((want != 0).any(-1).double().mean()) < 0.7
    q, k, v = R.tier2_inputs(kernel, prec, P, T, ch, seed=11)
    ratio = _ratio(kernel, prec, _emu(kernel, prec, q, k, v, keep=keep, inv_keep=2.0), q, k, v, keep=keep, p=p)
    print(f"[emulation {kernel} {prec} dropout] err / bound {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ defects must fail
def _mutant_report(mutant, kernel, prec):
    """(tier 1 rejected on some pattern, worst tier-2 ratio) of a defect over the kernel's cases where it can occur"""
    diag = kernel in DIAG
    t1, t2, ran = False, 0.0, False
    for B, T, heads, ch in R.CASES[kernel]:
        P, nt = B * heads, (T + 63) // 64
        if mutant == "mask_off_by_one" and T % 64 == 0:
            continue
        if mutant == "skip_rescale" and nt == 1:
            continue
        ran = True
        groups = R.group_layout(T)
        mk = {"double_key": groups[1][0], "swap_v": (5, 9)}.get(mutant)
        for _, q, k, v, ex in _sel_cases(kernel, P, T, ch):
            t1 |= not torch.equal(_emu(kernel, prec, q, k, v, mutant=mutant, mkey=mk), ex)
        q, k, v = R.tier2_inputs(kernel, prec, P, T, ch, seed=7 * T + ch)
        t2 = max(t2, _ratio(kernel, prec, _emu(kernel, prec, q, k, v, mutant=mutant, mkey=mk), q, k, v))
    return ran, t1, t2


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_defects_are_rejected(mutant):
    seen1 = False
    for kernel, prec in KP:
        if mutant == "no_diag" and kernel not in DIAG:
            continue
        if mutant == "first_rescale" and kernel not in ("attn_flash", "lsa64", "lsa_mx8"):      # only the kernels with a first-tile reference have one
            continue
        ran, t1, t2 = _mutant_report(mutant, kernel, prec)
        if not ran:
            continue
        print(f"[defect {mutant:16s} {kernel:11s} {prec:11s}] tier 1 {'REJECTS' if t1 else 'passes '}  tier 2 err / bound {t2:10.2f}")
        seen1 |= t1
        if mutant != "skip_rescale" or kernel != "attn64":
            assert t1, (mutant, kernel, prec)
        if mutant in ("drop_last", "double_key", "mask_off_by_one", "swap_v", "no_diag") and prec in ("f16", "fp32", "parity"):
            assert t2 > 1.0, (mutant, kernel, prec, t2)
    assert seen1


# ------------------------------------------------------------------------------------------------ Swin cosine window attention
SWIN_MODES = [("f16", 1), ("bf16", 1), ("f16", 3), ("bf16", 3)]


@pytest.mark.parametrize("H,W,shift", R.SWIN_CASES + [(16, 24, 4)])
def test_swin_reference_vs_oracle(H, W, shift):
    from oracle import swin as osw
    g = torch.Generator().manual_seed(8)
    N, heads = 2, 3
    C = heads * 32
    d = torch.float64
    p = {"a.qkv.weight": torch.randn(3 * C, C, generator=g, dtype=d) / math.sqrt(C), "a.qkv.bias": torch.randn(3 * C, generator=g, dtype=d) * 0.5,
         "a.logit_scale": torch.tensor([1.0, 2.5, 5.0], dtype=d).view(heads, 1, 1), "a.cpb_mlp.0.weight": torch.randn(64, 2, generator=g, dtype=d),
         "a.cpb_mlp.0.bias": torch.randn(64, generator=g, dtype=d), "a.cpb_mlp.2.weight": torch.randn(heads, 64, generator=g, dtype=d),
         "a.proj.weight": torch.eye(C, dtype=d), "a.proj.bias": torch.zeros(C, dtype=d)}
    x = torch.randn(N, H, W, C, generator=g, dtype=d)
    want = osw.window_attention(x, p, "a.", heads, shift)
    bias = p["a.qkv.bias"].clone()
    bias[C:2 * C] = 0
    qkv = (x.reshape(-1, C) @ p["a.qkv.weight"].t() + bias).view(N, H * W, 3, heads, 32)
    b3 = bias.view(3, heads, 32)
    pad = (R.swin_normalize(b3[0]), torch.zeros(heads, 32, dtype=d), b3[2])
    scale = torch.clamp(p["a.logit_scale"], max=math.log(100.0)).exp().view(heads)
    assert float(scale.max()) == pytest.approx(100.0)
    r = R.swin_attention(R.swin_normalize(qkv[:, :, 0]), R.swin_normalize(qkv[:, :, 1]), qkv[:, :, 2], pad, scale,
                         osw.position_bias(p, "a.", heads), H, W, shift)
    assert float((r["out"].reshape(N, H, W, C) - want).abs().max()) < 1e-12


def _swin_case(H, W, shift, dtype, npass, in16=False):
    N, heads = R.SWIN_N, R.SWIN_HEADS
    qkv, bias, ops_, pad = R.swin_operands(N, H, W, heads, dtype, npass, seed=H * 100 + W, in16=in16)
    g = torch.Generator().manual_seed(H + W)
    scale = torch.tensor([2.0, 4.0, 6.0], dtype=torch.float64)
    rpb = torch.rand(heads, 64, 64, generator=g).double().float().double() * 2.0
    return qkv, bias, ops_, pad, scale, rpb


@pytest.mark.parametrize("prec,npass", SWIN_MODES)
def test_swin_honest_emulation_and_defects(prec, npass):
    dtype = R.DTYPES[prec]
    uT = R.u_of(dtype)[0]
    worst, seen = 0.0, {"roll": False, "visible": False}
    t2 = {"roll": 0.0, "visible": 0.0}
    for H, W, shift in R.SWIN_CASES:
        N, heads = R.SWIN_N, R.SWIN_HEADS
        # tier 1: uniform
        _, _, ops_, pad = R.swin_uniform(N, H, W, heads)
        scale, rpb0 = torch.tensor([2.0, 4.0, 6.0], dtype=torch.float64), torch.zeros(heads, 64, 64, dtype=torch.float64)
        want = R.swin_attention(*ops_, pad, scale, rpb0, H, W, shift)["out"]
        got = R.swin_attention(*ops_, pad, scale, rpb0, H, W, shift, emu=(dtype, npass))
        assert float((got - want).abs().max()) <= 2 * uT
        # tier 2: random
        _, _, ops2, pad2, scale, rpb = _swin_case(H, W, shift, dtype, npass)
        r = R.swin_attention(*ops2, pad2, scale, rpb, H, W, shift)
        assert r["spread"] < 20.0, r["spread"]
        b = R.swin_bound(r, dtype, npass)
        got2 = R.swin_attention(*ops2, pad2, scale, rpb, H, W, shift, emu=(dtype, npass))
        worst = max(worst, float(((got2 - r["out"]).abs() / b).max()))
        if npass == 1:                                # the int16 qkv form: rows already rounded to the type, then normalised and rounded again
            qkv16, _, ops3, pad3, _, _ = _swin_case(H, W, shift, dtype, npass, in16=True)
            assert torch.equal(qkv16.to(dtype).float(), qkv16)
            r3 = R.swin_attention(*ops3, pad3, scale, rpb, H, W, shift)
            got3 = R.swin_attention(*ops3, pad3, scale, rpb, H, W, shift, emu=(dtype, npass))
            worst = max(worst, float(((got3 - r3["out"]).abs() / R.swin_bound(r3, dtype, npass)).max()))
        masked = R.swin_index(H, W, shift)[2]
        if not masked:
            continue
        for name, kw in (("roll", dict(roll_delta=1)), ("visible", dict(visible=True))):
            bad = R.swin_attention(*ops_, pad, scale, rpb0, H, W, shift, emu=(dtype, npass), **kw)
            d1 = float((bad - want).abs().max())
            seen[name] |= d1 > 2 * uT
            assert d1 >= 1.0 / 64 - 2 * uT
            bad2 = R.swin_attention(*ops2, pad2, scale, rpb, H, W, shift, emu=(dtype, npass), **kw)
            t2[name] = max(t2[name], float(((bad2 - r["out"]).abs() / b).max()))
    print(f"[swin emulation {prec} x{npass}] worst err / bound {worst:.3f}; defects: roll by shift - 1 tier 2 {t2['roll']:.1f}, "
          f"region mask all-visible tier 2 {t2['visible']:.1f}")
    assert worst <= 1.0 and seen["roll"] and seen["visible"]
    assert t2["roll"] > 1.0 and t2["visible"] > 1.0
