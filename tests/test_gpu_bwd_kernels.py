"""GPU tier (-m gpu): the helper kernels of the training step (stedm_amd/csrc/bwd.hip with silu_bwd.hpp, and sum_planes of wgrad.hip), each called through
its `ops` wrapper and held against the plain references of tests/refs_bwd.py at the shapes where such kernels go wrong: tails, partial
tiles, odd leading dimensions, unaligned views, more than one trip of a grid-stride loop, accumulate on and off.

  exact kernels (data movement, casts, one or two roundings in a fixed order): torch.equal
  fixed-order sums on dyadic inputs (tests.refs_bwd.dyadic): torch.equal against the fp64 sum, one lost or doubled term changes a bit
  rounded kernels (silu, geglu_bwd, ln_bwd): per-element bounds derived in tests/refs_bwd.py from the operation counts, none of them taken
  from a run of the kernel; tests/test_bwd_refs_cpu.py holds the same bounds against fp32 torch. Each test prints its worst error / bound.

Every output and workspace buffer is filled with NaN (a NaN bit pattern for the 16-bit planes) before the call: an element nobody wrote,
or a pad element somebody read, shows up. q_sample allocates its own output, so there the comparison alone speaks."""
import pytest
import torch

from tests import refs_bwd as R

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
NAN16 = 0x7FC0              # bf16 quiet NaN as an int16 word
GUARD = 1234.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def nanfull(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def guarded(n, dev, fill=NAN, guard=64):
    """flat fp32 buffer of n elements followed by `guard` guard words; returns (whole buffer, view of the first n)"""
    buf = torch.full((n + guard,), GUARD, dtype=torch.float32, device=dev)
    buf[:n] = fill
    return buf, buf[:n]


def guard_ok(buf, n):
    return bool((buf[n:] == GUARD).all())


def worst(err, bound):
    return float((err / bound).max())


# ================================================================================================ exact kernels
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_im2col_t16_exact(dev, ks, mode):
    from stedm_amd import ops
    n = 0
    for B in (1, 3):
        for H, W in ((8, 8), (5, 7), (6, 10)):
            if (H, W) == (5, 7) and mode != 0:        # odd sizes: stride 1 only
                continue
            for C in (8, 72, 128):
                src = R.finite_bf16_bits((B, H, W, C), 100 * B + 10 * H + C)
                Ho, Wo = (2 * H, 2 * W) if mode == 1 else ((H // 2, W // 2) if mode == 2 else (H, W))
                P = B * Ho * Wo
                for extra in (0, 64):
                    Ppad = (P + 63) // 64 * 64 + extra
                    dst = torch.full((ks * ks * C, Ppad), NAN16, dtype=torch.int16, device=dev)
                    ops.im2col_t16(src.to(dev), dst, ks, mode)
                    got = dst.cpu()
                    ref = R.im2col_t(src, ks, mode, Ppad)
                    assert bool((got[:, P:] == 0).all()), f"pad columns B={B} {H}x{W} C={C} Ppad={Ppad}"
                    assert torch.equal(got, ref), f"B={B} {H}x{W} C={C} Ppad={Ppad}"
                    n += 1
    assert n == (36 if mode == 0 else 24)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("with_lo", [True, False])
def test_zero_insert16_exact(dev, dt, with_lo):
    from stedm_amd import ops
    from stedm_amd._lib import BF16, F16
    prec = ops.Precision(F16 if dt == torch.float16 else BF16, 1)
    # ties of both formats (f16 spacing at 1 is 2^-10, bf16 2^-7), the f16 overflow threshold 65520 and values far above the f16 range
    special = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -11), 65519.0, 65520.0, 70000.0, -70000.0,
                            1e6, 3.0e38, 1e-8, 3e-8, 0.0, 2049.0, 2051.0, 257.0, 259.0], dtype=torch.float32)
    for C in (4, 36):
        for B, Ho, Wo in ((1, 1, 1), (2, 3, 5), (1, 7, 3)):
            x = R.normal((B, Ho, Wo, C), 31, "zi.x", std=3.0)
            flat = x.view(-1)
            k = min(flat.numel(), special.numel())
            flat[:k] = special[:k]
            hi = nanfull((B, 2 * Ho, 2 * Wo, C), dev, dt)
            lo = nanfull((B, 2 * Ho, 2 * Wo, C), dev, dt) if with_lo else None
            ops.zero_insert16(x.to(dev), hi, lo, prec)
            rh, rl = R.split16(R.zero_insert(x), dt)
            assert torch.equal(hi.cpu(), rh), (C, B, Ho, Wo)
            if with_lo:
                assert torch.equal(lo.cpu(), rl), (C, B, Ho, Wo)


@pytest.mark.parametrize("gen", ["dyadic", "normal"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_sum2x2_exact(dev, gen, accumulate):
    from stedm_amd import ops
    for C in (4, 36, 128):
        for B, H, W in ((1, 1, 1), (3, 5, 7), (64, 8, 8)):
            if gen == "dyadic":
                x, prior = R.dyadic((B, 2 * H, 2 * W, C), 41), R.dyadic((B, H, W, C), 42)
            else:
                x, prior = R.normal((B, 2 * H, 2 * W, C), 41, "s2.x"), R.normal((B, H, W, C), 41, "s2.prior")
            out = prior.to(dev) if accumulate else nanfull((B, H, W, C), dev)
            ops.sum2x2(x.to(dev), out, accumulate)
            ref = R.sum2x2(x, prior if accumulate else None)           # fp32, the kernel's order
            assert torch.equal(out.cpu(), ref), (C, B, H, W)
            if gen == "dyadic":
                assert torch.equal(ref.double(), R.sum2x2(x.double(), prior.double() if accumulate else None))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape", [(1,), (255,), (4, 32, 32)])
def test_q_sample_exact(dev, B, shape):
    from stedm_amd import ops
    T = 1000
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=torch.float64) ** 2
    ac = torch.cumprod(1.0 - betas, 0)
    sa, s1 = ac.sqrt().float(), (1.0 - ac).sqrt().float()
    x0, nz = R.normal((B,) + shape, 51, "qs.x0"), R.normal((B,) + shape, 51, "qs.noise")
    for t in ([[0], [T - 1]] if B == 1 else [[0, T - 1, 1, 500, T - 1], [T - 1, 0, 0, 999, 37]]):
        t = torch.tensor(t, dtype=torch.int64)
        got = ops.q_sample(x0.to(dev), nz.to(dev), t.to(dev), sa.to(dev), s1.to(dev))
        assert torch.equal(got.cpu(), R.q_sample(x0, nz, t, sa, s1)), t


@pytest.mark.parametrize("n", R.L1_NS)
def test_l1_loss_exact(dev, n):
    """dyadic pred / target: |pred - target| is exact in fp32, the fp64 sum is exact, so loss == float32(sum / n); d_pred is a sign times one
    fp32 constant. n = 1024 * 4096 + 3 takes the grid-stride loop round a second time; many elements have pred == target."""
    from stedm_amd import ops
    p, q = R.l1_inputs(n)
    assert int((p == q).sum()) > 0 or n == 1
    pd, qd = p.to(dev), q.to(dev)
    for gs in (1.0, 0.25, 3.0):
        ref_loss, ref_d = R.l1(p, q, gs)
        d = nanfull((n,), dev)
        loss, ws = nanfull((1,), dev), nanfull((1024,), dev, torch.float64)
        ops.l1_loss(pd, qd, d, ws, loss, gs)
        assert float(loss) == float(ref_loss), (gs, float(loss), float(ref_loss))
        assert torch.equal(d.cpu(), ref_d)
        assert bool((d[pd == qd] == 0).all())
    loss, ws = nanfull((1,), dev), nanfull((1024,), dev, torch.float64)
    ops.l1_loss(pd, qd, None, ws, loss)
    assert float(loss) == float(R.l1(p, q, 1.0)[0])
    loss = nanfull((1,), dev)
    ops.l1_loss(pd, pd.clone(), None, ws, loss)                  # pred == target everywhere
    assert float(loss) == 0.0


# ================================================================================================ exact sums on dyadic inputs
@pytest.mark.parametrize("B", [1, 15, 16, 17, 48, 49, 64, 65, 130])
def test_chan_sum_fold_exact(dev, B):
    """B >= 49 enters the four-samples-per-lane loop, B = 65 and 130 leave it with a tail; cs[..., 1] is NaN and must not be read; the pad
    columns C..ld of per_sample must stay as they were"""
    from stedm_amd import ops
    for nslab in (1, 3):
        for C in (4, 16, 40):
            cs = torch.full((B, nslab, C, 2), NAN)
            cs[..., 0] = R.dyadic((B, nslab, C), 1000 * B + 10 * C + nslab)
            ref_per, ref_tot = R.chan_sum_fold(cs.double())
            prior = R.dyadic((C,), 61)
            csd, ld = cs.to(dev), C + 3
            for want_per, want_tot, want_tot2, acc in ((1, 1, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1), (0, 1, 1, 0), (1, 0, 0, 0)):
                per = nanfull((B, ld), dev) if want_per else None
                tot = (prior.to(dev) if acc else nanfull((C,), dev)) if want_tot else None
                tot2 = nanfull((C,), dev) if want_tot2 else None
                ops.chan_sum_fold(csd, per, ld, tot, bool(acc), tot2)
                tag = (B, nslab, C, want_per, want_tot, want_tot2, acc)
                if want_per:
                    assert torch.equal(per[:, :C].cpu(), ref_per.float()), tag
                    assert bool(torch.isnan(per[:, C:]).all()), tag
                if want_tot:
                    rt = (ref_tot + (prior.double() if acc else 0.0)).float()
                    assert torch.equal(tot.cpu(), rt), tag
                    if want_tot2:
                        assert torch.equal(tot2.cpu(), rt), tag


def _wgrad_case(dev, cout, cin, taps, cout_ld, cin_ld, nsplit, acc, unaligned=False, seed=0):
    from stedm_amd import ops
    dw = torch.full((nsplit, taps, cin_ld, cout_ld), NAN)                      # the padding of both leading dimensions is NaN: never read
    dw[:, :, :cin, :cout] = R.dyadic((nsplit, taps, cin, cout), 7000 + seed)
    n = cout * cin * taps
    prior = R.dyadic((n,), 71)
    buf, grad = guarded(n, dev)
    if acc:
        grad.copy_(prior)
    if unaligned:                                                              # a view that starts 4 bytes into its allocation
        base = torch.empty((dw.numel() + 1,), dtype=torch.float32, device=dev)
        dwd = base[1:]
        dwd.copy_(dw.view(-1))
        assert dwd.data_ptr() % 16 == 4
    else:
        dwd = dw.to(dev)
    ops.wgrad_to_oihw(dwd, grad.view(cout, cin, taps), cin_ld, cout_ld, bool(acc), nsplit)
    ref = R.wgrad_to_oihw(torch.nan_to_num(dw, nan=0.0).double(), cout, cin).view(-1) + (prior.double() if acc else 0.0)
    tag = (cout, cin, taps, cout_ld, cin_ld, nsplit, acc, unaligned)
    assert torch.equal(grad.cpu(), ref.float()), tag
    assert guard_ok(buf, n), tag


# wgrad_to_oihw_kernel<4> runs when ceil(cout / 32) * ceil(cin / 16) < 128 and nsplit >= 4: every pair below except (512, 512) (16 x 32 = 512
# blocks) with nsplit 4 or 32; nsplit 1 or 3, and (512, 512) at every nsplit, run wgrad_to_oihw_kernel<16>. Inside either form the 16-byte
# loads need cout_ld % 4 == 0, a full block of 32 couts and an aligned dw: (32, 16), (96, 3), (128, 128) and the first block of (48, 20) at
# cout_ld == cout; the scalar loop takes cout_ld == cout + 2, the last block of (48, 20), all of (4, 7), and the unaligned view.
@pytest.mark.parametrize("cout,cin", [(32, 16), (48, 20), (128, 128), (96, 3), (4, 7)])
@pytest.mark.parametrize("taps", [1, 9])
def test_wgrad_to_oihw_exact(dev, cout, cin, taps):
    i = 0
    for cout_ld in (cout, cout + 2):
        for nsplit in (1, 3, 4, 32):
            for acc in (0, 1):
                _wgrad_case(dev, cout, cin, taps, cout_ld, cin + 5, nsplit, acc, seed=i)
                i += 1
    for nsplit in (1, 4):
        _wgrad_case(dev, cout, cin, taps, cout, cin + 4, nsplit, 0, unaligned=True, seed=i)


@pytest.mark.parametrize("taps,cout_ld,nsplit,acc", [(9, 512, 3, 0), (9, 514, 1, 1), (1, 512, 32, 1), (1, 514, 4, 0), (1, 512, 4, 0)])
def test_wgrad_to_oihw_exact_512(dev, taps, cout_ld, nsplit, acc):
    _wgrad_case(dev, 512, 512, taps, cout_ld, 512 + 4, nsplit, acc, seed=taps + nsplit)


@pytest.mark.parametrize("cout,cin", [(32, 16), (48, 20), (128, 128), (96, 3), (4, 7), (512, 512)])
def test_sum_planes_exact(dev, cout, cin):
    from stedm_amd import ops
    for taps, nsplit in (((9, 1), (1, 5)) if cout == 512 else ((1, 1), (1, 5), (9, 1), (9, 5))):
        n = cout * cin * taps
        part = R.dyadic((nsplit, n), 81 + taps + nsplit)
        prior = R.dyadic((n,), 82)
        for acc in (0, 1):
            buf, out = guarded(n, dev)
            if acc:
                out.copy_(prior)
            ops.sum_planes(part.to(dev), out, nsplit, bool(acc))
            ref = R.sum_planes(part.double()) + (prior.double() if acc else 0.0)
            assert torch.equal(out.cpu(), ref.float()), (cout, cin, taps, nsplit, acc)
            assert guard_ok(buf, n)


def test_wgrad3x3_oihw_sum_planes_matches_wgrad3x3_to_oihw(dev):
    """the direct 3x3 weight gradient at a shape with more than one split-K slice: slices in the parameter's order + sum_planes against
    slices in GEMM order + wgrad_to_oihw, and both against the fp64 im2col GEMM (dyadic bf16 operands: every partial sum is exact)"""
    from stedm_amd import ops
    from stedm_amd._lib import BF16
    prec = ops.Precision(BF16, 1)
    B, H, W, cin, cout = 4, 16, 8, 128, 64
    ks = ops.wgrad3x3_plan(B, H, W, cin, cout)
    assert ks > 1, ks
    x, dy = R.dyadic((B, H, W, cin), 91), R.dyadic((B, H, W, cout), 92)
    x16 = x.to(torch.bfloat16).view(torch.int16).to(dev)
    dy16 = dy.to(torch.bfloat16).view(torch.int16).to(dev)
    n = cout * cin * 9
    part_a = nanfull((ks, 9, cin, cout), dev)
    ops.wgrad3x3(x16, dy16, part_a, prec)
    buf_a, grad_a = guarded(n, dev)
    ops.wgrad_to_oihw(part_a, grad_a.view(cout, cin, 3, 3), cin, cout, False, ks)
    part_b = nanfull((ks, cout, cin, 3, 3), dev)
    ops.wgrad3x3_oihw(x16, dy16, part_b, prec)
    buf_b, grad_b = guarded(n, dev)
    ops.sum_planes(part_b, grad_b, ks)
    assert not bool(torch.isnan(part_a).any()) and not bool(torch.isnan(part_b).any())
    assert torch.equal(part_b.cpu(), part_a.permute(0, 3, 2, 1).reshape(ks, cout, cin, 3, 3).cpu())
    assert torch.equal(grad_a, grad_b) and guard_ok(buf_a, n) and guard_ok(buf_b, n)
    P = B * H * W
    col = R.im2col_t(x.double(), 3, 0, P)
    ref = R.wgrad_to_oihw((col @ dy.double().view(P, cout)).view(1, 9, cin, cout), cout, cin)
    assert torch.equal(grad_a.cpu(), ref.float().view(-1))


@pytest.mark.parametrize("rows,dim", [(1, 1), (1, 100), (65, 1), (65, 2048), (4098, 100), (4098, 2048), (131072 + 5, 64)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_ln_bwd_dbeta_exact(dev, rows, dim, accumulate):
    """dyadic dy: dbeta is exactly the column sums (plus the prior value); dx has no unwritten element"""
    from stedm_amd import ops
    x, _, gamma, _ = R.ln_inputs(rows, dim)
    dy = R.dyadic((rows, dim), 93)
    prior = R.dyadic((dim,), 94)
    dx = nanfull((rows, dim), dev)
    dgamma = prior.to(dev) if accumulate else nanfull((dim,), dev)
    dbeta = prior.to(dev) if accumulate else nanfull((dim,), dev)
    ops.ln_bwd(x.to(dev), dy.to(dev), gamma.to(dev), R.LN_EPS, dx, dgamma, dbeta, None, accumulate)
    ref = dy.double().sum(0) + (prior.double() if accumulate else 0.0)
    assert torch.equal(dbeta.cpu(), ref.float())
    assert not bool(torch.isnan(dx).any()) and not bool(torch.isnan(dgamma).any())


# ================================================================================================ rounded kernels
def test_silu_bounds(dev):
    """forward: c = 6 = exp argument (2 |x|, inside the (1 + |x|) factor) + v_exp_f32 2 + add 1 + v_rcp_f32 2 + product 1, in units of 2^-24,
    relative to |ref|. gradient: c = 12 relative to |dy| sigmoid(x) (1 + |x| (1 - sigmoid(x))), the magnitudes of the two terms of silu':
    silu' changes sign at x = -1.2785, so no bound relative to |ref| holds there for any fp32 evaluation (tests/test_bwd_refs_cpu.py shows it
    for correctly rounded fp32 torch); for x >= 0 the two forms are the same number. Derivations: tests/refs_bwd.py."""
    from stedm_amd import ops
    x, dy = R.silu_inputs()
    xd, dyd = x.to(dev), dy.to(dev)
    x64, dy64 = xd.double(), dyd.double()
    out = nanfull(x.shape, dev)
    ops.silu(xd, out)
    e_f = (out.double() - R.silu(x64)).abs()
    b_f = R.silu_bound(x64, R.silu(x64))
    outg = nanfull(x.shape, dev)
    ops.silu(xd, outg, dyd)
    e_g = (outg.double() - R.silu_grad(x64, dy64)).abs()
    b_g = R.silu_grad_bound(x64, dy64)
    print(f"\nsilu worst err/bound {worst(e_f, b_f):.3f}; silu_grad {worst(e_g, b_g):.3f}")
    for name, e, b in (("silu", e_f, b_f), ("silu_grad", e_g, b_g)):
        bad = (~(e <= b)).nonzero().view(-1)[:8].cpu()
        assert bad.numel() == 0, (name, [(float(x[i]), float(e[i]), float(b[i])) for i in bad])


@pytest.mark.parametrize("M,I", R.GEGLU_SHAPES)
def test_geglu_bwd_bounds(dev, M, I):
    """|err d_value| <= 8 u |d gate|, |err d_gate| <= 12 u |d value| (u = 2^-24): absolute in cdf, because 1 + erf cancels for negative gates
    (derivation and operation counts in tests/refs_bwd.py). 20481 x 1280 is past one trip of the grid-stride loop (65536 blocks x 256)."""
    from stedm_amd import ops
    g, dh = R.geglu_inputs(M, I)
    gd, dhd = g.to(dev), dh.to(dev)
    dg = nanfull((M, 2 * I), dev)
    ops.geglu_bwd(gd, dhd, dg)
    g64, dh64 = gd.double(), dhd.double()
    err = (dg.double() - R.geglu_bwd(g64, dh64)).abs()
    bound = R.geglu_bwd_bound(g64, dh64)
    print(f"\ngeglu_bwd M={M} I={I} worst err/bound {worst(err, bound):.3f}")
    assert bool((err <= bound).all()), worst(err, bound)


@pytest.mark.parametrize("rows,dim", R.LN_SHAPES)
def test_ln_bwd_bounds(dev, rows, dim):
    """dx per element inside refs_bwd.ln_bwd_dx_bound ((D / 2 + 9.5) u rstd (|dxh| + |m1| + |xh m2|) plus the summation terms of the three row
    means, D = ceil(dim / 64) + 6), dgamma / dbeta inside the worst-case column bounds; add None / given x accumulate 0 / 1; the workspace is
    exactly ln_bwd_ws_floats with guard words behind it. rows = 131077 gives a block 65 rows."""
    from stedm_amd import ops
    x, dy, gamma, add = (t.to(dev) for t in R.ln_inputs(rows, dim))
    x64, dy64, g64, a64 = x.double(), dy.double(), gamma.double(), add.double()
    prior_g, prior_b = R.normal((dim,), 95, "ln.pg").to(dev), R.normal((dim,), 95, "ln.pb").to(dev)
    rpb, nb = R.ln_block_rows(rows)
    need = ops.ln_bwd_ws_floats(rows, dim)
    assert need >= 2 * dim * nb
    wx = wg = wb = 0.0
    for with_add in (False, True):
        rx, rg, rb = R.ln_bwd(x64, dy64, g64, R.LN_EPS, a64 if with_add else None)
        bx = R.ln_bwd_dx_bound(x64, dy64, g64, R.LN_EPS, a64 if with_add else None)
        for acc in (False, True):
            dx = nanfull((rows, dim), dev)
            dgamma = prior_g.clone() if acc else nanfull((dim,), dev)
            dbeta = prior_b.clone() if acc else nanfull((dim,), dev)
            wsbuf, ws = guarded(need, dev)
            ops.ln_bwd(x, dy, gamma, R.LN_EPS, dx, dgamma, dbeta, add if with_add else None, acc, ws)
            bg, bb = R.ln_bwd_param_bounds(x64, dy64, R.LN_EPS, rpb, nb, prior_g.double() if acc else None, prior_b.double() if acc else None)
            eg = (dgamma.double() - (rg + (prior_g.double() if acc else 0.0))).abs()
            eb = (dbeta.double() - (rb + (prior_b.double() if acc else 0.0))).abs()
            ex = (dx.double() - rx).abs()
            tag = (rows, dim, with_add, acc)
            assert guard_ok(wsbuf, need), tag
            assert bool((ex <= bx).all()), (tag, worst(ex, bx))
            assert bool((eg <= bg).all()) and bool((eb <= bb).all()), (tag, worst(eg, bg), worst(eb, bb))
            wx, wg, wb = max(wx, worst(ex, bx)), max(wg, worst(eg, bg)), max(wb, worst(eb, bb))
    print(f"\nln_bwd rows={rows} dim={dim} worst err/bound dx {wx:.3f} dgamma {wg:.3f} dbeta {wb:.3f}")


@pytest.mark.parametrize("rows,dim", [(4098, 100), (131072 + 5, 64)])
def test_ln_bwd_one_row_probes(dev, rows, dim):
    """dy nonzero in a single row: dbeta must be that row exactly and dgamma must be dy * xh inside the per-element bound of one term (the
    worst-case column bound of a whole tensor cannot see one lost row). Probed: the first row, rows 63 and 64 (the last row of the first block
    and the first of the second at 64 rows per block; the last two rows of the first block at 65), the last row of a middle block, the first
    and the last row of the last block (= the last row)."""
    from stedm_amd import ops
    x, dy_full, gamma, _ = R.ln_inputs(rows, dim)
    xd, gd = x.to(dev), gamma.to(dev)
    rpb, nb = R.ln_block_rows(rows)
    xh64, _ = R.ln_stats(x.double(), R.LN_EPS)
    w = 0.0
    for r in (0, 63, 64, rpb - 1, 5 * rpb - 1, 5 * rpb, (nb - 1) * rpb - 1, (nb - 1) * rpb, rows - 1):
        dy = torch.zeros((rows, dim))
        dy[r] = dy_full[r]
        dx, dgamma, dbeta = nanfull((rows, dim), dev), nanfull((dim,), dev), nanfull((dim,), dev)
        ops.ln_bwd(xd, dy.to(dev), gd, R.LN_EPS, dx, dgamma, dbeta)
        assert torch.equal(dbeta.cpu(), dy[r]), r
        ref = dy[r].double() * xh64[r]
        bound = R.ln_bwd_dgamma_term_bound(x[r:r + 1].double(), dy[r:r + 1].double(), R.LN_EPS)[0]
        err = (dgamma.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), (r, worst(err, bound))
        w = max(w, worst(err, bound))
        assert not bool(torch.isnan(dx).any()), r
    print(f"\nln_bwd one-row probes rows={rows} dim={dim} worst dgamma err/bound {w:.3f}")


# ================================================================================================ argument rejection
def test_bad_arguments_are_rejected_and_nothing_is_written(dev):
    from stedm_amd import ops
    from stedm_amd._lib import F16, StedmHipError
    prec = ops.Precision(F16, 1)

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == NAN16).all()) for t in ts)

    out = nanfull((1, 2, 2, 6), dev)
    with pytest.raises(StedmHipError):
        ops.sum2x2(torch.ones((1, 4, 4, 6), device=dev), out, False)
    assert untouched(out)
    hi, lo = nanfull((1, 4, 4, 6), dev, torch.float16), nanfull((1, 4, 4, 6), dev, torch.float16)
    with pytest.raises(StedmHipError):
        ops.zero_insert16(torch.ones((1, 2, 2, 6), device=dev), hi, lo, prec)
    assert untouched(hi, lo)
    for C, Ppad in ((12, 128), (8, 128 + 32), (8, 64)):          # C % 8, Ppad % 64, Ppad < P = 2 * 8 * 8
        dst = torch.full((C, Ppad), NAN16, dtype=torch.int16, device=dev)
        with pytest.raises(StedmHipError):
            ops.im2col_t16(torch.ones((2, 8, 8, C), dtype=torch.int16, device=dev), dst, 1, 0)
        assert untouched(dst)
    dx, dg, db = nanfull((2, 2049), dev), nanfull((2049,), dev), nanfull((2049,), dev)
    ws = nanfull((ops.ln_bwd_ws_floats(2, 2049),), dev)
    with pytest.raises(StedmHipError):
        ops.ln_bwd(torch.ones((2, 2049), device=dev), torch.ones((2, 2049), device=dev), torch.ones((2049,), device=dev), 1e-5, dx, dg, db, None, False, ws)
    assert untouched(dx, dg, db, ws)
    grad = nanfull((4, 4, 10), dev)
    with pytest.raises(StedmHipError):
        ops.wgrad_to_oihw(torch.ones((1, 10, 4, 4), device=dev), grad, 4, 4, False, 1)
    assert untouched(grad)
    grad = nanfull((4, 8, 1), dev)
    with pytest.raises(StedmHipError):
        ops.wgrad_to_oihw(torch.ones((1, 1, 8, 4), device=dev), grad, 7, 4, False, 1)
    assert untouched(grad)
