"""CPU tier: pins the references of tests/refs_bwd.py themselves, where there is no GPU. Each restatement equals torch autograd (or the
convolution it stands for) in fp64, and every tolerance formula the GPU file uses holds for the same expression evaluated by torch in fp32
against fp64 on the GPU test's own inputs: the reference alone passes its own bound."""
import pytest
import torch
import torch.nn.functional as F

from tests import refs_bwd as R
from tests import refs_conv as RC

# the GPU test modules switch autograd off at import; the tests below that differentiate switch it on for themselves
with_grad = torch.enable_grad()


def _close64(got, ref, tol=1e-11):
    scale = max(float(ref.abs().max()), 1.0)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= tol * scale, float((got - ref).abs().max()) / scale


def test_dyadic_sums_are_exact_in_any_order():
    v = R.dyadic(((1 << 17) - 1,), 3)
    assert float(v.abs().max()) == 1.0 and torch.equal(v * 8, (v * 8).round())
    ref = v.double().sum()
    for perm_seed in range(3):
        p = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(perm_seed))
        s = torch.zeros((), dtype=torch.float32)
        for chunk in v[p].split(4096):                  # a chain of fp32 partial sums, each of them exact
            s = s + chunk.sum(dtype=torch.float32)
        assert float(s) == float(ref)
        assert float(v[p].cumsum(0, dtype=torch.float32)[-1]) == float(ref)


def test_finite_bf16_bits():
    b = R.finite_bf16_bits((1 << 16,), 5)
    f = b.view(torch.bfloat16).float()
    assert bool(torch.isfinite(f).all()) and b.unique().numel() > 30000


@pytest.mark.parametrize("rows,dim", [(1, 1), (3, 64), (7, 100), (65, 320)])
@pytest.mark.parametrize("with_add", [False, True])
@with_grad
def test_ln_bwd_is_layer_norm_autograd(rows, dim, with_add):
    x, dy, gamma, add = (t.double() for t in R.ln_inputs(rows, dim))
    beta = R.normal((dim,), 2, "beta").double()
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = F.layer_norm(xr, (dim,), gr, br, R.LN_EPS)
    loss = (y * dy).sum() + ((xr * add).sum() if with_add else 0.0)
    gx, gg, gb = torch.autograd.grad(loss, (xr, gr, br))
    dx, dgamma, dbeta = R.ln_bwd(x, dy, gamma, R.LN_EPS, add if with_add else None)
    _close64(dx, gx); _close64(dgamma, gg); _close64(dbeta, gb)


@with_grad
def test_geglu_bwd_is_autograd():
    g, dh = (t.double() for t in R.geglu_inputs(5, 320))
    gr = g.clone().requires_grad_()
    val, gate = gr.chunk(2, dim=-1)
    (gg,) = torch.autograd.grad((val * F.gelu(gate) * dh).sum(), gr)
    _close64(R.geglu_bwd(g, dh), gg)


@with_grad
def test_silu_and_grad_are_autograd():
    x, dy = (t.double() for t in R.silu_inputs())
    xr = x.clone().requires_grad_()
    y = F.silu(xr)
    _close64(R.silu(x), y.detach())
    (gx,) = torch.autograd.grad((y * dy).sum(), xr)
    _close64(R.silu_grad(x, dy), gx)


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (3, 6, 10)])
@with_grad
def test_im2col_gemm_is_conv_weight_gradient(ks, mode, B, H, W):
    cin, cout = 8, 5
    x = R.normal((B, H, W, cin), 21, "x").double()
    Ho, Wo = (2 * H, 2 * W) if mode == 1 else ((H // 2, W // 2) if mode == 2 else (H, W))
    dy = R.normal((B, Ho, Wo, cout), 21, "dy").double()
    w = R.normal((cout, cin, ks, ks), 21, "w").double().requires_grad_()
    xn = x.permute(0, 3, 1, 2)
    if mode == 1:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    y = F.conv2d(xn, w, None, stride=2 if mode == 2 else 1, padding=ks // 2)
    assert tuple(y.shape) == (B, cout, Ho, Wo)
    (gw,) = torch.autograd.grad((y * dy.permute(0, 3, 1, 2)).sum(), w)
    P = B * Ho * Wo
    Ppad = (P + 63) // 64 * 64 + 64
    col = R.im2col_t(x, ks, mode, Ppad)
    assert tuple(col.shape) == (ks * ks * cin, Ppad) and float(col[:, P:].abs().max()) == 0.0
    dyT = torch.zeros((cout, Ppad), dtype=torch.float64)
    dyT[:, :P] = dy.reshape(P, cout).t()
    dw = (col @ dyT.t()).view(1, ks * ks, cin, cout)                       # dW[(tap, ci)][co]
    got = R.wgrad_to_oihw(dw, cout, cin).view(cout, cin, ks, ks)
    _close64(got, gw)


def test_wgrad_to_oihw_sums_the_slices_and_drops_the_padding():
    dw = R.dyadic((3, 9, 24, 50), 4).double()
    got = R.wgrad_to_oihw(dw, 48, 20)
    assert tuple(got.shape) == (48, 20, 9)
    assert torch.equal(got, dw.sum(0)[:, :20, :48].permute(2, 1, 0))
    assert torch.equal(R.sum_planes(dw.view(3, -1)), dw.sum(0).view(-1))


@with_grad
def test_zero_insert_conv_is_stride2_input_gradient():
    B, cin, cout, H, W = 2, 4, 6, 8, 12
    x = R.normal((B, cin, H, W), 22, "x").double().requires_grad_()
    w = R.normal((cout, cin, 3, 3), 22, "w").double()
    dy = R.normal((B, H // 2, W // 2, cout), 22, "dy").double()
    y = F.conv2d(x, w, None, stride=2, padding=1)
    (gx,) = torch.autograd.grad((y * dy.permute(0, 3, 1, 2)).sum(), x)
    z = R.zero_insert(dy).permute(0, 3, 1, 2)
    assert tuple(z.shape) == (B, cout, H, W)
    got = F.conv2d(z, w.flip(2, 3).transpose(0, 1), None, stride=1, padding=1)
    _close64(got, gx)


@with_grad
def test_sum2x2_is_upsample_gradient():
    x = R.normal((2, 4, 3, 5), 23, "x").double().requires_grad_()
    dy = R.normal((2, 6, 10, 4), 23, "dy").double()                         # NHWC
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    (gx,) = torch.autograd.grad((up * dy.permute(0, 3, 1, 2)).sum(), x)
    _close64(R.sum2x2(dy).permute(0, 3, 1, 2), gx)
    prior = R.normal((2, 3, 5, 4), 23, "prior").double()
    _close64(R.sum2x2(dy, prior), R.sum2x2(dy) + prior)


# ------------------------------------------------------------------------------------------------ convolution backward references
def _conv_fwd(x_nhwc, w, mode):
    xn = x_nhwc.permute(0, 3, 1, 2)
    if mode == 1:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    return F.conv2d(xn, w, None, stride=2 if mode == 2 else 1, padding=w.shape[-1] // 2)


@pytest.mark.parametrize("ks,mode", [(1, 0), (3, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (3, 6, 10), (2, 4, 14)])
@with_grad
def test_conv_backward_refs_are_autograd(ks, mode, B, H, W):
    """wgrad_ref, dgrad_ref (+ zero_insert for stride 2, + sum2x2 behind the nearest-2x upsample) and bias_ref against autograd through
    F.conv2d, F.interpolate(nearest) + conv2d and conv2d(stride=2, padding=1), in fp64, on ragged small shapes"""
    cin, cout = 7, 5
    Ho, Wo = R.wgrad_out_hw(H, W, mode)
    x = R.normal((B, H, W, cin), 31, "x").double().requires_grad_()
    w = R.normal((cout, cin, ks, ks), 31, "w").double().requires_grad_()
    b = R.normal((cout,), 31, "b").double().requires_grad_()
    dy = R.normal((B, Ho, Wo, cout), 31, "dy").double()
    y = _conv_fwd(x, w, mode) + b[None, :, None, None]
    assert tuple(y.shape) == (B, cout, Ho, Wo)
    gx, gw, gb = torch.autograd.grad((y * dy.permute(0, 3, 1, 2)).sum(), (x, w, b))
    xd, wd = x.detach(), w.detach()
    _close64(R.wgrad_ref(xd, dy, ks, mode), gw)
    _close64(R.bias_ref(dy), gb)
    if mode == 0:
        dx = R.dgrad_ref(dy, wd)
    elif mode == 1:
        dx = R.sum2x2(R.dgrad_ref(dy, wd))
    else:
        dx = R.dgrad_ref(R.zero_insert(dy), wd)
    _close64(dx, gx)                  # (x is NHWC itself: so is its gradient)


def test_backward_dyadic_ok_states_the_exactness_condition():
    R.backward_dyadic_ok(2 ** 18)
    with pytest.raises(AssertionError):
        R.backward_dyadic_ok(2 ** 18 + 1)
    # at the limit the fp32 sum of K products of magnitude 1 is still exact; every tier-1 case of the GPU file stays below it
    assert float(torch.tensor(2.0 ** 18, dtype=torch.float32) - 1.0 / 64) != 2.0 ** 18
    assert float(torch.tensor(2.0 ** 19, dtype=torch.float32) - 1.0 / 64) == 2.0 ** 19


def test_dyadic_backward_in_fp32_equals_fp64_bit_for_bit():
    """the tier-1 argument on the references themselves: on dyadic data the fp32 evaluation of every reference IS the fp64 one"""
    x, dy, w = R.dyadic((3, 6, 10, 16), 1), R.dyadic((3, 6, 10, 24), 2), R.dyadic((24, 16, 3, 3), 3)
    R.backward_dyadic_ok(9 * 24); R.backward_dyadic_ok(3 * 6 * 10)
    assert torch.equal(R.dgrad_ref(dy, w).double(), R.dgrad_ref(dy.double(), w.double()))
    assert torch.equal(R.wgrad_ref(x, dy, 3, 0).double(), R.wgrad_ref(x.double(), dy.double(), 3, 0))
    assert torch.equal(R.bias_ref(dy).double(), R.bias_ref(dy.double()))
    hi, lo = R.split16(x, torch.bfloat16)
    assert torch.equal(hi.float(), x) and not bool(lo.float().any())           # the 16-bit planes hold the values themselves, lo is zero


def _planes64(x32, parity):
    hi, lo = R.split16(x32, torch.bfloat16)
    return hi.double(), (lo.double() if parity else None)


def _t2_ratio(fn, a, b, parity):
    """max |fp32 torch - fp64| / (u S) of fn over the rounded planes of (a, b): what the GPU tier asserts of the kernels, here of torch"""
    ah, al = _planes64(a, parity)
    bh, bl = _planes64(b, parity)
    if parity:
        ref = RC.three_products(ah, al, bh, bl, fn)
        got = RC.three_products(ah.float(), al.float(), bh.float(), bl.float(), fn).double()
        S = fn(ah.abs() + al.abs(), bh.abs() + bl.abs())
    else:
        ref, got, S = fn(ah, bh), fn(ah.float(), bh.float()).double(), fn(ah.abs(), bh.abs())
    return float(((got - ref).abs() / (R.U * S)).max())


@pytest.mark.parametrize("name", list(R.DGRAD_T2) + list(R.DGRAD_T2_PARITY))
def test_dgrad_tier2_bound_holds_for_fp32_torch(name):
    parity = name in R.DGRAD_T2_PARITY
    dy, w = R.dgrad_t2_inputs(name, (R.DGRAD_T2_PARITY if parity else R.DGRAD_T2)[name])
    r = _t2_ratio(R.dgrad_ref, dy, w, parity)
    print(f"fp32 torch {name} max err / (u S) = {r:.3f}")
    assert r <= RC.G


@pytest.mark.parametrize("name", list(R.WGRAD_T2) + list(R.WGRAD_T2_PARITY))
def test_wgrad_tier2_bound_holds_for_fp32_torch(name):
    parity = name in R.WGRAD_T2_PARITY
    shape = (R.WGRAD_T2_PARITY if parity else R.WGRAD_T2)[name]
    src, dy = R.wgrad_t2_inputs(name, shape)
    r = _t2_ratio(lambda s_, d_: R.wgrad_ref(s_, d_, shape[5], shape[6]), src, dy, parity)
    print(f"fp32 torch {name} max err / (u S) = {r:.3f}")
    assert r <= RC.G


def test_chan_sum_fold_and_q_sample_and_l1():
    cs = R.dyadic((5, 3, 8, 2), 6)
    per, tot = R.chan_sum_fold(cs.double())
    assert torch.equal(per, cs[..., 0].double().sum(1)) and torch.equal(tot, cs[..., 0].double().sum((0, 1)))
    x0, nz = R.normal((3, 7), 7, "x0"), R.normal((3, 7), 7, "nz")
    sa, s1 = torch.rand(10), torch.rand(10)
    t = torch.tensor([0, 9, 4])
    ref = torch.stack([sa[t[b]] * x0[b] + s1[t[b]] * nz[b] for b in range(3)])
    assert torch.equal(R.q_sample(x0, nz, t, sa, s1), ref)
    p, q = R.dyadic((255,), 8), R.dyadic((255,), 9)
    loss, d = R.l1(p, q, 3.0)
    assert float(loss) == float(torch.tensor(float((p.double() - q.double()).abs().sum()) / 255).float())
    assert torch.equal(d, torch.sign(p - q) * torch.tensor(3.0 / 255, dtype=torch.float32)) and bool((d[p == q] == 0).all())


@pytest.mark.parametrize("n", R.L1_NS)
def test_l1_reference_has_one_rounding(n):
    """the kernel forms sum * (1 / n) in fp64 and rounds to fp32, the reference float32(sum / n): on these inputs the two agree, so the exact
    comparison of the GPU test is a fair one"""
    p, q = R.l1_inputs(n)
    s = (p.double() - q.double()).abs().sum()
    assert float(s) * 8 == round(float(s) * 8) and float(s) < 2.0 ** 50
    assert float((s / n).float()) == float((s * (1.0 / n)).float()) == float(R.l1(p, q, 1.0)[0])


# ------------------------------------------------------------------------------------------------ the reference passes its own bounds
def _worst(err, bound):
    return float((err / bound).max())


def test_silu_bounds_hold_for_fp32_torch():
    x, dy = R.silu_inputs()
    x64, dy64 = x.double(), dy.double()
    r = _worst((R.silu(x).double() - R.silu(x64)).abs(), R.silu_bound(x64, R.silu(x64)))
    rg = _worst((R.silu_grad(x, dy).double() - R.silu_grad(x64, dy64)).abs(), R.silu_grad_bound(x64, dy64))
    print(f"fp32 torch silu err/bound {r:.3f}, silu_grad {rg:.3f}")
    assert r <= 1.0 and rg <= 1.0


def test_silu_grad_has_no_bound_relative_to_its_own_value():
    """why silu_grad_bound is relative to the magnitudes of the two terms of silu' and not to |silu'|: silu' crosses zero at x = -1.2785,
    where a correctly rounded fp32 evaluation already misses c (1 + |x|) 2^-24 |ref| by orders of magnitude"""
    x = torch.linspace(-1.2790, -1.2780, 2001, dtype=torch.float32)
    dy = torch.ones_like(x)
    ref = R.silu_grad(x.double(), dy.double())
    err = (R.silu_grad(x, dy).double() - ref).abs()
    naive = R.SILU_GRAD_C * (1.0 + x.double().abs()) * R.U * ref.abs() + R.TINY
    assert _worst(err, naive) > 1.0
    assert _worst(err, R.silu_grad_bound(x.double(), dy.double())) <= 1.0


@pytest.mark.parametrize("M,I", [s for s in R.GEGLU_SHAPES if s[0] * s[1] < 1 << 24])
def test_geglu_bound_holds_for_fp32_torch(M, I):
    g, dh = R.geglu_inputs(M, I)
    assert M * I == 1 or (float(g[:, I:].min()) <= -12.0 and float(g[:, I:].max()) >= 12.0)
    r = _worst((R.geglu_bwd(g, dh).double() - R.geglu_bwd(g.double(), dh.double())).abs(), R.geglu_bwd_bound(g.double(), dh.double()))
    print(f"fp32 torch geglu_bwd err/bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("rows,dim", R.LN_SHAPES)
def test_ln_bounds_hold_for_fp32_torch(rows, dim):
    x, dy, gamma, add = R.ln_inputs(rows, dim)
    x64, dy64, g64, a64 = x.double(), dy.double(), gamma.double(), add.double()
    rpb, nb = R.ln_block_rows(rows)
    worst = 0.0
    for a32, a in ((None, None), (add, a64)):
        dx, dg, db = R.ln_bwd(x, dy, gamma, R.LN_EPS, a32)
        rx, rg, rb = R.ln_bwd(x64, dy64, g64, R.LN_EPS, a)
        bg, bb = R.ln_bwd_param_bounds(x64, dy64, R.LN_EPS, rpb, nb)
        worst = max(worst, _worst((dx.double() - rx).abs(), R.ln_bwd_dx_bound(x64, dy64, g64, R.LN_EPS, a)),
                    _worst((dg.double() - rg).abs(), bg), _worst((db.double() - rb).abs(), bb))
    xh32, _ = R.ln_stats(x, R.LN_EPS)
    xh64, _ = R.ln_stats(x64, R.LN_EPS)
    worst = max(worst, _worst(((dy * xh32).double() - dy64 * xh64).abs(), R.ln_bwd_dgamma_term_bound(x64, dy64, R.LN_EPS)))
    print(f"fp32 torch ln_bwd rows={rows} dim={dim} err/bound {worst:.3f}")
    assert worst <= 1.0


def test_ln_block_rows():
    assert R.ln_block_rows(1) == (1, 1) and R.ln_block_rows(64) == (64, 1) and R.ln_block_rows(65) == (33, 2)
    assert R.ln_block_rows(4098) == (64, 65) and R.ln_block_rows(131072) == (64, 2048) and R.ln_block_rows(131077) == (65, 2017)
