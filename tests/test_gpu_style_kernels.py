"""GPU tier (-m gpu): the small kernels around the style encoders, the VQ first stage and the prediction epilogue (svit.hip, swin.hip, vq.hip,
post.hip, misc.hip), each called through its `ops` wrapper and held against the plain references of tests/refs_style.py at the shapes where
such kernels go wrong: lane tails, idle lanes and waves, every pooling path of svit_head, both lane widths of swin_ln, pad columns, strided
views, a second trip of a grid-stride loop.

  exact kernels (gathers, casts, table lookups, fixed-order sums): torch.equal; sums on dyadic inputs also against the fp64 result
  rounded kernels: per-element bounds derived in tests/refs_style.py from the operation counts, none of them taken from a run of a kernel;
  tests/test_style_refs_cpu.py holds the same bounds against fp32 torch. Each test prints its worst error / bound.
  16-bit planes: the asserted invariant is on the PAIR, |hi + lo - ref| inside the kernel's bound plus what the lo plane cannot hold, and hi
  inside the bound plus half a 16-bit ulp: under the current compiler an f16 hi is a single rounding of the exact product in geglu16,
  ln_apply16 and svit_patch_ln16 (v_fma_mixlo_f16), which may differ from fp32_value.to(float16) by one ulp and is right with its own lo.

Outputs and workspaces are filled with NaN before the call; flat buffers are followed by guard words."""
import pytest
import torch

from tests import refs_style as R

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
GUARD = 1234.5
DTS = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def nanfull(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def guarded(n, dev, dtype=torch.float32, guard=64):
    """flat buffer of n NaN elements followed by `guard` guard words; returns (whole buffer, view of the first n)"""
    buf = torch.full((n + guard,), GUARD, dtype=dtype, device=dev)
    buf[:n] = NAN
    return buf, buf[:n]


def guard_ok(buf, n):
    return bool((buf[n:] == GUARD).all())


def prec_of(dt):
    from stedm_amd import ops
    from stedm_amd._lib import BF16, F16
    return ops.Precision(F16 if dt == torch.float16 else BF16, 1)


def worst(err, bound):
    return float((err / bound).max())


def d(*ts):
    return tuple(None if t is None else t.double() for t in ts)


def check_planes(hi, lo, ref64, b, dt, tag):
    """hi inside the bound + half a 16-bit ulp; hi + lo inside the bound + what lo cannot hold. Every element, nothing filtered. Returns the worst ratio."""
    eh = (hi.double() - ref64).abs()
    bh = R.hi_bound(ref64, b, dt)
    assert bool((eh <= bh).all()), (tag, "hi", worst(eh, bh))
    w = worst(eh, bh)
    if lo is not None:
        ep = (hi.double() + lo.double() - ref64).abs()
        bp = R.pair_bound(ref64, b, dt)
        assert bool((ep <= bp).all()), (tag, "hi + lo", worst(ep, bp))
        w = worst(ep, bp)
    return w


def check_split(hi, lo, v32, dt, tag):
    rh, rl = R.split16(v32, dt)
    assert torch.equal(hi, rh), tag
    if lo is not None:
        assert torch.equal(lo, rl), tag


# ================================================================================================ exact kernels
def test_svit_tok_place_exact(dev):
    """the last case has more than 16384 x 256 float4 elements: a second trip of the grid-stride loop"""
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    for B, ntok, dim in [(B, n, dd) for B in (1, 3) for n in (1, 5) for dd in (4, 36)] + [(1, 466100, 36)]:
        tok = R.normal((B, ntok, dim), 51, "tp.tok").to(dev)
        pos, cls = R.normal((ntok + 2, dim), 51, "tp.pos").to(dev), R.normal((dim,), 51, "tp.cls").to(dev)
        n = B * (ntok + 2) * dim
        assert (n // 4 > 16384 * 256) == (ntok > 5)
        buf, x = guarded(n, dev)
        ops.svit_tok_place(tok, pos, cls, x.view(B, ntok + 2, dim))
        assert torch.equal(x.view(B, ntok + 2, dim), R.tok_place(tok, pos, cls)), (B, ntok, dim)
        assert guard_ok(buf, n)
    x = nanfull((1, 3, 6), dev)
    with pytest.raises(StedmHipError):
        ops.svit_tok_place(torch.ones((1, 1, 6), device=dev), torch.ones((3, 6), device=dev), torch.ones((6,), device=dev), x)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())


@pytest.mark.parametrize("gen", ["onehot", "dyadic"])
def test_seg_merge_exact(dev, gen):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    for K in (2, 3, 7):
        for HW in (1, 257):
            for B in (1, 3):
                if gen == "onehot":
                    cls = torch.randint(0, K, (B, 1, HW), generator=torch.Generator().manual_seed(K + HW + B))
                    seg = torch.nn.functional.one_hot(cls, K).permute(0, 3, 1, 2).float().contiguous()
                else:
                    seg = R.dyadic((B, K, 1, HW), 52)
                got = ops.seg_merge(seg.to(dev)).cpu()
                assert torch.equal(got, R.seg_merge(seg)), (K, HW, B)
                assert torch.equal(got.double(), R.seg_merge(seg.double())), (K, HW, B)
    with pytest.raises(StedmHipError):
        ops.seg_merge(torch.ones((1, 1, 2, 2), device=dev))


@pytest.mark.parametrize("dt", [torch.int64, torch.float32])
def test_step_set_t_exact(dev, dt):
    from stedm_amd import ops
    S = 50
    table = (torch.arange(S, 0, -1) * 20 - 1).to(dt) if dt == torch.int64 else R.normal((S,), 53, "sst.table")
    for B in (1, 257):
        for i in (0, S - 1):
            idx = torch.tensor([i], dtype=torch.int32, device=dev)
            buf = torch.full((B + 64,), -7, dtype=dt, device=dev)
            ops.step_set_t(table.to(dev), idx, buf[:B])
            assert torch.equal(buf[:B].cpu(), R.step_set_t(table, i, B)), (B, i)
            assert bool((buf[B:] == -7).all())


def test_agg_reduce_exact(dev):
    """max: exact (no +-0 ties in normal inputs); mean: the kernel's order in fp32, and the fp64 result on dyadic inputs"""
    from stedm_amd import ops
    B = 3
    for n in (1, 2, 8):
        for Fd in (1, 300):
            f = R.normal((B * n, Fd), 54, "agg.f")
            assert not bool((f == 0).any())
            buf, out = guarded(B * Fd, dev)
            ops.agg_reduce(f.to(dev), out.view(B, Fd), n, 1)
            assert torch.equal(out.view(B, Fd).cpu(), R.agg_max(f, n)) and guard_ok(buf, B * Fd), (n, Fd)
            buf, out = guarded(B * Fd, dev)
            ops.agg_reduce(f.to(dev), out.view(B, Fd), n, 0)
            assert torch.equal(out.view(B, Fd).cpu(), R.agg_mean_ordered(f, n)) and guard_ok(buf, B * Fd), (n, Fd)
            fd = R.dyadic((B * n, Fd), 55)
            buf, out = guarded(B * Fd, dev)
            ops.agg_reduce(fd.to(dev), out.view(B, Fd), n, 0)
            assert torch.equal(out.view(B, Fd).cpu(), R.agg_mean(fd.double(), n).float()), (n, Fd)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("with_lo", [True, False])
def test_swin_patch16_exact(dev, dt, with_lo):
    from stedm_amd import ops
    for H, W in ((4, 4), (8, 12)):
        nhwc = R.normal((2, H, W, 3), 56, "sp.img").to(dev)
        for img in (nhwc.permute(0, 3, 1, 2).contiguous(), nhwc.permute(0, 3, 1, 2)):
            rows = 2 * (H // 4) * (W // 4)
            hi = nanfull((rows, 64), dev, dt)
            lo = nanfull((rows, 64), dev, dt) if with_lo else None
            ops.swin_patch16(img, hi, lo, prec_of(dt))
            check_split(hi, lo, R.swin_patch_rows(img), dt, (H, W, img.is_contiguous()))
            assert bool((hi[:, 48:] == 0).all()) and (lo is None or bool((lo[:, 48:] == 0).all()))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("with_lo", [True, False])
def test_swin_merge16_exact(dev, dt, with_lo):
    from stedm_amd import ops
    for H, W in ((5, 7), (4, 6), (1, 1), (3, 2)):
        for C in (4, 32):
            x = R.normal((2, H, W, C), 57, "sm.x", std=3.0).to(dev)
            rows = 2 * ((H + 1) // 2) * ((W + 1) // 2)
            hi = nanfull((rows, 4 * C), dev, dt)
            lo = nanfull((rows, 4 * C), dev, dt) if with_lo else None
            ops.swin_merge16(x, hi, lo, prec_of(dt))
            check_split(hi, lo, R.swin_merge(x), dt, (H, W, C))


def test_swin_token_mean_exact(dev):
    from stedm_amd import ops
    for T in (1, 3, 25):
        for C in (1, 64, 65, 96):
            x = R.normal((2, T, C), 58, "tm.x")
            buf, out = guarded(2 * C, dev)
            ops.swin_token_mean(x.to(dev), out.view(2, C))
            assert torch.equal(out.view(2, C).cpu(), R.token_mean_ordered(x)) and guard_ok(buf, 2 * C), (T, C)
            xd = R.dyadic((2, T, C), 59)
            out = nanfull((2, C), dev)
            ops.swin_token_mean(xd.to(dev), out)
            assert torch.equal(out.cpu(), R.token_mean(xd.double()).float()), (T, C)


# ================================================================================================ set-ViT patch path
@pytest.mark.parametrize("shape", R.PATCH_SHAPES)
def test_svit_patch_ln16_bounds(dev, shape):
    """tokens per block 1, 2, 8 (exactly the 48 KB budget), 4 (just over it); patch_dim 144 and 48 leave a lane tail in the LayerNorm loops"""
    from stedm_amd import ops
    B, ns, H, W, p = shape
    img, g, b = (t.to(dev) for t in R.patch_inputs(shape))
    ref = R.patch_ln(*d(img), p, *d(g, b), R.LN_EPS)
    bound = R.patch_ln_bound(*d(img), p, *d(g, b), R.LN_EPS)
    n = ref.numel()
    w = 0.0
    for dt in DTS:
        for with_lo in (True, False):
            bh, hi = guarded(n, dev, dt)
            bl, lo = guarded(n, dev, dt) if with_lo else (None, None)
            ops.svit_patch_ln16(img, g, b, R.LN_EPS, hi, lo, p, prec_of(dt))
            w = max(w, check_planes(hi.view(ref.shape), None if lo is None else lo.view(ref.shape), ref, bound, dt, (shape, dt, with_lo)))
            assert guard_ok(bh, n) and (bl is None or guard_ok(bl, n))
    print(f"\nsvit_patch_ln16 {shape} worst err/bound {w:.3f}")


@pytest.mark.parametrize("shape", [(1, 2, 16, 48, 8), (2, 3, 8, 12, 4)])
@pytest.mark.parametrize("dim", [8, 300])
def test_svit_patch_embed_bounds(dev, shape, dim):
    """the kernel computes the Linear itself: the bound carries the patch_dim-term fma chain; token rows 0 and 1 are one rounded sum each"""
    from stedm_amd import ops
    B, ns, H, W, p = shape
    img, g, b = (t.to(dev) for t in R.patch_inputs(shape))
    wt, bias, pos, cls = (t.to(dev) for t in R.embed_inputs(shape, dim))
    ntok = (H // p) * (W // p)
    n = B * (ntok + 2) * dim
    buf, x = guarded(n, dev)
    x = x.view(B, ntok + 2, dim)
    ops.svit_patch_embed(img, g, b, R.LN_EPS, wt, bias, pos, cls, x, p)
    ref = R.patch_embed(*d(img), p, *d(g, b), R.LN_EPS, *d(wt, bias, pos, cls))
    bound = R.patch_embed_bound(*d(img), p, *d(g, b), R.LN_EPS, *d(wt, bias, pos))
    err = (x[:, 2:].double() - ref[:, 2:]).abs()
    print(f"\nsvit_patch_embed {shape} dim={dim} worst err/bound {worst(err, bound):.3f}")
    assert bool((err <= bound).all()), worst(err, bound)
    assert torch.equal(x[:, 0], (cls + pos[0]).expand(B, dim)) and torch.equal(x[:, 1], pos[1].expand(B, dim))
    assert guard_ok(buf, n)


# ================================================================================================ pooled head
@pytest.mark.parametrize("dim", R.HEAD_DIMS)
def test_svit_head_pooling_paths(dev, dim):
    """dim 4: 256 token lanes; 36: 28 lanes, 4 idle threads; 384: 2 lanes; 1024: 1 lane; 1028 and 6: the scalar fallback"""
    from stedm_amd import ops
    B, w = 3, 0.0
    for T in R.HEAD_TS:
        for ncls in R.HEAD_NCLS:
            x, c_old, g, b, wt, bias = (t.to(dev) for t in R.head_inputs(B, T, dim, ncls))
            for pool in (0, 1, 2):
                for co in (None, c_old):
                    a = d(x, co, g, b)
                    ref = R.head(a[0], pool, a[1], a[2], a[3], R.LN_EPS, *d(wt, bias))
                    bound = R.head_bound(a[0], pool, a[1], a[2], a[3], R.LN_EPS, *d(wt, bias))
                    buf, out = guarded(B * ncls, dev)
                    ops.svit_head(x, pool, co, g, b, R.LN_EPS, wt, bias, out.view(B, ncls))
                    err = (out.view(B, ncls).double() - ref).abs()
                    assert bool((err <= bound).all()), ((dim, T, ncls, pool, co is None), worst(err, bound))
                    assert guard_ok(buf, B * ncls)
                    w = max(w, worst(err, bound))
    print(f"\nsvit_head dim={dim} worst err/bound {w:.3f}")


@pytest.mark.parametrize("B,T", [(1, 256), (3, 300)])
@pytest.mark.parametrize("dim", [36, 384])
def test_svit_head_slab_path(dev, B, T, dim):
    """a workspace and T >= 256 pool over slabs in a first kernel. Dyadic x: the pooled sums are exact in any order, so the slab result must
    equal the direct one bit for bit (a mean divided by the slab count instead of T would not). ws of 1024 dim; of exactly 3 B dim (3 slabs);
    below 2 B dim (the direct path: ws stays untouched)."""
    from stedm_amd import ops
    ncls = 5
    x, c_old, g, b, wt, bias = (t.to(dev) for t in R.head_inputs(B, T, dim, ncls, dyadic_x=True))
    w = 0.0
    for pool in (0, 2):
        for co in (None, c_old):
            direct = nanfull((B, ncls), dev)
            ops.svit_head(x, pool, co, g, b, R.LN_EPS, wt, bias, direct)
            a = d(x, co, g, b)
            ref = R.head(a[0], pool, a[1], a[2], a[3], R.LN_EPS, *d(wt, bias))
            bound = R.head_bound(a[0], pool, a[1], a[2], a[3], R.LN_EPS, *d(wt, bias))
            err = (direct.double() - ref).abs()
            assert bool((err <= bound).all()), worst(err, bound)
            w = max(w, worst(err, bound))
            for nws, slabs in ((1024 * dim, True), (3 * B * dim, True), (2 * B * dim - 1, False)):
                buf, ws = guarded(nws, dev)
                out = nanfull((B, ncls), dev)
                ops.svit_head(x, pool, co, g, b, R.LN_EPS, wt, bias, out, ws)
                assert torch.equal(out, direct), (pool, co is None, nws)
                assert guard_ok(buf, nws)
                assert bool(torch.isnan(ws).all()) != slabs, (pool, nws)
                if nws == 3 * B * dim:
                    assert not bool(torch.isnan(ws).any())
    print(f"\nsvit_head slab B={B} T={T} dim={dim} worst err/bound {w:.3f}")


# ================================================================================================ rescaler, GEGLU
def test_spatial_rescale_bounds(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    wmax = 0.0
    for n_stages in (0, 1, 2):
        f = 1 << n_stages
        for mult in ((1, 1), (3, 5)):
            x, w = (t.to(dev) for t in R.rescale_inputs(n_stages, mult))
            for ww in (None, w):
                cout = 3 if ww is None else 5
                n = 2 * cout * mult[0] * mult[1]
                buf, out = guarded(n, dev)
                ops.spatial_rescale(x, ww, out.view(2, cout, mult[0], mult[1]), n_stages)
                ref = R.rescale(x.double(), None if ww is None else ww.double(), n_stages)
                bound = R.rescale_bound(x.double(), None if ww is None else ww.double(), n_stages)
                err = (out.view(ref.shape).double() - ref).abs()
                assert bool((err <= bound).all()), ((n_stages, mult, ww is None), worst(err, bound))
                assert guard_ok(buf, n)
                wmax = max(wmax, worst(err, bound))
    print(f"\nspatial_rescale worst err/bound {wmax:.3f}")
    out = nanfull((1, 3, 1, 2), dev)
    with pytest.raises(StedmHipError):
        ops.spatial_rescale(torch.ones((1, 3, 6, 8), device=dev), None, out, 2)
    out5 = nanfull((1, 5, 2, 2), dev)
    with pytest.raises(StedmHipError):
        ops.spatial_rescale(torch.ones((1, 3, 8, 8), device=dev), None, out5, 2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out5).all())


@pytest.mark.parametrize("M,I", R.GEGLU_SHAPES)
def test_geglu16_bounds(dev, M, I):
    """gates from -9 to 9; 233100 x 36 is past one trip of the grid-stride loop (8192 blocks x 256 threads x 4 elements)"""
    from stedm_amd import ops
    g = R.geglu_inputs(M, I).to(dev)
    assert (M * I // 4 > 8192 * 256) == (M > 3)
    ref, bound = R.geglu(g.double()), R.geglu_bound(g.double())
    w = 0.0
    for dt in DTS:
        for with_lo in (True, False):
            bh, hi = guarded(M * I, dev, dt)
            bl, lo = guarded(M * I, dev, dt) if with_lo else (None, None)
            ops.geglu16(g, hi, lo, prec_of(dt))
            w = max(w, check_planes(hi.view(M, I), None if lo is None else lo.view(M, I), ref, bound, dt, (M, I, dt, with_lo)))
            assert guard_ok(bh, M * I) and (bl is None or guard_ok(bl, M * I))
    print(f"\ngeglu16 M={M} I={I} worst err/bound {w:.3f}")


def test_geglu16_f16_constructed_ties(dev):
    """value x gate = +-2^k (1 + 2^-11 + 2^-24) with gates where GELU is the identity: the fp32 product is an exact f16 tie. One rounding of the
    exact product gives 1 + 2^-10, the rounding of the rounded product 1.0; each is right only with the lo taken against it, so hi + lo must
    be the fp32 product whichever hi the compiler chose (tests/test_style_refs_cpu.py shows that a mismatched pair is outside the bound)."""
    from stedm_amd import ops
    g = R.geglu_tie_inputs().to(dev)
    I = g.shape[1] // 2
    hi, lo = nanfull((1, I), dev, torch.float16), nanfull((1, I), dev, torch.float16)
    ops.geglu16(g, hi, lo, prec_of(torch.float16))
    ref, bound = R.geglu(g.double()), R.geglu_bound(g.double())
    w = check_planes(hi, lo, ref, bound, torch.float16, "ties")
    v32 = (g[:, :I] * g[:, I:]).double()
    single = int((hi.double() != v32.float().to(torch.float16).double()).sum())
    print(f"\ngeglu16 ties worst pair err/bound {w:.3f}; {single} of {I} hi values are single roundings of the exact product")
    # sharper than the bound here, where GELU is the identity: hi + lo is the fp32 product exactly (lo holds the 2^-11 remainder without rounding)
    assert torch.equal(hi.double() + lo.double(), v32)


# ================================================================================================ first stage
@pytest.mark.parametrize("rows", R.SOFTMAX_ROWS)
@pytest.mark.parametrize("n", R.SOFTMAX_NS)
def test_softmax_rows16_bounds(dev, rows, n):
    """x is a column slice of a wider tensor (ld_in = n + 7); the last row spreads its logits over +-80; ld_out = n, the next multiple of 64,
    and 64 more: columns n.. must be exactly zero in both planes; the rows after `rows` stay NaN; every row sums to 1 inside its summed bound"""
    from stedm_amd import ops
    wide, _ = R.softmax_inputs(rows, n)
    x = wide.to(dev)[:, 3:3 + n]
    assert x.stride(0) == n + 7
    ref, bound = R.softmax_scaled(x.double(), R.SOFTMAX_SCALE), R.softmax_bound(x.double(), R.SOFTMAX_SCALE)
    w = 0.0
    for ld in sorted({n, (n + 63) // 64 * 64, (n + 63) // 64 * 64 + 64}):
        for dt in DTS:
            for with_lo in (True, False):
                bh, hi = guarded(rows * ld, dev, dt, guard=2 * ld)
                bl, lo = guarded(rows * ld, dev, dt, guard=2 * ld) if with_lo else (None, None)
                hi2, lo2 = hi.view(rows, ld), None if lo is None else lo.view(rows, ld)
                ops.softmax_rows16(x, R.SOFTMAX_SCALE, hi2, lo2, prec_of(dt))
                tag = (rows, n, ld, dt, with_lo)
                assert guard_ok(bh, rows * ld) and (bl is None or guard_ok(bl, rows * ld)), tag
                assert bool((hi2[:, n:] == 0).all()) and (lo2 is None or bool((lo2[:, n:] == 0).all())), tag
                w = max(w, check_planes(hi2[:, :n], None if lo2 is None else lo2[:, :n], ref, bound, dt, tag))
                if with_lo:
                    tot = (hi2.double() + lo2.double()).sum(-1)
                    assert bool(((tot - 1.0).abs() <= R.pair_bound(ref, bound, dt).sum(-1)).all()), tag
    print(f"\nsoftmax_rows16 rows={rows} n={n} worst err/bound {w:.3f}")


@pytest.mark.parametrize("cin", R.CONV_CH)
def test_conv1x1_nchw_bounds(dev, cin):
    from stedm_amd import ops
    w = 0.0
    for cout in R.CONV_CH:
        for HW in R.CONV_HW:
            for B in (1, 3):
                x, wt, bias = (t.to(dev) for t in R.conv_inputs(B, cin, cout, HW))
                for bb in (None, bias):
                    out = ops.conv1x1_nchw(x, wt, bb)
                    a = d(x, wt, bb)
                    err = (out.double() - R.conv1x1(*a)).abs()
                    bound = R.conv1x1_bound(*a)
                    assert bool((err <= bound).all()), ((cin, cout, HW, B, bb is None), worst(err, bound))
                    w = max(w, worst(err, bound))
                x, wt, bias = (t.to(dev) for t in R.conv_inputs(B, cin, cout, HW, dyadic_in=True))
                for bb in (None, bias):
                    assert torch.equal(ops.conv1x1_nchw(x, wt, bb).double(), R.conv1x1(*d(x, wt, bb))), (cin, cout, HW, B)
    print(f"\nconv1x1_nchw cin={cin} worst err/bound {w:.3f}")


# ================================================================================================ Swin-V2
@pytest.mark.parametrize("dim", R.SWIN_LN_DIMS)
def test_swin_ln_bounds(dev, dim):
    """dim <= 192: 32 lanes per row, above: 64. out only / hi only / out + hi + lo; res absent, separate, aliased with out; plain and gated
    (gates 0, 1, 1 / (1 - p) over 1 or 3 rows each); ld16 = dim and dim + 32, where the pad columns keep the sentinel written before the call.
    A gate of 0 gives out == res bit for bit."""
    from stedm_amd import ops
    SENT = 7.0
    w = 0.0
    for rows in R.SWIN_LN_ROWS:
        y, g, b, res = (t.to(dev) for t in R.swin_ln_inputs(rows, dim))
        for r in (None, res):
            for rpg in ((None,) if rows != 9 else (None, 1, 3)):
                gate = None if rpg is None else R.swin_gates(rows // rpg).to(dev)
                a = d(y, g, b)
                ref = R.swin_ln(*a, R.LN_EPS, *d(r, gate), rpg or 1)
                bound = R.swin_ln_bound(*a, R.LN_EPS, *d(r, gate), rpg or 1)
                zero = None if gate is None else (gate.repeat_interleave(rpg) == 0)
                for dt in DTS:
                    for mode in ("out", "hi", "all"):
                        for alias in ((False, True) if (r is not None and mode != "hi") else (False,)):
                            for ld in ((dim,) if mode == "out" else (dim, dim + 32)):
                                tag = (dim, rows, r is None, rpg, dt, mode, alias, ld)
                                out = None if mode == "hi" else (r.clone() if alias else nanfull((rows, dim), dev))
                                hi = lo = None
                                if mode != "out":
                                    hi = torch.full((rows, ld), SENT, dtype=dt, device=dev); hi[:, :dim] = NAN
                                if mode == "all":
                                    lo = torch.full((rows, ld), SENT, dtype=dt, device=dev); lo[:, :dim] = NAN
                                ops.swin_ln(y, g, b, R.LN_EPS, out if alias else r, out, hi, lo, prec_of(dt), gate, rpg or 1)
                                if out is not None:
                                    err = (out.double() - ref).abs()
                                    assert bool((err <= bound).all()), (tag, worst(err, bound))
                                    w = max(w, worst(err, bound))
                                    if zero is not None and r is not None:
                                        assert torch.equal(out[zero], r[zero]), tag
                                if hi is not None:
                                    check_planes(hi[:, :dim], None if lo is None else lo[:, :dim], ref, bound, dt, tag)
                                    assert bool((hi[:, dim:] == SENT).all()) and (lo is None or bool((lo[:, dim:] == SENT).all())), tag
                                    if zero is not None and r is not None:
                                        check_split(hi[:, :dim][zero], None if lo is None else lo[:, :dim][zero], r[zero], dt, tag)
    print(f"\nswin_ln dim={dim} worst err/bound {w:.3f}")


@pytest.mark.parametrize("heads", [1, 3])
def test_swin_rpb_bounds(dev, heads):
    """the index holds an entry below 0 and two beyond the table: all clamp"""
    from stedm_amd import ops
    cpb, index = R.rpb_inputs(heads)
    assert int(index.min()) < 0 and int(index.max()) >= cpb.shape[0]
    got = ops.swin_rpb(cpb.to(dev), index.to(dev), heads).cpu()
    ref, bound = R.swin_rpb(cpb.double(), index, heads), R.swin_rpb_bound(cpb.double(), index, heads)
    err = (got.double() - ref).abs()
    print(f"\nswin_rpb heads={heads} worst err/bound {worst(err, bound):.3f}")
    assert bool((err <= bound).all()), worst(err, bound)


# ================================================================================================ f16 hi / lo pairs on large inputs
def _pair_report(name, hi, v32ref):
    n = int((hi.double() != v32ref.to(torch.float16).double()).sum())
    print(f"\n{name}: f16 pair holds; {n} of {hi.numel()} hi values differ from float16(the fp32 reference)")


@pytest.mark.parametrize("rows,dim,seed", [R.PAIR_LN_APPLY + (21,), R.PAIR_LN_APPLY_SCALAR + (25,)])
def test_ln_apply16_f16_pair(dev, rows, dim, seed):
    """an input with (tests/test_style_refs_cpu.py counts them) at least 8 elements whose f16 rounding differs between the fp32 and the fp64
    evaluation: a hi that is a single rounding is accepted, a pair whose halves disagree is not. dim 256: the vector form; 200: the scalar form."""
    from stedm_amd import ops
    x, g, b = (t.to(dev) for t in R.pair_ln_inputs(rows, dim, seed))
    hi, lo = nanfull((rows, dim), dev, torch.float16), nanfull((rows, dim), dev, torch.float16)
    ops.ln_apply16(x, g, b, R.PAIR_EPS, hi, lo, prec_of(torch.float16))
    a = d(x, g, b)
    check_planes(hi, lo, R.ln(*a, R.PAIR_EPS), R.ln_fwd_bound(*a, R.PAIR_EPS, R.ln_D(dim)), torch.float16, (rows, dim))
    _pair_report(f"ln_apply16 {rows}x{dim}", hi, R.ln(x, g, b, R.PAIR_EPS))


def test_svit_patch_ln16_f16_pair(dev):
    from stedm_amd import ops
    img, g, b = (t.to(dev) for t in R.pair_patch_inputs())
    p = R.PAIR_PATCH[4]
    ref = R.patch_ln(*d(img), p, *d(g, b), R.PAIR_EPS)
    hi, lo = nanfull(ref.shape, dev, torch.float16), nanfull(ref.shape, dev, torch.float16)
    ops.svit_patch_ln16(img, g, b, R.PAIR_EPS, hi, lo, p, prec_of(torch.float16))
    check_planes(hi, lo, ref, R.patch_ln_bound(*d(img), p, *d(g, b), R.PAIR_EPS), torch.float16, "pair")
    _pair_report("svit_patch_ln16", hi, R.patch_ln(img, p, g, b, R.PAIR_EPS))


@pytest.mark.parametrize("rows,dim,seed", [R.PAIR_SWIN_LN + (22,), R.PAIR_SWIN_LN_WIDE + (26,)])
def test_swin_ln_f16_pair(dev, rows, dim, seed):
    from stedm_amd import ops
    y, g, b = (t.to(dev) for t in R.pair_ln_inputs(rows, dim, seed))
    out = nanfull((rows, dim), dev)
    hi, lo = nanfull((rows, dim), dev, torch.float16), nanfull((rows, dim), dev, torch.float16)
    ops.swin_ln(y, g, b, R.PAIR_EPS, None, out, hi, lo, prec_of(torch.float16))
    a = d(y, g, b)
    check_planes(hi, lo, R.swin_ln(*a, R.PAIR_EPS), R.swin_ln_bound(*a, R.PAIR_EPS), torch.float16, (rows, dim))
    check_split(hi, lo, out, torch.float16, "planes of the stored fp32 value")      # what swin.hip's rounded() is there for
    _pair_report(f"swin_ln {rows}x{dim}", hi, R.swin_ln(y, g, b, R.PAIR_EPS))


def test_softmax_rows16_f16_pair(dev):
    from stedm_amd import ops
    x, scale = R.pair_softmax_inputs()
    x = x.to(dev)
    hi, lo = nanfull(x.shape, dev, torch.float16), nanfull(x.shape, dev, torch.float16)
    ops.softmax_rows16(x, scale, hi, lo, prec_of(torch.float16))
    check_planes(hi, lo, R.softmax_scaled(x.double(), scale), R.softmax_bound(x.double(), scale), torch.float16, "pair")
    _pair_report("softmax_rows16", hi, R.softmax_scaled(x, scale))


# ================================================================================================ argument rejection
def test_bad_arguments_are_rejected_and_nothing_is_written(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    prec = prec_of(torch.float16)

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in ts)

    hi, lo = nanfull((1, 4 * 4 * 3), dev, torch.float16), nanfull((1, 4 * 4 * 3), dev, torch.float16)
    with pytest.raises(StedmHipError):                                   # H % patch
        ops.svit_patch_ln16(torch.ones((1, 1, 6, 4, 3), device=dev), torch.ones((48,), device=dev), torch.ones((48,), device=dev), 1e-5, hi, lo, 4, prec)
    assert untouched(hi, lo)
    with pytest.raises(StedmHipError):                                   # cin = 17
        ops.conv1x1_nchw(torch.ones((1, 17, 2, 2), device=dev), torch.ones((3, 17), device=dev), None)
    one = lambda *s: torch.ones(s, device=dev)
    out, h = nanfull((2, 769), dev), nanfull((2, 769), dev, torch.float16)
    with pytest.raises(StedmHipError):                                   # dim = 769
        ops.swin_ln(one(2, 769), one(769), one(769), 1e-5, None, out, h, None, prec)
    assert untouched(out, h)
    out, h = nanfull((2, 96), dev), nanfull((2, 64), dev, torch.float16)
    with pytest.raises(StedmHipError):                                   # ld16 < dim
        ops.swin_ln(one(2, 96), one(96), one(96), 1e-5, None, out, h, None, prec)
    assert untouched(out, h)
    out = nanfull((9, 96), dev)
    with pytest.raises((StedmHipError, AssertionError)):                 # rows % rows_per_gate (the wrapper's own assert speaks first)
        ops.swin_ln(one(9, 96), one(96), one(96), 1e-5, None, out, None, None, prec, one(4), 2)
    assert untouched(out)
    from stedm_amd._lib import check, lib
    y, gb, gate = one(9, 96), one(96), one(4)                            # the C entry point itself, past the wrapper's assert
    rc = lib().stedm_swin_ln_gated(y.data_ptr(), gb.data_ptr(), gb.data_ptr(), 1e-5, None, out.data_ptr(), None, None, 9, 96, 96, gate.data_ptr(), 2,
                                   prec.mm_dtype, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(StedmHipError):
        check(rc, "stedm_swin_ln_gated")
    assert untouched(out)
