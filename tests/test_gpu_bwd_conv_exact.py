"""GPU tier (-m gpu): the Python dispatch of stedm_amd/train.py that turns a layer's backward into kernel calls - _dpack, _dgrad, _wgrad,
_wgrad_gemm, _up_bwd, _down_bwd and the padded packs of the first / last convolution - called directly on a trainer over the TINY U-Net
and held against the plain references of tests/refs_bwd.py (wgrad_ref, dgrad_ref, zero_insert, sum2x2, bias_ref), in the two tiers of
tests/test_gpu_conv_exact.py:

  tier 1, bit-exact (every case): dyadic activations, gradients, weights and prior contents (refs_bwd.dyadic; the 16-bit planes are
    refs_bwd.split16 of them, the lo plane all zero). Every product is a multiple of 1/64 and every fp32 partial sum is exact in any order
    (refs_bwd.backward_dyadic_ok states the condition per case), so whichever pack, kernel, K split, batch chunk or launch split a branch
    takes, the result must equal the fp64 gradient of the ORIGINAL tensors: torch.equal. One missing, doubled or misplaced term fails; so
    does a filter that is not flipped / transposed, a chunk that overwrites instead of accumulating, a prior value that is dropped.
    Outputs are filled with NaN first (except where a prior value is part of the case); a second identical call must give the same bits.
  tier 2, operand-exact (marked cases): silu(1.3 x + 0.1) activations, 0.1 N(0, 1) gradients, N(0, 1) / sqrt(K) weights. Activations and
    gradients are handed over as their rounded planes, the reference weights are read back from ops.pack_conv_weight_strided(...,
    want_hi=True) of the arguments _dpack uses; the parity trainer uses hi + lo and refs_conv.three_products. Asserted elementwise:
    |out - ref64| <= G u S, G = refs_conv.G = 8, S the same operation on the magnitudes. tests/test_bwd_refs_cpu.py holds torch's own fp32
    evaluation of the same shapes and inputs to the same bound.

Every case asserts the branch it took, from a trace of the ops.* calls the dispatch made (which weight-gradient kernel, how many batch
chunks with which accumulate flags, how many GEMM launches, whether a fragment pack was built), from ops.wgrad3x3_plan / wgrad1x1_plan,
and for the dgrad convolutions from conv_igemm(query_rs=True) re-issued with the very arguments of the traced call: the lazy hi planes
must have been materialised exactly when the query declines the register-streamed kernel. If the query and the dispatcher inside
stedm_conv_igemm disagreed, an LDS-operand kernel would read the fragment pack as [O][taps][I] planes: wrong numbers, which tier 1 catches.
The expected answers are those of a 256-CU device (asserted through ops.device_cus()); they follow conv_rs_pick's rule for a 3x3 with
T = 256-row tiles x 128-column tiles: admitted on a full grid when 4 T >= 3 CUs (T >= 192), else only with a K split (the workspace of
UNetTrainer._ws is always there) of at least 1 / 2 / 4 chunks per share for T <= 16 / <= 32 / more. So at 8 x 8 with 64 forward output
channels (4 chunks of 16) B <= 128 (T <= 32) runs register-streamed with a K split, B = 129 .. 767 falls to the LDS-operand kernels.
Four cases therefore reach another branch than their names (from the plan of this file) say; they keep their shape and data, assert the
branch they do reach, and a neighbour reaches the named one:
  d_frag_rs  (25, 32, 32; 32 -> 64): T = 100, 4 chunks: declined, planes materialised   (d_frag_rs_full, B = 48: T = 192, admitted)
  d_frag_lds (3, 8, 8; 32 -> 64):    T = 1: admitted with a 4-way K split               (d_frag_lds_declined, B = 129: T = 33, declined)
  d_m16      (97, 16, 16; 64 -> 288): T = 97, 9 chunks of 32: declined                  (d_m16_full, B = 769 at 8 x 8, 32 -> 256: T = 193)
  w_chunks mode 2 (9 samples, dy 64 x 64): Bc = 16 holds all nine, ONE chunk            (w_chunks_mode2, 17 samples: 16 + 1)

Measured on an MI355X, max over the output of |out - ref64| / (u S), G = 8 (fp32 torch on the CPU tier in brackets):

  d_frag_rs              1.88 (0.74)      d_splitk               0.21 (0.21)      w_gemm_frag              1.33 (2.64)
  d_frag_rs_full         1.87 (0.82)      d_splitk_acc           0.24             w_chunks                 0.19 (0.09)
  d_frag_lds             0.40 (0.58)      d_parity_frag_lds      2.03 (0.63)      w_parity_nofrag          3.85 (2.83)
  d_frag_lds_declined    1.69 (0.83)      w_direct_n             0.48 (0.65)      w_parity_nofrag_ragged   3.00 (3.66)
  d_m16                  1.97 (0.75)      w_direct_n_t           0.48             w_parity_mode2           2.60 (2.27)
  d_m16_small            0.34 (0.40)      d_m16_full             2.28 (0.61)

(The largest single-product figure is 2.28, the largest of all 3.85 in the three-product GEMM form at K = 128, where fp32 torch sits at
2.8 .. 3.7 itself: few terms, activations of one sign. The K-split forms stay under 0.5. No form comes near G; no case failed tier 1.)
"""
import contextlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from stedm_amd.utils import prng
from tests import refs_bwd as R
from tests import refs_conv as RC

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
U = R.U
G = RC.G
BF = torch.bfloat16
CUS = 256              # the branch expectations below are those of a 256-CU device
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
TRACED = ("conv_igemm", "pack_conv_weight", "pack_conv_weight_strided", "pack_conv_weight_frag16", "im2col_t16", "wgrad_to_oihw", "wgrad3x3",
          "wgrad3x3_oihw", "wgrad1x1", "sum_planes", "sum2x2", "zero_insert16")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def _trainer(dev, precision):
    from stedm_amd.train import UNetTrainer
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, **TINY).eval()
    prng.fill_module_(m, seed=6)
    m = m.to(dev)
    tr = UNetTrainer(m)
    m._prepare()
    tr._alloc_grads()
    return tr


@pytest.fixture(scope="module")
def tr1(dev):
    """single-product backward"""
    tr = _trainer(dev, "bf16")
    assert tr.bprec.npass == 1
    return tr


@pytest.fixture(scope="module")
def tr3(dev):
    """three-product backward"""
    tr = _trainer(dev, "parity")
    assert tr.bprec.npass == 3
    return tr


def _reset(tr):
    from stedm_amd import ops
    tr._dpacks.clear()
    tr._dpacks_step.clear()
    tr._dplan = ops.PackPlan(tr.bprec)
    tr.G.clear()


@contextlib.contextmanager
def _trace():
    """records (name, args, kwargs) of every traced ops.* call made inside the block, and calls through"""
    from stedm_amd import ops
    calls, saved = [], {n: getattr(ops, n) for n in TRACED}

    def wrap(n, f):
        def g(*a, **k):
            calls.append((n, a, k))
            return f(*a, **k)
        return g

    for n, f in saved.items():
        setattr(ops, n, wrap(n, f))
    try:
        yield calls
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)


def _names(calls):
    return [n for n, _, _ in calls]


def _conv_branch(calls):
    """(rs, lazy, materialised) of the first convolution of a traced call: the capability query on the call's own arguments. Lazy hi planes
    must have been packed exactly when the register-streamed kernel does not run."""
    from stedm_amd import ops
    assert ops.device_cus() == CUS, f"the branch expectations of this file are those of a {CUS}-CU device, this one has {ops.device_cus()}"
    convs = [c for c in calls if c[0] == "conv_igemm"]
    _, a, k = next((c for c in convs if isinstance(c[1][1], ops.LazyPlanes)), convs[0])     # the dgrad convolution, where a weight-gradient GEMM ran too
    lazy = isinstance(a[1], ops.LazyPlanes)
    mat = a[1]._val is not None if lazy else None
    rs = bool(ops.conv_igemm(*a, **dict(k, query_rs=True)))
    assert not lazy or mat == (not rs), f"lazy planes materialised: {mat}, register-streamed kernel admitted: {rs}"
    return rs, lazy, mat


def _where(bad):
    i = bad.nonzero()
    return f"{int(bad.sum())} of {bad.numel()} elements differ, first at {i[0].tolist()}, last at {i[-1].tolist()}"


def _exact(out, ref, what=""):
    bad = out.double() != ref
    assert not bool(bad.any()), f"{what}: " + _where(bad)
    assert torch.equal(out.double(), ref)


def _planes(x32, parity, tier):
    hi, lo = R.split16(x32, BF)
    if tier == 1:
        assert torch.equal(hi.float(), x32) and not bool(lo.float().any())
    return (hi.view(torch.int16), lo.view(torch.int16) if parity else None), hi.double(), (lo.double() if parity else None)


def _ratio(name, what, out, ref, S):
    assert bool(torch.isfinite(out).all()), "output elements left unwritten"
    g = (out.double() - ref).abs() / (U * S)
    print(f"\n  MEASURED {name:24s} {what:8s} max err / (u S) = {float(g.max()):.3f}", end="")
    bad = g > G
    assert not bool(bad.any()), f"max err / (u S) = {float(g.max()):.3f} > G = {G}: " + _where(bad)


_CACHE = {}          # one entry: the operands and the reference of the case at hand, shared by the runs of that case


def _cached(key, make):
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


# ================================================================================================ _dgrad
def dcase(name, B, H, W, cin, cout, ks=3, pack="frag", rs=False, t2=False, pad_cin=0, pad_cout=0, acc=False, ws=False, data=None):
    """forward convolution cin -> cout on a B x H x W grid; pack: what _dpack builds ('frag' | 'frag16' | 'planes'); rs: what the capability
    query says on a 256-CU device; ws: the K split must have written the workspace; data: the case whose inputs it shares"""
    return pytest.param(SimpleNamespace(name=name, B=B, H=H, W=W, cin=cin, cout=cout, ks=ks, pack=pack, rs=rs, t2=t2, pad_cin=pad_cin, pad_cout=pad_cout,
                                        acc=acc, ws=ws, data=data or name), id=name)


SWEEP_B = (1, 3, 4, 5, 63, 64, 65, 128, 129, 257)
DGRAD = [
    dcase("d_frag_rs", 25, 32, 32, 32, 64, t2=True),                       # 100 tiles, 4 chunks: declined (see the module docstring)
    dcase("d_frag_rs_full", 48, 32, 32, 32, 64, rs=True, t2=True),         # 192 tiles: the register-streamed kernel on a full grid
    dcase("d_frag_lds", 3, 8, 8, 32, 64, rs=True, t2=True, ws=True),       # one tile: register-streamed with a 4-way K split
    dcase("d_frag_lds_declined", 129, 8, 8, 32, 64, t2=True),              # 33 tiles: the query declines, planes materialised
] + [dcase(f"d_sweep_b{B}", B, 8, 8, 32, 64, rs=B <= 128, ws=B <= 128) for B in SWEEP_B] + [
    dcase("d_m16", 97, 16, 16, 64, 288, pack="frag16", t2=True),
    dcase("d_m16_small", 2, 8, 8, 128, 256, pack="frag16", rs=True, t2=True, ws=True),
    dcase("d_m16_full", 769, 8, 8, 32, 256, pack="frag16", rs=True, t2=True),
    dcase("d_1x1_frag", 493, 10, 10, 96, 64, ks=1, rs=True),
    dcase("d_1x1_planes", 3, 4, 4, 64, 96, ks=1, pack="planes"),
    dcase("d_splitk", 2, 8, 8, 64, 1024, pack="frag16", rs=True, t2=True, ws=True),
    dcase("d_splitk_acc", 2, 8, 8, 64, 1024, pack="frag16", rs=True, t2=True, ws=True, acc=True, data="d_splitk"),
    dcase("d_pad_out", 3, 16, 16, 64, 4, pack="planes", pad_cin=32),
    dcase("d_pad_in", 3, 16, 16, 7, 32, pack="planes", pad_cout=32),
]
DGRAD_PARITY = [     # hi / lo planes, no fragments: the LDS-operand three-product kernel
    dcase("d_parity_frag_lds", 3, 8, 8, 32, 64, pack="planes", t2=True),
    dcase("d_parity_m16_small", 2, 8, 8, 128, 256, pack="planes"),
    dcase("d_parity_pad_in", 3, 16, 16, 7, 32, pack="planes", pad_cout=32),
]
_DBY = {p.values[0].name: p.values[0] for p in DGRAD + DGRAD_PARITY}


def _dgrad_operands(dev, c, tier):
    """dy fp32 [B, H, W, cout (padded to pad_cin)], w OIHW, prior [B, H, W, cin (padded to pad_cout)] or None, on the device"""
    def make():
        seed = R.case_seed(c.data)
        if tier == 1:
            dy, w = R.dyadic((c.B, c.H, c.W, c.cout), seed), R.dyadic((c.cout, c.cin, c.ks, c.ks), seed + 1)
            prior = R.dyadic((c.B, c.H, c.W, c.cin), seed + 2) if c.acc else None
        else:
            dy, w = R.dgrad_t2_inputs(c.data, (c.B, c.H, c.W, c.cin, c.cout, c.ks))
            prior = R.t2_grad((c.B, c.H, c.W, c.cin), seed + 2) if c.acc else None
        if c.pad_cin:        # the last convolution's gradient, padded to pad_cin channels with zeros
            dy = torch.cat([dy, dy.new_zeros((c.B, c.H, c.W, c.pad_cin - c.cout))], -1)
        return SimpleNamespace(dy=dy.to(dev), w=w.to(dev), prior=None if prior is None else prior.to(dev))
    return _cached((c.data, c.acc, tier), make)


def _dgrad_ref(c, o, dyh, dyl, wh, wl):
    """the fp64 input gradient (+ prior), zero in the channels a padded filter adds"""
    ref = R.dgrad_ref(dyh[..., :c.cout], wh) if dyl is None else RC.three_products(dyh[..., :c.cout], dyl[..., :c.cout], wh, wl, R.dgrad_ref)
    if c.pad_cout:
        ref = torch.cat([ref, ref.new_zeros((c.B, c.H, c.W, c.pad_cout - c.cin))], -1)
    return ref if o.prior is None else ref + o.prior.double()


def _run_dgrad(tr, dev, c, tier, holder=None):
    """two identical _dgrad calls into NaN-filled (or prior-filled) outputs; the branch of the first is asserted and printed"""
    _reset(tr)
    o = _dgrad_operands(dev, c, tier)
    parity = tr.bprec.npass == 3
    dy16, dyh, dyl = _planes(o.dy, parity, tier)
    holder = holder if holder is not None else SimpleNamespace(weight=o.w)
    outs = []
    for rep in range(2):
        out = o.prior.clone() if c.acc else torch.full((c.B, c.H, c.W, c.pad_cout or c.cin), NAN, device=dev)
        ws = tr._ws(out.numel())
        ws.fill_(NAN)
        with _trace() as calls:
            got = tr._dgrad(holder, dy16, out, accumulate=c.acc, pad_cin=c.pad_cin, pad_cout=c.pad_cout)
        assert got is out
        outs.append(out)
        if rep:
            continue
        n, a, k = next(x for x in calls if x[0] == "conv_igemm")
        kind = "frag16" if k["w_frag16"] is not None else ("frag" if k["w_frag"] is not None else "planes")
        rs, lazy, mat = _conv_branch(calls)
        assert (k["res"] is out) == c.acc, "an accumulating dgrad adds onto its own output: the residual is the output tensor"
        assert k["ws"] is ws
        print(f"\n  BRANCH {c.name:22s} npass {tr.bprec.npass} pack {kind:6s} lazy {lazy} materialised {mat} register-streamed {rs} "
              f"workspace written {not bool(torch.isnan(ws).all())} calls {_names(calls)}", end="")
        assert kind == c.pack and lazy == (kind != "planes") and rs == c.rs
        assert not c.ws or not bool(torch.isnan(ws).all()), "the K split did not run: the workspace is untouched"
    torch.cuda.synchronize()
    return o, outs, dyh, dyl


def _dgrad_bit_exact(tr, dev, c):
    R.backward_dyadic_ok(c.ks * c.ks * c.cout + (1 if c.acc else 0))
    o = _dgrad_operands(dev, c, 1)
    if not hasattr(o, "ref"):
        o.ref = _dgrad_ref(c, o, o.dy.double(), None, o.w.double(), None)
        assert bool((o.ref * 64 == (o.ref * 64).round()).all()) and float(o.ref.abs().max()) * 64 < 2 ** 24
    _, outs, _, _ = _run_dgrad(tr, dev, c, 1)
    _exact(outs[0], o.ref, c.name)
    assert torch.equal(outs[1], outs[0]), "the second run differs from the first"
    if c.pad_cout:
        assert not bool(outs[0][..., c.cin:].any()), "the channels a padded filter adds must be exactly zero"


def _read_back_oihw(tr, w):
    """the weights the dgrad convolution multiplies: the hi (/ lo) planes of the pack _dpack makes, [cin][taps reversed][cout], back as OIHW fp64"""
    from stedm_amd import ops
    co, ci, ks, _ = w.shape
    taps = ks * ks
    hi, lo, _ = ops.pack_conv_weight_strided(w, taps, ci * taps, True, ci, co, ks, tr.bprec, want_hi=True, want_frag=False)
    un = lambda p: None if p is None else RC.as_f64(p, "bf16").flip(1).permute(2, 0, 1).reshape(co, ci, ks, ks)
    return un(hi), un(lo)


def _dgrad_operand_exact(tr, dev, c):
    o, outs, dyh, dyl = _run_dgrad(tr, dev, c, 2)
    wh, wl = _read_back_oihw(tr, o.w)
    ref = _dgrad_ref(c, o, dyh, dyl, wh, wl)
    S = R.dgrad_ref(dyh.abs() if dyl is None else dyh.abs() + dyl.abs(), wh.abs() if wl is None else wh.abs() + wl.abs())
    if o.prior is not None:
        S = S + o.prior.double().abs()
    _ratio(c.name, f"npass {tr.bprec.npass}", outs[0], ref, S)
    assert torch.equal(outs[1], outs[0]), "the second run differs from the first"


@pytest.mark.parametrize("c", DGRAD)
def test_dgrad_bit_exact_on_dyadic_operands(dev, tr1, c):
    _dgrad_bit_exact(tr1, dev, c)


@pytest.mark.parametrize("c", DGRAD_PARITY)
def test_dgrad_bit_exact_three_products(dev, tr3, c):
    _dgrad_bit_exact(tr3, dev, c)


@pytest.mark.parametrize("c", [p for p in DGRAD if p.values[0].t2])
def test_dgrad_operand_exact(dev, tr1, c):
    _dgrad_operand_exact(tr1, dev, c)


@pytest.mark.parametrize("c", [p for p in DGRAD_PARITY if p.values[0].t2])
def test_dgrad_operand_exact_three_products(dev, tr3, c):
    _dgrad_operand_exact(tr3, dev, c)


@pytest.mark.parametrize("name", ["d_frag_rs", "d_frag_rs_full", "d_frag_lds", "d_m16_small"])
def test_dgrad_plan_route_equals_holder_route(dev, tr1, name):
    """a plain holder with a .weight is packed for this step only (_dpacks_step); an nn.Conv2d whose parameter is the filter goes through
    the persistent PackPlan (_dpacks). Same bits, and both the exact gradient."""
    c = _DBY[name]
    o = _dgrad_operands(dev, c, 1)
    _, held, _, _ = _run_dgrad(tr1, dev, c, 1)
    assert len(tr1._dpacks_step) == 1 and not tr1._dpacks and not tr1._dplan.items
    conv = nn.Conv2d(c.cin, c.cout, c.ks, padding=c.ks // 2).to(dev)
    conv.weight.copy_(o.w)
    _, planned, _, _ = _run_dgrad(tr1, dev, c, 1, holder=conv)
    assert id(conv) in tr1._dpacks and not tr1._dpacks_step and len(tr1._dplan.items) == 1, "the persistent-plan route was expected"
    assert torch.equal(planned[0], held[0]) and torch.equal(planned[1], held[0])
    _exact(planned[0], _dgrad_ref(c, o, o.dy.double(), None, o.w.double(), None), name)


# ================================================================================================ _wgrad
def wcase(name, B, H, W, cin, cout, ks=3, mode=0, f32=True, kind="gemm", nsplit=0, chunks=1, frag=True, launches=1, t2=False, flags=None, data=None):
    """source plane [B, H, W, cin], gradient on the convolution's output grid. kind: 'direct' | 'direct_t' (transposing reduce) | '1x1' |
    'gemm'; nsplit: what the direct kernel's plan must say; chunks / frag / launches: batch chunks of the GEMM form, whether each builds
    the fragment-order dY^T, GEMM launches per chunk; flags: trainer attributes set for the call"""
    return pytest.param(SimpleNamespace(name=name, B=B, H=H, W=W, cin=cin, cout=cout, ks=ks, mode=mode, f32=f32, kind=kind, nsplit=nsplit, chunks=chunks,
                                        frag=frag, launches=launches, t2=t2, flags=flags or {}, data=data or name), id=name)


WGRAD = [
    wcase("w_direct_1", 3, 8, 8, 128, 64, kind="direct", nsplit=1),
    wcase("w_direct_n8", 8, 8, 8, 128, 64, kind="direct", nsplit=2),
    wcase("w_direct_n8_t", 8, 8, 8, 128, 64, kind="direct_t", nsplit=2, flags=dict(wgrad_oihw=False), data="w_direct_n8"),
    wcase("w_direct_n", 2, 32, 32, 128, 64, kind="direct", nsplit=8, t2=True),
    wcase("w_direct_n_t", 2, 32, 32, 128, 64, kind="direct_t", nsplit=8, t2=True, flags=dict(wgrad_oihw=False), data="w_direct_n"),
    wcase("w_1x1", 1, 64, 64, 128, 128, ks=1, kind="1x1", nsplit=16),
    wcase("w_1x1_gemm", 1, 64, 64, 128, 128, ks=1, flags=dict(direct_wgrad1=False), data="w_1x1"),
    wcase("w_gemm_frag", 2, 8, 8, 64, 96, t2=True),
    wcase("w_gemm_nofrag", 2, 8, 8, 64, 96, f32=False, frag=False, data="w_gemm_frag"),
    wcase("w_gemm_nofrag_ragged", 3, 10, 10, 64, 96, frag=False),                      # P = 300, Ppad = 320
    wcase("w_mode1", 2, 6, 6, 64, 96, mode=1, frag=False),                              # dy 12 x 12: P = 288, Ppad = 320
    wcase("w_mode2", 2, 16, 16, 64, 64, mode=2),                                        # dy 8 x 8: P = 128
    wcase("w_chunks", 5, 128, 128, 32, 32, chunks=2, t2=True),                          # Bc = 4: 4 + 1 samples
    wcase("w_chunks_mode2_9", 9, 128, 128, 32, 32, mode=2),                             # dy 64 x 64: Bc = 16, one chunk (see the module docstring)
    wcase("w_chunks_mode2", 17, 128, 128, 32, 32, mode=2, chunks=2),                    # 16 + 1 samples
    wcase("w_launch_split", 1, 8, 8, 1024, 1024, launches=2, flags=dict(direct_wgrad=False)),
]
WGRAD_PARITY = [
    wcase("w_parity_nofrag", 2, 8, 8, 64, 96, frag=False, t2=True),
    wcase("w_parity_nofrag_ragged", 3, 10, 10, 64, 96, frag=False, t2=True),
    wcase("w_parity_mode2", 2, 16, 16, 64, 64, mode=2, frag=False, t2=True),
]


def _wgrad_operands(dev, c, tier):
    def make():
        Ho, Wo = R.wgrad_out_hw(c.H, c.W, c.mode)
        if tier == 1:
            seed = R.case_seed(c.data)
            src, dy = R.dyadic((c.B, c.H, c.W, c.cin), seed), R.dyadic((c.B, Ho, Wo, c.cout), seed + 1)
        else:
            src, dy = R.wgrad_t2_inputs(c.data, (c.B, c.H, c.W, c.cin, c.cout, c.ks, c.mode))
        return SimpleNamespace(src=src.to(dev), dy=dy.to(dev))
    return _cached((c.data, tier), make)


def _expected_wgrad_calls(tr, c):
    if c.kind == "direct":
        return ["wgrad3x3_oihw"] + (["sum_planes"] if c.nsplit > 1 else [])
    if c.kind == "direct_t":
        return ["wgrad3x3", "wgrad_to_oihw"]
    if c.kind == "1x1":
        return ["wgrad1x1", "wgrad_to_oihw"]
    one = ["im2col_t16"] * (4 if tr.bprec.npass == 3 else 2) + (["pack_conv_weight_strided"] if c.frag else []) + ["conv_igemm"] * c.launches + ["wgrad_to_oihw"]
    return one * c.chunks


def _run_wgrad(tr, dev, c, tier):
    from stedm_amd import ops
    _reset(tr)
    o = _wgrad_operands(dev, c, tier)
    parity = tr.bprec.npass == 3
    src16, sh, sl = _planes(o.src, parity, tier)
    dy16, dh, dl = _planes(o.dy, parity, tier)
    Ho, Wo = dy16[0].shape[1:3]
    saved = {k: getattr(tr, k) for k in c.flags}
    outs = []
    try:
        for k, v in c.flags.items():
            setattr(tr, k, v)
        for rep in range(2):
            grad = torch.full((c.cout, c.cin, c.ks, c.ks), NAN, device=dev)
            with _trace() as calls:
                tr._wgrad(src16, dy16, o.dy if c.f32 else None, None, c.ks, c.mode, grad=grad)
            outs.append(grad)
            if rep:
                continue
            assert ops.device_cus() == CUS
            names = _names(calls)
            plan3 = ops.wgrad3x3_plan(c.B, c.H, c.W, c.cin, c.cout) if c.ks == 3 and c.mode == 0 else 0
            plan1 = ops.wgrad1x1_plan(c.B * c.H * c.W, c.cin, c.cout) if c.ks == 1 else 0
            acc = [a[4] for n, a, k in calls if n == "wgrad_to_oihw"]
            rs = [bool(ops.conv_igemm(*a, **dict(k, query_rs=True))) for n, a, k in calls if n == "conv_igemm"]
            print(f"\n  BRANCH {c.name:22s} npass {tr.bprec.npass} wgrad3x3_plan {plan3} wgrad1x1_plan {plan1} calls {names} accumulate {acc} "
                  f"GEMM register-streamed {rs}", end="")
            assert names == _expected_wgrad_calls(tr, c), (names, _expected_wgrad_calls(tr, c))
            if c.kind in ("direct", "direct_t"):
                assert plan3 == c.nsplit
            elif c.kind == "1x1":
                assert plan1 == c.nsplit
            else:
                Bc = max(1, 65536 // (Ho * Wo))
                assert (c.B + Bc - 1) // Bc == c.chunks and acc == [False] + [True] * (c.chunks - 1), "batch chunks accumulate after the first"
                assert c.chunks == 1 or c.B % Bc != 0, "a chunked case ends on a ragged chunk"
                assert parity or not tr.direct_wgrad or c.mode != 0 or not (plan3 if c.ks == 3 else plan1 and tr.direct_wgrad1)
            if c.launches == 2:
                # the tile-count-aware launch split, computed as _wgrad_gemm does: rows of dW that fill whole rounds of the chip first
                rows, cus = c.ks * c.ks * c.cin, ops.device_cus()
                tm, tn = (rows + 255) // 256, (c.cout + 127) // 128
                total = tm * tn
                m_full = (total // cus) * cus // tn
                assert total > cus and 0 < total % cus < 0.6 * cus and 0 < m_full < tm, (total, cus, m_full, tm)
                shapes = [tuple(a[3].shape) for n, a, k in calls if n == "conv_igemm"]
                assert shapes == [(1, m_full * 256, 1, c.cout), (1, rows - m_full * 256, 1, c.cout)], shapes
    finally:
        for k, v in saved.items():
            setattr(tr, k, v)
    torch.cuda.synchronize()
    return o, outs, (sh, sl, dh, dl)


def _wgrad_bit_exact(tr, dev, c):
    Ho, Wo = R.wgrad_out_hw(c.H, c.W, c.mode)
    R.backward_dyadic_ok(c.B * Ho * Wo)
    o = _wgrad_operands(dev, c, 1)
    if not hasattr(o, "ref"):
        o.ref = R.wgrad_ref(o.src.double(), o.dy.double(), c.ks, c.mode)
        assert bool((o.ref * 64 == (o.ref * 64).round()).all()) and float(o.ref.abs().max()) * 64 < 2 ** 24
    _, outs, _ = _run_wgrad(tr, dev, c, 1)
    assert not bool(torch.isnan(outs[0]).any()), "gradient elements left unwritten"
    _exact(outs[0], o.ref, c.name)
    assert torch.equal(outs[1], outs[0]), "the second run differs from the first"


def _wgrad_operand_exact(tr, dev, c):
    o, outs, (sh, sl, dh, dl) = _run_wgrad(tr, dev, c, 2)
    fn = lambda s_, d_: R.wgrad_ref(s_, d_, c.ks, c.mode)
    if sl is None:
        ref, S = fn(sh, dh), fn(sh.abs(), dh.abs())
    else:
        ref, S = RC.three_products(sh, sl, dh, dl, fn), fn(sh.abs() + sl.abs(), dh.abs() + dl.abs())
    _ratio(c.name, f"npass {tr.bprec.npass}", outs[0], ref, S)
    assert torch.equal(outs[1], outs[0]), "the second run differs from the first"


@pytest.mark.parametrize("c", WGRAD)
def test_wgrad_bit_exact_on_dyadic_operands(dev, tr1, c):
    _wgrad_bit_exact(tr1, dev, c)


@pytest.mark.parametrize("c", WGRAD_PARITY)
def test_wgrad_bit_exact_three_products(dev, tr3, c):
    _wgrad_bit_exact(tr3, dev, c)


@pytest.mark.parametrize("c", [p for p in WGRAD if p.values[0].t2])
def test_wgrad_operand_exact(dev, tr1, c):
    _wgrad_operand_exact(tr1, dev, c)


@pytest.mark.parametrize("c", [p for p in WGRAD_PARITY if p.values[0].t2])
def test_wgrad_operand_exact_three_products(dev, tr3, c):
    _wgrad_operand_exact(tr3, dev, c)


# ================================================================================================ _up_bwd / _down_bwd on the trainer's own layers
def _layer_case(tr, dev, layer, conv, B, hw, up, seed):
    """dyadic filter into the layer's own convolution, dyadic input, output gradient and prior; the three fp64 gradients"""
    C, co = conv.in_channels, conv.out_channels
    ho = 2 * hw if up else hw // 2
    w = R.dyadic((co, C, 3, 3), seed).to(dev)
    conv.weight.copy_(w)
    hin, dout, prior = R.dyadic((B, hw, hw, C), seed + 1).to(dev), R.dyadic((B, ho, ho, co), seed + 2).to(dev), R.dyadic((B, hw, hw, C), seed + 3).to(dev)
    R.backward_dyadic_ok(B * max(ho, hw) ** 2)                  # weight and bias gradient: a sum over all output pixels
    R.backward_dyadic_ok((4 if up else 1) * 9 * co + 1)         # input gradient: taps x cout (x 4 pixels of the 2 x 2 sum) + the prior
    d64 = dout.double()
    dx = R.sum2x2(R.dgrad_ref(d64, w.double())) if up else R.dgrad_ref(R.zero_insert(d64), w.double())
    return SimpleNamespace(hin=hin, dout=dout, prior=prior, out=torch.empty((B, ho, ho, co), device=dev), dw=R.wgrad_ref(hin.double(), d64, 3, 1 if up else 2),
                           db=R.bias_ref(d64), dx=dx)


def _run_layer(tr, fn, layer, conv, s, with_prior):
    """one _up_bwd / _down_bwd call: dout registered as the gradient of `out`, the input's gradient buffer NaN-filled and unregistered
    (acc False) or holding the prior (acc True); the parameters' gradients NaN-filled in the arena"""
    _reset(tr)
    tr.G[s.out.data_ptr()] = s.dout
    g = tr._buf(f"g.{s.hin.data_ptr()}", tuple(s.hin.shape))
    if with_prior:
        g.copy_(s.prior)
        tr.G[s.hin.data_ptr()] = g
    else:
        g.fill_(NAN)
    conv.weight.grad.fill_(NAN)
    conv.bias.grad.fill_(NAN)
    with _trace() as calls:
        fn(layer, s.hin, s.out)
    assert tr.G[s.hin.data_ptr()] is g
    torch.cuda.synchronize()
    return g, calls


def _check_layer(s, conv, g, with_prior, what):
    _exact(conv.weight.grad, s.dw, what + " weight gradient")
    _exact(conv.bias.grad, s.db, what + " bias gradient")
    _exact(g, s.dx + s.prior.double() if with_prior else s.dx, what + " input gradient")


@pytest.mark.parametrize("hw,direct", [(4, True), (6, False)])
def test_up_bwd_bit_exact(dev, tr1, hw, direct):
    """the TINY U-Net's Upsample at 128 channels. 4 x 4 -> 8 x 8: the direct weight-gradient kernel over the materialised nearest-2x plane;
    6 x 6 -> 12 x 12: the plan declines, the mode-1 GEMM form runs (and the dgrad convolution takes the im2col form: 12 x 12 has no tiling)"""
    from stedm_amd import ops
    from stedm_amd.unet import Upsample
    layer = next(m for m in tr1.m.modules() if isinstance(m, Upsample) and m.channels == 128)
    B, C, co = 3, 128, layer.conv.out_channels
    s = _layer_case(tr1, dev, layer, layer.conv, B, hw, True, 4100 + hw)
    assert (ops.wgrad3x3_plan(B, 2 * hw, 2 * hw, C, co) > 0) == direct and tr1.direct_wgrad
    for with_prior in (False, True):
        first = None
        for rep in range(2):
            g, calls = _run_layer(tr1, tr1._up_bwd, layer, layer.conv, s, with_prior)
            names = _names(calls)
            if rep == 0:
                rs, lazy, mat = _conv_branch(calls)
                print(f"\n  BRANCH up {hw}x{hw} prior {with_prior}: direct {direct} dgrad register-streamed {rs} lazy {lazy} materialised {mat} calls {names}", end="")
            if direct:
                assert "im2col_t16" not in names and names.count("wgrad3x3_oihw") == 1
            else:
                assert "wgrad3x3_oihw" not in names and [a[3] for n, a, k in calls if n == "im2col_t16"] == [1, 0], "mode-1 im2col of the source, plain of dy"
            assert [a[2] for n, a, k in calls if n == "sum2x2"] == [with_prior], "the 2 x 2 sum accumulates exactly when the input already has a gradient"
            _check_layer(s, layer.conv, g, with_prior, f"up {hw}x{hw} prior {with_prior}")
            first = g.clone() if rep == 0 else first
            assert torch.equal(g, first), "the second run differs from the first"


@pytest.mark.parametrize("channels", [32, 64])
def test_down_bwd_bit_exact(dev, tr1, channels):
    """the TINY U-Net's Downsample layers, 16 x 16 -> 8 x 8: mode-2 GEMM weight gradient, dgrad over the zero-inserted gradient, accumulated in
    place onto a prior input gradient (the residual of the convolution IS its output)"""
    from stedm_amd.unet import Downsample
    layer = next(m for m in tr1.m.modules() if isinstance(m, Downsample) and m.channels == channels)
    s = _layer_case(tr1, dev, layer, layer.op, 3, 16, False, 4200 + channels)
    for with_prior in (False, True):
        first = None
        for rep in range(2):
            g, calls = _run_layer(tr1, tr1._down_bwd, layer, layer.op, s, with_prior)
            names = _names(calls)
            convs = [(a, k) for n, a, k in calls if n == "conv_igemm"]
            if rep == 0:
                rs, lazy, mat = _conv_branch([c for c in calls if c[0] == "conv_igemm"][-1:])
                print(f"\n  BRANCH down {channels} prior {with_prior}: dgrad register-streamed {rs} lazy {lazy} materialised {mat} calls {names}", end="")
            assert names.count("zero_insert16") == 1 and [a[3] for n, a, k in calls if n == "im2col_t16"] == [2, 0], "mode-2 im2col of the source, plain of dy"
            a, k = convs[-1]                       # the dgrad convolution (after the weight-gradient GEMM)
            assert a[3] is g and (k["res"] is g) == with_prior, "accumulate exactly when the input already has a gradient, onto the output itself"
            _check_layer(s, layer.op, g, with_prior, f"down {channels} prior {with_prior}")
            first = g.clone() if rep == 0 else first
            assert torch.equal(g, first), "the second run differs from the first"


# ================================================================================================ bad arguments
def test_wgrad_rejects_mismatched_planes(dev, tr1):
    """source and gradient planes over different pixel grids: the direct kernel's argument check raises before any launch"""
    from stedm_amd import ops
    _reset(tr1)
    src = torch.zeros((3, 8, 8, 128), dtype=torch.int16, device=dev)
    dy = torch.zeros((3, 8, 4, 64), dtype=torch.int16, device=dev)
    assert ops.wgrad3x3_plan(3, 8, 8, 128, 64) == 1 and tr1.direct_wgrad and tr1.wgrad_oihw
    grad = torch.full((64, 128, 3, 3), NAN, device=dev)
    with _trace() as calls, pytest.raises(AssertionError):
        tr1._wgrad((src, None), (dy, None), None, None, 3, 0, grad=grad)
    torch.cuda.synchronize()
    assert _names(calls) == ["wgrad3x3_oihw"] and bool(torch.isnan(grad).all()), "the gradient must be left untouched"


def test_dgrad_planes_only_3x3_pack_is_refused_by_the_kernels(dev, tr1):
    """d_planes_3x3, (3, 8, 8; 32 -> 40; 3): 40 forward output channels are no multiple of 16, so _dpack builds the planes only - and no
    convolution kernel contracts over 40 channels (conv_setup: multiples of 32). Every multiple of 32 is a multiple of 16: in the single-product
    backward the planes-only 3x3 branch of _dpack leads to this error and nowhere else. Asserted: the pack kind, the error, the untouched output."""
    from stedm_amd import _lib, ops
    _reset(tr1)
    holder = SimpleNamespace(weight=R.dyadic((40, 32, 3, 3), 7).to(dev))
    hi, lo, frag, ks, frag16 = tr1._dpack(holder)
    assert not isinstance(hi, ops.LazyPlanes) and tuple(hi.shape) == (32, 9, 40) and lo is None and frag is None and frag16 is None and ks == 3
    dy16, _, _ = _planes(R.dyadic((3, 8, 8, 40), 8).to(dev), False, 1)
    out = torch.full((3, 8, 8, 32), NAN, device=dev)
    with pytest.raises(_lib.StedmHipError, match="multiples of 32"):
        tr1._dgrad(holder, dy16, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "the output must be left untouched"


def test_dgrad_rejects_mismatched_channels(dev, tr1):
    """a gradient plane whose channel count is not the filter's forward output channels: conv_igemm's shape check of the weight planes
    raises before the convolution is launched (a planes-only pack: the check reads the planes' shape)"""
    _reset(tr1)
    holder = SimpleNamespace(weight=R.dyadic((40, 32, 3, 3), 7).to(dev))
    dy = torch.zeros((3, 8, 8, 48), dtype=torch.int16, device=dev)
    out = torch.full((3, 8, 8, 32), NAN, device=dev)
    with pytest.raises(AssertionError):
        tr1._dgrad(holder, (dy, None), out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "the output must be left untouched"
