"""GPU tier (-m gpu): stedm_avgpool2x2 / stedm_replicate2x2 (stedm_amd/csrc/resample.hip) against the restatements of tests/refs_resample.py,
exactly. The inputs are small dyadic values (multiples of 1/8, magnitude <= 2): every sum of four, its quarter, every square and every sum
of a sample's squares is exact in fp32 whatever the order of additions, so outputs, per-slot statistics and slot-folded statistics are
compared bit for bit - no tolerance is involved. Sentinels around every output buffer must stay untouched.

Shapes (the high-resolution side for the pool, the input for the replicate): the smallest that reach each edge - one output row pair;
odd batch, non-square, C not a power of two; a 256-pixel slot boundary with a ragged last slot (pool 40 x 32 -> 320 output pixels,
replicate 10 x 16 -> 640); C = 4 (one quad, 256 pixel lanes) and C = 1024 (several channel blocks) at 4 x 4; C = 36: a last channel
block of one quad."""
import pytest
import torch

from tests import refs_resample as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD = 64           # sentinel floats on either side of a buffer (256 B: the payload stays 16-byte aligned)
SENT = 12345.0
POOL_SHAPES = [(2, 4, 4, 32), (3, 6, 10, 96), (2, 40, 32, 36), (1, 4, 4, 4), (2, 4, 4, 1024)]
REP_SHAPES = [(2, 4, 4, 32), (3, 6, 10, 96), (2, 10, 16, 36), (1, 4, 4, 4), (2, 4, 4, 1024)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def guarded(dev, shape, fill=None):
    """(flat buffer with sentinels, the payload view of `shape`), the payload filled with NaN or with the tensor `fill`"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * PAD,), SENT, device=dev)
    v = flat[PAD:PAD + n].view(shape)
    if fill is not None:
        v.copy_(fill.to(dev))
    else:
        v.fill_(float("nan"))
    return flat, v


def sentinels_ok(flat):
    return bool((flat[:PAD] == SENT).all()) and bool((flat[-PAD:] == SENT).all())


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("stats", [True, False])
def test_avgpool2x2_exact(dev, shape, stats):
    from stedm_amd import ops
    B, H, W, C = shape
    g = torch.Generator().manual_seed(11)
    x = R.dyadic(g, shape)
    ref = R.avgpool2x2(x)
    assert torch.equal(ref.double(), R.avgpool2x2(x.double())), "the inputs are exact in fp32"
    fo, out = guarded(dev, (B, H // 2, W // 2, C))
    ns = ops.gn_chan_nslab((H // 2) * (W // 2))
    assert ns == R.nslab(H // 2, W // 2)
    fc, cs = guarded(dev, (B, ns, C, 2))
    ops.avgpool2x2(x.to(dev), out, cs if stats else None)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)
    assert sentinels_ok(fo) and sentinels_ok(fc)
    if stats:
        want = R.chan_stats(ref, R.pool_slots(H // 2, W // 2), ns)
        assert torch.equal(cs.cpu().double(), want), "per-slot statistics"
        assert torch.equal(R.fold(cs.cpu().double()), R.fold(want))
        # ... and they are what the separate pass gives for the same tensor
        cs2 = torch.empty_like(cs)
        ops.gn_chan_stats(out, cs2)
        assert torch.equal(cs2, cs)
    else:
        assert bool(torch.isnan(cs).all()), "no statistics asked: none written"


@pytest.mark.parametrize("shape", REP_SHAPES)
@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("accumulate", [False, True])
def test_replicate2x2_exact(dev, shape, scale, accumulate):
    from stedm_amd import ops
    B, H, W, C = shape
    g = torch.Generator().manual_seed(12)
    x = R.dyadic(g, shape)
    prior = R.dyadic(g, (B, 2 * H, 2 * W, C)) if accumulate else None
    ref = R.replicate2x2(x, scale, prior)
    assert torch.equal(ref.double(), R.replicate2x2(x.double(), scale, None if prior is None else prior.double()))
    fo, out = guarded(dev, (B, 2 * H, 2 * W, C), prior)
    ns = ops.gn_chan_nslab(4 * H * W)
    assert ns == R.nslab(2 * H, 2 * W)
    fc, cs = guarded(dev, (B, ns, C, 2))
    stats = not accumulate              # (the statistics are those of scale * in: accumulate = 0 only)
    ops.replicate2x2(x.to(dev), out, scale, accumulate, cs if stats else None)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)
    assert sentinels_ok(fo) and sentinels_ok(fc)
    if stats:
        want = R.chan_stats(ref, R.replicate_slots(H, W), ns)
        assert torch.equal(cs.cpu().double(), want), "per-slot statistics"
        assert torch.equal(R.fold(cs.cpu().double()), R.fold(want))
        cs2 = torch.empty_like(cs)
        ops.gn_chan_stats(out, cs2)      # (another partition - runs of 256 output pixels: equal once folded)
        assert torch.equal(R.fold(cs2.cpu().double()), R.fold(want))
    else:
        assert bool(torch.isnan(cs).all())


def test_pool_then_quarter_replicate_onto_a_prior_gradient(dev):
    """replicate2x2(avgpool2x2(x), 0.25, accumulate) onto a gradient that is already there, the form UNetTrainer._down_bwd uses"""
    from stedm_amd import ops
    g = torch.Generator().manual_seed(13)
    x = R.dyadic(g, (2, 8, 12, 16))
    prior = R.dyadic(g, (2, 8, 12, 16))
    out = torch.empty((2, 4, 6, 16), device=dev)
    ops.avgpool2x2(x.to(dev), out)
    gbuf = prior.clone().to(dev)
    ops.replicate2x2(out, gbuf, 0.25, True)
    assert torch.equal(gbuf.cpu(), R.replicate2x2(R.avgpool2x2(x), 0.25, prior))


def test_argument_errors_raise_before_any_launch(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError

    def f(*s):
        return torch.full(s, SENT, device=dev)
    for H, W in ((5, 4), (4, 7)):
        out = f(1, H // 2, W // 2, 8)
        with pytest.raises(StedmHipError, match="even"):
            ops.avgpool2x2(f(1, H, W, 8), out)
        torch.cuda.synchronize()
        assert bool((out == SENT).all())
    with pytest.raises(StedmHipError, match="C %"):
        ops.avgpool2x2(f(1, 4, 4, 6), f(1, 2, 2, 6))
    with pytest.raises(StedmHipError, match="C %"):
        ops.replicate2x2(f(1, 2, 2, 6), f(1, 4, 4, 6))
    out = f(1, 4, 4, 8)
    with pytest.raises(StedmHipError, match="accumulate"):
        ops.replicate2x2(f(1, 2, 2, 8), out, 1.0, True, f(1, 1, 8, 2))
    with pytest.raises(AssertionError):          # a statistics buffer of another slot count never reaches the library
        ops.avgpool2x2(f(1, 4, 4, 8), f(1, 2, 2, 8), f(1, 2, 8, 2))
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
