"""GPU tier (-m gpu): the small kernels of the style encoder's backward (csrc/svit_bwd.hip) - gelu_bwd, svit_head_bwd, svit_tok_bwd,
svit_patch_gather, widen16 - each against its torch restatement (tests/refs_svit_bwd.py) at the shapes of the f34 fixture plus one with
dim = 256.

  exact: the gather, the widening and the fixed-order batch sums (d pos_embedding, d cls_token, the head's d bias), where the restatement
         sums in the kernel's order (ascending b, fp32): torch.equal.
  gelu_bwd: |error| <= 1e-6 |dh| per element against fp64 - erff within 2 ulp of a value <= 1, halved (1.2e-7); x phi(x) <= 0.25 with the
         hardware exp within 2 ulp and its argument x^2 / 2 <= 18 rounded once (3e-7); three roundings of a result <= 1.13 (2e-7).
  svit_head_bwd: max-abs error over max-abs reference per tensor <= 8 x the same figure of the fp32 restatement against the fp64 one
         (the largest of the case's tensors): reference against reference, the factor for a different but fixed summation order."""
import pytest
import torch

from tests import refs_svit_bwd as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(2, 6, 64, 32, "mean"), (1, 66, 64, 32, "cls"), (3, 10, 256, 512, "mean"), (2, 10, 256, 40, "cls")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _n(name, shape, std=1.0):
    from stedm_amd.utils import prng
    return prng.normal(35, name, shape, std=std)


@pytest.mark.parametrize("n", [2 * 6 * 64, 66 * 128, 5 * 256 * 257 + 3])
def test_gelu_bwd(dev, n):
    from stedm_amd import ops
    pre, dh = _n(f"gelu.pre.{n}", (n,), 2.0), _n(f"gelu.dh.{n}", (n,))
    pre[:4] = torch.tensor([0.0, -6.0, 6.0, -0.75])
    out = torch.full((n,), float("nan"), device=dev)
    ops.gelu_bwd(pre.to(dev), dh.to(dev), out)
    ref = dh.double() * R.gelu_grad(pre.double())
    err = (out.cpu().double() - ref).abs()
    bound = 1e-6 * dh.double().abs() + 1e-30
    print(f"gelu_bwd n={n}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    dh_d = dh.to(dev)
    ops.gelu_bwd(pre.to(dev), dh_d, dh_d)                  # in place (the backward's use)
    assert torch.equal(dh_d, out)


@pytest.mark.parametrize("img,ns,B", [(16, 2, 2), (64, 1, 1), (24, 3, 2)])
def test_patch_gather_exact(dev, img, ns, B):
    from stedm_amd import ops
    x = _n(f"gather.{img}.{ns}", (B, ns, img, img, 3))
    n, pd = (img // 8) ** 2, 64 * 3 * ns
    rows = torch.full((B * n, pd), float("nan"), device=dev)
    ops.svit_patch_gather(x.to(dev), rows, 8)
    assert torch.equal(rows.cpu(), R.patch_rows(x, 8).reshape(B * n, pd))


@pytest.mark.parametrize("mode", ["f16", "bf16", "parity"])
def test_widen16_exact(dev, mode):
    from stedm_amd import ops
    prec = ops.Precision.parse(mode)
    x = _n(f"widen.{mode}", (37, 64)).to(dev)
    dt = torch.float16 if mode != "bf16" else torch.bfloat16
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt) if prec.npass == 3 else None
    out = torch.full((37, 64), float("nan"), device=dev)
    ops.widen16(hi.view(torch.int16), None if lo is None else lo.view(torch.int16), out, prec)
    assert torch.equal(out, hi.float() + (lo.float() if lo is not None else 0.0))


@pytest.mark.parametrize("B,T,dim", [(2, 6, 64), (1, 66, 64), (3, 10, 256)])
def test_tok_bwd_exact(dev, B, T, dim):
    from stedm_amd import ops
    dx = _n(f"tok.{B}.{T}.{dim}", (B, T, dim))
    nan = float("nan")
    dpos, dcls, dtok = torch.full((T, dim), nan, device=dev), torch.full((dim,), nan, device=dev), torch.full((B * (T - 2), dim), nan, device=dev)
    ops.svit_tok_bwd(dx.to(dev), dpos, dcls, dtok)
    rp, rc, rt = R.tok_bwd(dx)
    assert torch.equal(dpos.cpu(), rp) and torch.equal(dcls.cpu(), rc) and torch.equal(dtok.cpu(), rt)
    ops.svit_tok_bwd(dx.to(dev), dpos, dcls, dtok, accumulate=True)          # added onto the tensors
    assert torch.equal(dpos.cpu(), rp + rp) and torch.equal(dcls.cpu(), rc + rc) and torch.equal(dtok.cpu(), rt)


@pytest.mark.parametrize("B,T,dim,ncls,pool", SHAPES)
def test_head_bwd(dev, B, T, dim, ncls, pool):
    from stedm_amd import ops
    tag = f"head.{B}.{T}.{dim}.{pool}"
    x, d_out = _n(tag + ".x", (B, T, dim)), _n(tag + ".g", (B, ncls))
    ln_w, ln_b = 1.0 + _n(tag + ".lw", (dim,), 0.1), _n(tag + ".lb", (dim,), 0.1)
    w = _n(tag + ".w", (ncls, dim), dim ** -0.5)
    ref = R.head_bwd(x.double(), pool, ln_w.double(), ln_b.double(), w.double(), d_out.double())
    r32 = R.head_bwd(x, pool, ln_w, ln_b, w, d_out)
    figure = max(R.rel_err(a, b) for a, b in zip(r32, ref))
    bound = 8.0 * figure
    nan = float("nan")
    mk = lambda shp: torch.full(shp, nan, device=dev)
    dx, dg, db, dw, dbias = mk((B, T, dim)), mk((dim,)), mk((dim,)), mk((ncls, dim)), mk((ncls,))
    args = (x.to(dev), {"mean": 0, "cls": 1}[pool], ln_w.to(dev), ln_b.to(dev), 1e-5, w.to(dev), d_out.to(dev), dx, dg, db, dw, dbias)
    ops.svit_head_bwd(*args)
    got = [t.cpu() for t in (dx, dg, db, dw, dbias)]
    errs = [R.rel_err(a, b) for a, b in zip(got, ref)]
    print(f"svit_head_bwd {tag}: errors " + " ".join(f"{e:.2e}" for e in errs) + f" | bound {bound:.2e}")
    assert all(e <= bound for e in errs), (errs, bound)
    s = torch.zeros(ncls)
    for b in range(B):
        s = s + d_out[b]
    assert torch.equal(got[4], s)                                            # fixed-order batch sum
    if pool == "cls":
        assert bool((got[0][:, 1:] == 0).all())
    ops.svit_head_bwd(*args, accumulate=True)                                # parameter gradients doubled bit for bit, dx rewritten
    for t, g0 in zip((dg, db, dw, dbias), got[1:]):
        assert torch.equal(t.cpu(), g0 + g0)
    assert torch.equal(dx.cpu(), got[0])
