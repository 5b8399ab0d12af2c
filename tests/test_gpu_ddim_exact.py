"""GPU tier (-m gpu): the three DDIM entries (stedm_ddim_step, stedm_ddim_step_ex, stedm_ddim_step_rows) against the exact restatement
of tests/refs_ddim.py, bit for bit (torch.equal) on x_prev, pred_x0 and, through _ex, eps_out and noise_out. One shape for every
instantiation of ddim_step_kernel that the dispatchers can select, at its smallest:

  scalar entries (DdimScalarForm: one workgroup per sample, parts = 256 / W)
    (2,4,16,16)    R = 4
    (2,4,16,32)    R = 8
    (2,4,32,32)    R = 16
    (2,3,40,40)    looped, 256 % W != 0, idle threads
    (2,3,8,8)      looped, parts 24 .. 31 own no row
    (1,3,128,128)  looped, the native latent
  per-row entry (DdimRowsForm: a workgroup per sample and 16 columns, 16 parts, R by ceil(C H / 16); scales cycle 1, 3, 5, 1.5, 7.5 so that
  a scale-1 row sits between guided ones; a one-sample shape, whose cycle is [1], also runs at scale 3)
    (5,4,8,8)      R = 2, W < 16
    (2,4,12,24)    R = 4, ragged rows, a tail chunk
    (2,3,40,40)    R = 8, ragged
    (1,4,64,20)    R = 16
    (1,3,128,128)  R = 24
    (1,4,100,20)   looped
The restatement was fitted to the library of the commit before the five hand-copied kernels became one (every case here passed against it),
so these tests say that the merge moved no bit.
Per shape: the table row at eta = 1 and at eta = 0; unguided (e_u None) and guided (scale 1.5 for the scalar entries); the noise absent,
given, and drawn in the kernel (which must equal the given form fed ops.philox_normal's rows). Through _ex every case runs twice: plain
(<DRAW, false>: the noise joins by one fma) and with eps_out / noise_out (<DRAW, true>: every product of the noise term rounded), and on
one register shape and one looped shape with temperature 0.7 and dropout 0.25."""
import pytest
import torch

from oracle import ddim as od
from stedm_amd.utils import prng
from tests import refs_ddim as rd
from tests.test_ddim_options_oracle import drop_scale, keep_mask

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SCALAR_SHAPES = [(2, 4, 16, 16), (2, 4, 16, 32), (2, 4, 32, 32), (2, 3, 40, 40), (2, 3, 8, 8), (1, 3, 128, 128)]
ROWS_SHAPES = [(5, 4, 8, 8), (2, 4, 12, 24), (2, 3, 40, 40), (1, 4, 64, 20), (1, 3, 128, 128), (1, 4, 100, 20)]
CYCLE = [1.0, 3.0, 5.0, 1.5, 7.5]
N, IDX, SEED, ID0 = 20, 10, 1234, 5
ITER = N - 1 - IDX


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def operands(dev):
    """shape -> (x, e_c, e_u, given noise, the kernel's own draw) on the CPU and on the device, made once and left unchanged"""
    from stedm_amd import ops
    cache = {}

    def get(shape):
        if shape not in cache:
            x = prng.normal(7, "dd.x", shape)
            ec = prng.normal(7, "dd.ec", shape)
            eu = prng.normal(7, "dd.eu", shape) * 0.8 + 0.1 * ec
            nz = prng.normal(7, "dd.nz", shape)
            zd = ops.philox_normal(shape[0], shape[1:], SEED, 1 + ITER, dev, first_id=ID0)
            cpu = (x, ec, eu, nz, zd.cpu())
            cache[shape] = cpu, tuple(t.to(dev) for t in cpu)
        return cache[shape]
    return get


def _table(dev, eta):
    ds = od.DDIMSchedule(od.Schedule(), N, eta)
    return ds.scalars(IDX), torch.tensor([ds.scalars(i) for i in range(N)], dtype=torch.float32, device=dev)


def _same(got, want, what):
    for g, w, nm in zip(got, want, ("x_prev", "pred_x0", "eps_out", "noise_out")):
        g = g.cpu()
        assert torch.equal(g, w), (what, nm, int((g != w).sum()), float((g - w).abs().max()))


def _noise_term(row, z, T=1.0, ks=None):
    """what noise_out holds: ((sigma z) T) ks, every product rounded"""
    nz = (torch.tensor(row[2]) * z) * T
    return nz if ks is None else nz * ks


@pytest.mark.parametrize("eta", [1.0, 0.0])
@pytest.mark.parametrize("shape", SCALAR_SHAPES)
def test_ddim_step_and_ex_equal_the_restatement(dev, operands, shape, eta):
    from stedm_amd import ops
    (x, ec, eu, nz, zd), (xd, ecd, eud, nzd, zdd) = operands(shape)
    row, tab = _table(dev, eta)
    step = torch.tensor([IDX], dtype=torch.int32, device=dev)
    form = rd.scalar_form(shape[1] * shape[2], shape[3])
    new = lambda: torch.empty(shape, device=dev)
    for e_u, e_ud in ((None, None), (eu, eud)):
        for z, zdev, how in ((None, None, "none"), (nz, nzd, "given"), (zd, zdd, "drawn")):
            what = (shape, eta, e_u is not None, how)
            xp, x0, e = rd.ddim_step_ref(x, ec, e_u, row, 1.5, form, noise=z)
            kw = dict(draw=True, seed=SEED, first_id=ID0) if how == "drawn" else dict(noise=zdev)
            if how != "drawn":
                g, g0 = new(), new()
                ops.ddim_step(xd, ecd, e_ud, tab, g, pred_x0=g0, noise=zdev, step_idx=step, cfg_scale=1.5)
                _same((g, g0), (xp, x0), what + ("step",))
            g, g0 = new(), new()
            ops.ddim_step_ex(xd, ecd, e_ud, tab, g, pred_x0=g0, step_idx=step, n_iters=N, cfg_scale=1.5, **kw)
            _same((g, g0), (xp, x0), what + ("ex",))
            # with the optional outputs: the options path, its noise term rounded before it is added
            xq, _, _ = rd.ddim_step_ref(x, ec, e_u, row, 1.5, form, noise=z, ext=dict(temperature=1.0))
            g, g0, ge, gn = new(), new(), new(), new().fill_(float("nan"))
            ops.ddim_step_ex(xd, ecd, e_ud, tab, g, pred_x0=g0, step_idx=step, n_iters=N, cfg_scale=1.5, eps_out=ge, noise_out=gn, **kw)
            _same((g, g0, ge) + (() if z is None else (gn,)), (xq, x0, e) + (() if z is None else (_noise_term(row, z),)), what + ("ex+outs",))


@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (2, 3, 40, 40)])              # R = 4; looped
def test_ddim_step_ex_temperature_and_dropout_equal_the_restatement(dev, operands, shape):
    from stedm_amd import ops
    (x, ec, eu, nz, zd), (xd, ecd, eud, nzd, zdd) = operands(shape)
    row, tab = _table(dev, 1.0)
    step = torch.tensor([IDX], dtype=torch.int32, device=dev)
    form = rd.scalar_form(shape[1] * shape[2], shape[3])
    T, p = 0.7, 0.25
    B, n = shape[0], shape[1] * shape[2] * shape[3]
    keep = torch.from_numpy(keep_mask(SEED, range(ID0, ID0 + B), n, ITER, p)).view(shape)
    ks = keep.float() * drop_scale(p)
    for e_u, e_ud in ((None, None), (eu, eud)):
        for z, kw, how in ((nz, dict(noise=nzd), "given"), (zd, dict(draw=True), "drawn")):
            xp, x0, e = rd.ddim_step_ref(x, ec, e_u, row, 1.5, form, noise=z, ext=dict(temperature=T, ks=ks))
            g, g0, ge, gn = (torch.empty(shape, device=dev) for _ in range(4))
            ops.ddim_step_ex(xd, ecd, e_ud, tab, g, pred_x0=g0, step_idx=step, n_iters=N, cfg_scale=1.5, temperature=T, noise_dropout=p,
                             seed=SEED, first_id=ID0, eps_out=ge, noise_out=gn, **kw)
            _same((g, g0, ge, gn), (xp, x0, e, _noise_term(row, z, T, ks)), (shape, e_u is not None, how))
            g2 = torch.empty(shape, device=dev)                                    # the same without the optional outputs
            ops.ddim_step_ex(xd, ecd, e_ud, tab, g2, step_idx=step, n_iters=N, cfg_scale=1.5, temperature=T, noise_dropout=p, seed=SEED,
                             first_id=ID0, **kw)
            assert torch.equal(g2, g)


@pytest.mark.parametrize("eta", [1.0, 0.0])
@pytest.mark.parametrize("shape", ROWS_SHAPES)
def test_ddim_step_rows_equals_the_restatement(dev, operands, shape, eta):
    from stedm_amd import ops
    (x, ec, eu, nz, zd), (xd, ecd, eud, nzd, zdd) = operands(shape)
    row, tab = _table(dev, eta)
    step = torch.tensor([IDX], dtype=torch.int32, device=dev)
    cycle = [CYCLE[b % 5] for b in range(shape[0])]
    for scales in [cycle] + ([[3.0]] if shape[0] == 1 else []):                  # one sample: the cycle is [1], so a guided run besides
        sc = torch.tensor(scales, dtype=torch.float32, device=dev)
        for e_u, e_ud in ((None, None), (eu, eud)):
            for z, kw, how in ((None, {}, "none"), (nz, dict(noise=nzd), "given"),
                               (zd, dict(draw=True, n_iters=N, seed=SEED, first_id=ID0), "drawn")):
                xp, x0, _ = rd.ddim_step_ref(x, ec, e_u, row, scales, rd.ROWS, noise=z)
                g, g0 = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
                ops.ddim_step_rows(xd, ecd, e_ud, tab, g, sc, pred_x0=g0, step_idx=step, **kw)
                _same((g, g0), (xp, x0), (shape, eta, scales, e_u is not None, how))


@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (2, 3, 40, 40)])              # a register form and a looped form of the scalar entries
def test_x_prev_may_be_x_and_eps_out_may_be_e_c(dev, operands, shape):
    """the aliasing the samplers use: StepGraph.step_eager steps img in place, DDIMSampler._update takes the guided eps back into e_c"""
    from stedm_amd import ops
    _, (xd, ecd, eud, nzd, _) = operands(shape)
    _, tab = _table(dev, 1.0)
    step = torch.tensor([IDX], dtype=torch.int32, device=dev)
    sc = torch.tensor([3.0, 1.5], dtype=torch.float32, device=dev)
    ref, ref_e = torch.empty_like(xd), torch.empty_like(xd)
    ops.ddim_step_ex(xd, ecd, eud, tab, ref, noise=nzd, step_idx=step, n_iters=N, cfg_scale=1.5, eps_out=ref_e)
    xa, ea = xd.clone(), ecd.clone()
    ops.ddim_step_ex(xa, ea, eud, tab, xa, noise=nzd, step_idx=step, n_iters=N, cfg_scale=1.5, eps_out=ea)
    assert torch.equal(xa, ref) and torch.equal(ea, ref_e)
    ref = torch.empty_like(xd)
    ops.ddim_step(xd, ecd, eud, tab, ref, noise=nzd, step_idx=step, cfg_scale=1.5)
    xa = xd.clone()
    ops.ddim_step(xa, ecd, eud, tab, xa, noise=nzd, step_idx=step, cfg_scale=1.5)
    assert torch.equal(xa, ref)
    ref = torch.empty_like(xd)
    ops.ddim_step_rows(xd, ecd, eud, tab, ref, sc, noise=nzd, step_idx=step)
    xa = xd.clone()
    ops.ddim_step_rows(xa, ecd, eud, tab, xa, sc, noise=nzd, step_idx=step)
    assert torch.equal(xa, ref)


def test_ddim_step_rejects_a_wrong_shaped_operand(dev, operands):
    from stedm_amd import ops
    _, (xd, ecd, eud, nzd, _) = operands((2, 4, 16, 16))
    _, tab = _table(dev, 1.0)
    bad = torch.empty((2, 4, 16, 8), device=dev)
    for kw in (dict(e_u=bad), dict(e_u=eud, noise=bad), dict(e_u=eud, pred_x0=bad), dict(e_u=eud, x_prev=bad)):
        args = dict(e_u=None, x_prev=torch.empty_like(xd))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.ddim_step(xd, ecd, args.pop("e_u"), tab, args.pop("x_prev"), **args)
