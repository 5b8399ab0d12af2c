"""GPU tier (-m gpu): the HIP U-Net with train-mode dropout in its ResBlocks (UNetModel(dropout=0.1), openaimodel.py:241, :473) against
fixtures the reference itself produced on the CPU with the project's counter-based masks in place of torch's generator
(tests/golden/make_golden_dropout.py: TINY, B = 2, 16 x 16, seed 6, t = [951, 21], plain and use_scale_shift_norm) - the training forward,
the backward, the step counter eager and captured - and the unchanged routes: eval() and dropout = 0.

Thresholds: the ones this net has without dropout (test_gpu_unet.py / test_gpu_unet_film.py: 1e-3 parity, 6e-3 f16, 5e-2 bf16, max
error / std; the f29 gradient bounds). The measured errors are printed and recorded in DESIGN.md section 4.4."""
import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests.golden.make_golden_grads import pick_index
from tests.golden.summary import check_summary

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
B, HW, SEED = 2, 16, 6
MODE_TOL = {"parity": 1e-3, "f16": 6e-3, "bf16": 5e-2}
FORMS = [pytest.param(False, id="plain"), pytest.param(True, id="film")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(dev, precision="parity", film=False, dropout=0.1, train=True):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, use_scale_shift_norm=film, dropout=dropout, **TINY)
    m.train(train)
    prng.fill_module_(m, seed=SEED)
    return m.to(dev)


def inputs(dev, film=False):
    src = "film_tiny" if film else "tiny"
    x = prng.normal(SEED, f"unet.{src}.x", (B, 7, HW, HW)).to(dev)
    ctx = prng.normal(SEED, f"unet.{src}.ctx", (B, 128)).to(dev)
    target = prng.normal(SEED, f"unet.{src}.target", (B, 4, HW, HW)).to(dev)
    return x, ctx, target


def split(x):
    return x[:, :4].contiguous(), x[:, 4:].contiguous()


def rel(a, b):
    a = a.double().cpu(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max()) / (float(b.std()) + 1e-12)


def seeded(m, fx):
    """put the model at the fixture's (seed, step): the next training forward advances the counter onto drop_step"""
    m.dropout_seed = int(fx["drop_seed"])
    m.set_dropout_step(int(fx["drop_step"]) - 1)


# ------------------------------------------------------------------------------------------------ unchanged routes
@pytest.mark.parametrize("precision", ["parity", "f16", "bf16"])
def test_eval_with_dropout_equals_the_model_without(dev, precision):
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = split(x)
    outs = []
    for dropout in (0.0, 0.1):
        m = build(dev, precision, dropout=dropout, train=False)
        y = m(x, t, context=ctx).clone()
        e_c, e_u = [v.clone() for v in m.forward_cfg(xl, cc, t, ctx, ctx_u)]
        outs.append((y, e_c, e_u))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("precision", ["parity", "bf16"])
def test_zero_dropout_in_train_mode_takes_the_existing_route(dev, precision):
    """dropout = 0 in train() is not live: the training forward and the gradients carry the bits of the eval() model, and of a
    dropout = 0.1 model in eval()"""
    from stedm_amd.train import UNetTrainer
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    runs = []
    for dropout, train in ((0.0, True), (0.0, False), (0.1, False)):
        m = build(dev, precision, dropout=dropout, train=train)
        assert not m.dropout_live()
        tr = UNetTrainer(m)
        y = tr.forward(*split(x), t, ctx).clone()
        tr.loss_and_backward(*split(x), t, ctx, target)
        assert m.last_dropout is None and m._drop_ctr is None
        runs.append([y] + [p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))


def test_live_model_refuses_inference_before_any_launch(dev):
    m = build(dev)
    x, ctx, _ = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    key = m._pack_key
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m(x, t, context=ctx)
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m.forward_cfg(*split(x), t, ctx, ctx)
    assert m._pack_key == key and not m._packed, "nothing may have been packed or launched"
    m.eval()
    assert bool(torch.isfinite(m(x, t, context=ctx)).all())


# ------------------------------------------------------------------------------------------------ against the reference's fixtures
@pytest.mark.parametrize("film", FORMS)
@pytest.mark.parametrize("precision", ["parity", "f16", "bf16"])
def test_training_forward_vs_reference_golden(dev, golden, precision, film):
    from stedm_amd.train import UNetTrainer
    fx = golden("f30_unet_dropout_film_tiny" if film else "f30_unet_dropout_tiny")
    m = build(dev, precision, film)
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    seeded(m, fx)
    x, ctx, _ = inputs(dev, film)
    y = UNetTrainer(m).forward(*split(x), torch.from_numpy(fx["t"]).to(dev), ctx)
    m.check_f16_range()
    assert m.last_dropout == (int(fx["drop_seed"]), int(fx["drop_step"]))
    err = rel(y, fx["y"])
    print(f"[dropout tiny film={film} {precision}] max err / std vs reference golden: {err:.3e} (threshold {MODE_TOL[precision]:.0e})")
    assert err < MODE_TOL[precision]


def _check_grads(m, fx, tol, what):
    """the checks of tests/test_gpu_train.py::_check_grads"""
    worst = (0.0, "")
    nmax = max(float(fx[f"g.{name}.norm"]) for name, _ in m.named_parameters())
    for name, p in m.named_parameters():
        assert p.grad is not None, f"{name}: no gradient"
        n = float(fx[f"g.{name}.norm"])
        a = p.grad.double().reshape(-1).cpu()
        if n < 1e-6 * nmax:
            assert float(a.norm()) < 1e-5 * nmax, f"{what} {name}: expected a vanishing gradient"
            continue
        en = abs(float(a.norm()) - n) / (n + 1e-30)
        rms = n / np.sqrt(a.numel())
        ep = float(np.abs(a[torch.from_numpy(pick_index(a.numel()))].numpy() - fx[f"g.{name}.pick"]).max()) / (rms + 1e-30)
        worst = max(worst, (en, name + " (norm)"), (ep / 30, name + " (samples)"))
        assert en <= tol, f"{what} {name}: grad norm off by {en:.2e}"
        assert ep <= 30 * tol, f"{what} {name}: sampled grad entries off by {ep:.2e} of the tensor's rms"
    return worst


@pytest.mark.parametrize("film", FORMS)
def test_backward_vs_reference_golden(dev, golden, film):
    from stedm_amd.train import UNetTrainer
    tag = "dropout_film_tiny" if film else "dropout_tiny"
    fx = golden(f"f30_grads_{tag}")
    m = build(dev, "parity", film)
    tr = UNetTrainer(m)
    x, ctx, target = inputs(dev, film)
    t = torch.from_numpy(fx["t"]).to(dev)
    seeded(m, fx)
    loss, dx, dctx = tr.loss_and_backward(*split(x), t, ctx, target)
    assert m.last_dropout == (int(fx["drop_seed"]), int(fx["drop_step"]))
    ref_c = torch.from_numpy(fx["dctx"]).double()
    err_c = float((dctx.double().cpu() - ref_c).norm() / ref_c.norm())
    err_l = abs(float(loss) - float(fx["loss"])) / float(fx["loss"])
    print(f"[{tag}] loss {float(loss):.6f} (rel {err_l:.2e})  dctx rel-L2 {err_c:.2e}")
    assert err_l < 1e-4
    check_summary(dx, fx, "dx", 2e-3, tag)
    worst = _check_grads(m, fx, 1e-3, tag)
    print(f"[{tag}] worst param grad {worst[0]:.2e} at {worst[1]}")
    assert err_c < 1e-3
    # the same (seed, step) set by hand gives the same bits
    g1 = [p.grad.clone() for p in m.parameters()]
    seeded(m, fx)
    tr.loss_and_backward(*split(x), t, ctx, target)
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, m.parameters()))


# ------------------------------------------------------------------------------------------------ the counter
@pytest.mark.parametrize("precision", ["parity", "bf16"])
def test_every_training_forward_draws_fresh_masks_from_one_seed(dev, precision):
    from stedm_amd.train import UNetTrainer
    m = build(dev, precision)
    tr = UNetTrainer(m)
    x, ctx, _ = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    torch.manual_seed(1234)
    y1 = tr.forward(*split(x), t, ctx).clone()
    seed, step = m.last_dropout
    assert step == 1 and m.dropout_seed == seed, "the seed is drawn once, the first forward runs at step 1"
    y2 = tr.forward(*split(x), t, ctx).clone()
    assert m.last_dropout == (seed, 2) and int(m._drop_ctr.item()) == 2
    assert not torch.equal(y1, y2), "two training forwards must drop different elements"
    m.set_dropout_step(0)
    y3 = tr.forward(*split(x), t, ctx).clone()
    assert m.last_dropout == (seed, 1) and torch.equal(y1, y3)
    # torch.manual_seed governs a seed that was not given
    m2 = build(dev, precision)
    torch.manual_seed(1234)
    y4 = UNetTrainer(m2).forward(*split(x), t, ctx)
    assert m2.last_dropout == (seed, 1) and torch.equal(y1, y4)


def test_captured_train_step_advances_the_mask_counter(dev):
    """train_step_graphed with live dropout: GRAPH_WARMUP eager steps, then the captured step replayed three times, a different batch each,
    against train_step() on a second copy - losses and parameters bit for bit, which needs every replay to run at its own step; the host
    mirror equals the device word."""
    from stedm_amd.train import UNetTrainer
    runs = []
    nsteps = UNetTrainer.GRAPH_WARMUP + 3
    for graphed in (True, False):
        m = build(dev, "bf16")
        m.dropout_seed = 0xD0D0CAFE
        tr = UNetTrainer(m, lr=2e-4, weight_decay=0.01)
        losses = []
        for step in range(nsteps):
            x = prng.normal(SEED + step, f"unet.drop.cap{step}.x", (B, 7, HW, HW)).to(dev)
            ctx = prng.normal(SEED + step, f"unet.drop.cap{step}.ctx", (B, 128)).to(dev)
            target = prng.normal(SEED + step, f"unet.drop.cap{step}.target", (B, 4, HW, HW)).to(dev)
            t = torch.tensor([951 - 7 * step, 21 + step], device=dev)
            a = (*split(x), t, ctx, target)
            losses.append(float(tr.train_step_graphed(*a) if graphed else tr.train_step(*a)))
        torch.cuda.synchronize()
        if graphed:
            assert tr._graph is not None and tr.step_count == nsteps
        assert m._drop_step == nsteps == int(m._drop_ctr.item()) and m.last_dropout == (0xD0D0CAFE, nsteps)
        runs.append((losses, [p.detach().clone() for p in m.parameters()]))
    (la, pa), (lb, pb) = runs
    print("losses", ["%.5f" % v for v in la])
    assert la == lb, (la, lb)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))


def test_train_steps_with_dropout_reduce_the_loss(dev):
    from stedm_amd.train import UNetTrainer
    m = build(dev, "bf16")
    m.dropout_seed = 99
    tr = UNetTrainer(m, lr=2e-4, weight_decay=0.0)
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    losses = [float(tr.train_step(*split(x), t, ctx, target)) for _ in range(30)]
    print("losses", ["%.4f" % v for v in losses[::5]], "last", "%.4f" % losses[-1])
    # fresh masks make single steps noisy: the mean of the last five against the first
    assert sum(losses[-5:]) / 5 < losses[0] - 0.01
