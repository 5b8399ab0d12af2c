"""GPU tier of the full training objective (ddpm.py:1015-1048): the loss kernel (stedm_diffusion_loss) against tests/refs_objective.py and
the reference's own p_losses (fixture F24), and the training surface that runs on it (p_losses_backward, training_step_hip eager and
graphed, a learned logvar in the optimizer, the autograd bridge). Outputs are filled with NaN before every launch."""
import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests import refs_objective as ro
from tests.refs_bwd import dyadic, normal
from tests.test_gpu_train import TINY, _check_grads, _inputs, build
from tests.test_objective_cpu import CASES, check_against_f24, f24_case

pytestmark = pytest.mark.gpu

T = 1000
F24_T = [0, 999, 417, 417]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables():
    """(logvar, lvlb) fp32 [T] on the CPU: a logvar of both signs, the STEDM schedule's lvlb_weights"""
    from stedm_amd.schedule import lvlb_weights
    return normal((T,), 24, "logvar", std=0.5), torch.from_numpy(lvlb_weights(T, 0.0015, 0.0205))


def second_trip_n():
    """an n past blocks * 256 at the block cap: every block's stride loop goes round more than once, some threads once more than others"""
    from stedm_amd import ops
    cap = ops.diffusion_loss_blocks(1 << 40)
    n = cap * 1024 + 259
    assert ops.diffusion_loss_blocks(n) == cap and n > 2 * cap * 256
    return n


def launch(dev, pred, target, t, logvar, lvlb, kind, lsw, ew, gs=1.0, want_dpred=True, want_dlogvar=True):
    from stedm_amd import ops
    nan = float("nan")
    B = pred.shape[0]
    n = pred.numel() // B
    dp = torch.full(tuple(pred.shape), nan, device=dev) if want_dpred else None
    dl = torch.full((logvar.numel(),), nan, device=dev) if want_dlogvar else None
    ws = torch.full((ops.diffusion_loss_ws_doubles(B, n),), nan, dtype=torch.float64, device=dev)
    out = torch.full((4,), nan, device=dev)
    ops.diffusion_loss(pred.to(dev), target.to(dev), t.to(dev), logvar.to(dev), lvlb.to(dev), kind, lsw, ew, gs, dp, dl, ws, out)
    torch.cuda.synchronize()
    return out.cpu(), None if dp is None else dp.cpu(), None if dl is None else dl.cpu()


def kernel_shapes():
    return [(1, 1, [417]), (3, 105, [417, 0, 417]), (4, 1024, F24_T), (4, 120, F24_T), (2, None, [999, 999])]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("B,n,t", kernel_shapes())
def test_loss_kernel_on_dyadic_inputs(dev, tables, kind, B, n, t):
    n = second_trip_n() if n is None else n
    logvar, lvlb = tables
    t = torch.tensor(t, dtype=torch.long)
    pred, target = dyadic((B, n), 100 + n % 97), dyadic((B, n), 200 + n % 97)
    target[:, 0] = pred[:, 0] + 0.125                   # every sample has a nonzero difference ...
    if n > 1:
        target[:, 1] = pred[:, 1]                        # ... and a zero one
    lsw, ew = 0.75, 0.5
    d = (pred - target).double()
    base = None
    for gs in (1.0, 0.25):
        r = ro.objective(pred, target, t, logvar, lvlb, kind, lsw, ew, gs)
        out, dp, dl = launch(dev, pred, target, t, logvar, lvlb, kind, lsw, ew, gs)
        for i, name in enumerate(ro.SCALARS):
            err, bound = abs(float(out[i]) - float(r[name])), ro.scalar_bound(r, name, ro.K_KERNEL)
            print(f"kind {kind} ({B}, {n}) gs {gs} {name}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, name
        if base is None:
            base = out
        assert torch.equal(out, base)                   # grad_scale does not touch the scalars
        assert bool((dp[d == 0] == 0).all()) and bool(torch.isfinite(dp).all())
        if kind == 0:
            for b in range(B):
                nz = d[b] != 0
                cb = (dp[b][nz].double() * torch.sign(d[b][nz])).unique()
                assert cb.numel() == 1, "l1: |d_pred| is one value per sample"
                ulp = float(np.spacing(np.float32(abs(float(r["c"][b])))))
                assert abs(float(cb) - float(r["c"][b])) <= ulp, (b, float(cb), float(r["c"][b]))
        else:
            assert bool(((dp.double() - r["d_pred"]).abs() <= ro.d_pred_bound(r, ro.K_KERNEL_DPRED)).all())
        named = torch.zeros(T, dtype=torch.bool)
        named[t] = True
        assert bool((dl[~named] == 0).all()) and bool((dl[named] != 0).all())
        assert bool(((dl.double() - r["d_logvar"]).abs() <= ro.d_logvar_bound(r, ro.K_KERNEL)).all())
        # each gradient output is optional and leaves the rest as it was
        for wp, wl in ((False, True), (True, False), (False, False)):
            o2, dp2, dl2 = launch(dev, pred, target, t, logvar, lvlb, kind, lsw, ew, gs, wp, wl)
            assert torch.equal(o2, out) and (dp2 is None or torch.equal(dp2, dp)) and (dl2 is None or torch.equal(dl2, dl))


def test_loss_kernel_sums_the_duplicate_timestep(dev, tables):
    """d_logvar at a timestep two samples share is the sum of what each alone gives (dyadic data, a logvar of 0: every term is exact)."""
    logvar, lvlb = torch.zeros(T), tables[1]
    pred, target = dyadic((4, 120), 7), dyadic((4, 120), 8)
    t = torch.tensor(F24_T)
    _, _, dl = launch(dev, pred, target, t, logvar, lvlb, 1, 1.0, 0.0)
    ls = ((pred - target).double() ** 2).mean(1)
    f32 = lambda v: float(np.float32(float(v)))
    assert float(dl[417]) == f32(0.25 * ((1 - ls[2]) + (1 - ls[3])))
    assert float(dl[0]) == f32(0.25 * (1 - ls[0])) and float(dl[999]) == f32(0.25 * (1 - ls[1]))


@pytest.mark.parametrize("name", CASES)
def test_f24_cases_through_the_kernel(dev, golden, name):
    c = f24_case(golden, name)
    out, dp, dl = launch(dev, c["model_output"], c["target"], c["t"], c["logvar"], c["lvlb"], c["kind"], c["lsw"], c["ew"])
    got = {"loss": out[0].double(), "loss_simple": out[1].double(), "loss_gamma": out[2].double(), "loss_vlb": out[3].double(),
           "d_pred": dp.double(), "d_logvar": dl.double()}
    check_against_f24(c, got, ro.k_ref(120, 4) + ro.K_KERNEL, ro.K_REF_DPRED + ro.K_KERNEL_DPRED)


@pytest.mark.parametrize("kind", [0, 1])
def test_loss_kernel_is_bitwise_reproducible(dev, tables, kind):
    logvar, lvlb = tables
    pred, target = normal((6, 4, 33, 31), 3, "p"), normal((6, 4, 33, 31), 3, "q")
    t = torch.tensor([417, 3, 417, 417, 999, 3])
    a = launch(dev, pred, target, t, logvar, lvlb, kind, 0.9, 0.3)
    b = launch(dev, pred, target, t, logvar, lvlb, kind, 0.9, 0.3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the training surface
def _ld(dev, seed=6, **kw):
    from stedm_amd.latent_diffusion import LatentDiffusion
    unet = build(TINY, seed, dev)
    ld = LatentDiffusion(unet, linear_start=0.0015, linear_end=0.0205, image_size=16, channels=4, conditioning_key="hybrid", **kw).to(dev)
    return ld, unet


def _batch(dev, tag, seed=6, t=(417, 417)):
    x, ctx, noise = _inputs(tag, TINY, 2, 16, seed, dev)
    cond = {"c_concat": [x[:, 4:].contiguous()], "c_crossattn": [ctx]}
    return x[:, :4].contiguous(), cond, torch.tensor(t, device=dev), noise


def _oracle_cfg():
    from oracle import unet as ounet
    ocfg = ounet.UNetConfig(image_size=16, in_channels=7, model_channels=32, out_channels=4, channel_mult=(1, 2, 4), num_heads=4)
    return ocfg, prng.fill_state_dict(ounet.build_plan(ocfg).shapes, 6)


def test_objective_backward_end_to_end_vs_oracle(dev):
    """p_losses_backward with l2 + the VLB term + a nonzero logvar against autograd over the oracle's forward with the objective restated in
    refs_objective; measures and tolerances of test_unet_backward_vs_reference_golden's tiny case (loss 1e-4, parameter gradients 1e-3,
    dx 2e-3, dcontext 1e-3)."""
    from tests.golden.make_golden_grads import pick_index
    from tests.golden.summary import check_summary, summarize
    kw = dict(loss_type="l2", original_elbo_weight=0.5, logvar_init=-0.7)
    ld, unet = _ld(dev, **kw)
    x0, cond, t, noise = _batch(dev, "tiny", t=(951, 21))
    loss, ldict, dx, dctx = ld.p_losses_backward(x0, cond, t, noise)
    assert ld._trainer.last_loss_terms is not None and set(ldict) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    ocfg, P = _oracle_cfg()
    xq = ld.q_sample(x0, t, noise).cpu()
    loss_ref, grads, dx_ref, dctx_ref, y_ref = ro.unet_objective_and_grads(
        P, ocfg, torch.cat([xq, cond["c_concat"][0].cpu()], 1), t.cpu(), cond["c_crossattn"][0].cpu(), noise.cpu(), ld.logvar.cpu(),
        ld.lvlb_weights.cpu(), 1, 1.0, 0.5)
    print(f"loss {float(loss):.6f} ref {loss_ref:.6f}")
    assert abs(float(loss) - loss_ref) < 1e-4 * abs(loss_ref)
    assert float(ldict["train/loss"]) == float(loss)
    fx = {f"dx.{k}": v for k, v in summarize(dx_ref).items()}
    for name, g in grads.items():
        a = g.double().reshape(-1)
        fx[f"g.{name}.norm"] = float(a.norm())
        fx[f"g.{name}.pick"] = a[torch.from_numpy(pick_index(a.numel()))].numpy()
    check_summary(dx, fx, "dx", 2e-3, "objective")
    worst = _check_grads(unet, fx, 1e-3, "objective")
    err_c = float((dctx.double().cpu() - dctx_ref.double()).norm() / dctx_ref.double().norm())
    print(f"dctx rel-L2 {err_c:.2e}  worst param grad {worst[0]:.2e} at {worst[1]}")
    assert err_c < 1e-3


def test_learned_logvar_trains_with_adamw(dev):
    """Three eager training_step_hip calls with fixed t (a duplicate) and noise: logvar after each step against the oracle's AdamW fed the
    reference d_logvar of the device's model_output (tolerance of test_adamw_ema_step_vs_oracle); entries never drawn move by weight decay
    alone; no EMA shadow for logvar; the optimizer state round-trips with logvar as its last index."""
    from oracle import train as otrain
    lr, wd = 1e-3, 1e-2
    kw = dict(loss_type="l2", learn_logvar=True, logvar_init=0.3, original_elbo_weight=1e-3)
    ld, unet = _ld(dev, **kw)
    ld.train()
    tr = ld.configure_trainer(lr=lr, weight_decay=wd)
    assert len(tr.extra_params) == 1 and tr.extra_params[0] is ld.logvar
    preds, orig = [], tr.loss
    tr.loss = lambda pred, *a, **k: (preds.append(pred.detach().clone()), orig(pred, *a, **k))[1]
    x0, cond, t, noise = _batch(dev, "lv")
    ref = ld.logvar.detach().cpu().clone()
    m, v = torch.zeros_like(ref), torch.zeros_like(ref)
    for step in (1, 2, 3):
        ld.training_step_hip(x0, cond, t, noise)
        r = ro.objective(preds[-1].cpu(), noise.cpu(), t.cpu(), ref, ld.lvlb_weights.cpu(), 1, 1.0, 1e-3)
        otrain.adamw_step(ref, r["d_logvar"].float(), m, v, step, lr, weight_decay=wd)
        got = ld.logvar.detach().cpu()
        print(f"step {step}: logvar[417] {float(got[417]):.7f} ref {float(ref[417]):.7f}")
        assert torch.allclose(got, ref, rtol=2e-6, atol=2e-7), step
    assert float(got[417]) != float(got[5])
    decayed = torch.tensor(0.3)
    for _ in range(3):
        decayed = decayed * (1.0 - lr * wd)
    rest = torch.ones(T, dtype=torch.bool)
    rest[417] = False
    assert torch.allclose(got[rest], decayed.expand(T - 1), rtol=2e-6, atol=2e-7) and bool((got[rest] == got[5]).all())
    ema_keys = {k for k in ld.reference_state_dict() if "model_ema." in k}
    want = {"_model.model_ema.decay", "_model.model_ema.num_updates"} | {"_model.model_ema." + ld._ema_name("diffusion_model." + n)
                                                                         for n, _ in unet.named_parameters()}
    assert ema_keys == want
    sd = tr.optimizer_state_dict()
    last = len(list(unet.parameters()))
    assert max(sd["state"]) == last and tuple(sd["state"][last]["exp_avg"].shape) == (T,)
    assert np.flatnonzero(sd["state"][last]["exp_avg"].cpu().numpy()).tolist() == [417]
    ld2, _ = _ld(dev, **kw)
    tr2 = ld2.configure_trainer(lr=lr, weight_decay=wd)
    tr2.load_optimizer_state_dict(sd)
    sd2 = tr2.optimizer_state_dict()
    assert tr2.step_count == 3 and sd2["param_groups"] == sd["param_groups"]
    for i in sd["state"]:
        assert torch.equal(sd["state"][i]["exp_avg"], sd2["state"][i]["exp_avg"]) and torch.equal(sd["state"][i]["exp_avg_sq"], sd2["state"][i]["exp_avg_sq"])


@pytest.mark.parametrize("learn", [False, True])
def test_graphed_step_equals_the_eager_step_with_the_objective(dev, learn):
    """l2 + VLB term: 3 warm-up + 3 replayed steps of training_step_hip(graph=True) leave the parameters bit-identical to 6 eager steps (the
    shape of test_captured_train_step_equals_the_eager_step_bitwise); with a learned logvar the same flag runs the eager step."""
    kw = dict(loss_type="l2", original_elbo_weight=0.5, logvar_init=-0.7, learn_logvar=learn)
    runs = []
    for graph in (True, False):
        ld, unet = _ld(dev, **kw)
        ld.train()
        losses = []
        for step in range(6):
            x0, cond, t, noise = _batch(dev, f"g{step}", seed=6 + step, t=(951 - 7 * step, 21 + step))
            losses.append(float(ld.training_step_hip(x0, cond, t, noise, graph=graph)))
        torch.cuda.synchronize()
        tr = ld._trainer
        assert (getattr(tr, "_graph", None) is not None) == (graph and not learn) and tr.step_count == 6
        runs.append((losses, [p.detach().clone() for p in ld.parameters()], [e.clone() for e in tr.ema_parameters() if e is not None]))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)


def test_bridge_accumulates_logvar_grad_and_validation_reports_every_term(dev):
    kw = dict(loss_type="l2", learn_logvar=True, logvar_init=0.3, original_elbo_weight=1e-3)
    ld, unet = _ld(dev, **kw)
    ld.train()
    x0, cond, t, noise = _batch(dev, "br")

    def backward_n(k):
        ld.zero_grad(set_to_none=True)
        for _ in range(k):
            with torch.enable_grad():
                loss, ldict = ld.p_losses(x0, cond, t, noise)
                assert loss.requires_grad
                loss.backward()
        return ldict, ld.logvar.grad.clone(), [p.grad.clone() for p in unet.parameters()]

    ldict, lv1, g1 = backward_n(1)
    assert set(ldict) == {"train/loss_simple", "train/loss_gamma", "logvar", "train/loss_vlb", "train/loss"}
    _, lv2, g2 = backward_n(2)
    assert np.flatnonzero(lv1.cpu().numpy()).tolist() == [417]
    assert torch.equal(lv2, 2 * lv1) and all(torch.equal(b, 2 * a) for a, b in zip(g1, g2))
    # no-grad validation: every loss_dict key, against refs_objective on the device's model output
    ld.eval()
    with torch.no_grad():
        y = ld.apply_model(ld.q_sample(x0, t, noise), t, cond).clone()
        loss, vd = ld.p_losses(x0, cond, t, noise)
    assert not loss.requires_grad
    assert set(vd) == {"val/loss_simple", "val/loss_gamma", "logvar", "val/loss_vlb", "val/loss"}
    r = ro.objective(y.cpu(), noise.cpu(), t.cpu(), ld.logvar.detach().cpu(), ld.lvlb_weights.cpu(), 1, 1.0, 1e-3)
    for name in ro.SCALARS:
        err, bound = abs(float(vd["val/" + name]) - float(r[name])), ro.scalar_bound(r, name, ro.K_KERNEL)
        print(f"val/{name}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, name
    assert float(vd["logvar"]) == pytest.approx(0.3, rel=1e-6) and float(loss) == float(vd["val/loss"])
