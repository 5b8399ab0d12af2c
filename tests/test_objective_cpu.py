"""CPU tier of the full training objective (ddpm.py:1015-1048): tests/refs_objective.py against the reference's own p_losses and autograd
(fixture F24, tests/golden/make_golden_objective.py), the schedule's lvlb_weights, and the LatentDiffusion constructor surface."""
import numpy as np
import pytest
import torch

from tests import refs_objective as ro

CASES = ("l1_default", "l2_default", "l2_elbo", "l1_weighted", "l2_learned")


def f24_case(golden, name):
    g = golden("f24_objective")
    kind, lsw, ew, lv0, learn = (float(v) for v in g[name + "_cfg"])
    c = {"kind": int(kind), "lsw": lsw, "ew": ew, "lv0": lv0, "learn": bool(learn), "t": torch.from_numpy(g["t"]),
         "lvlb": torch.from_numpy(g["lvlb_weights"])}
    for k in ("model_output", "target", "d_model_output", "d_logvar", "loss", "loss_simple", "loss_vlb"):
        c[k] = torch.from_numpy(np.asarray(g[f"{name}_{k}"]))
    if c["learn"]:
        c["loss_gamma"] = torch.from_numpy(np.asarray(g[name + "_loss_gamma"]))
        c["logvar_mean"] = float(g[name + "_logvar_mean"])
    c["logvar"] = torch.full((1000,), lv0, dtype=torch.float32)
    return c


def check_against_f24(c, got, K, Kd):
    """got: {loss, loss_simple, loss_vlb, (loss_gamma), d_pred, d_logvar} as fp64 CPU tensors, against the fixture within the bounds that
    refs_objective derives for K (scalars, d_logvar) and Kd (d_pred) roundings."""
    r = ro.objective(c["model_output"], c["target"], c["t"], c["logvar"], c["lvlb"], c["kind"], c["lsw"], c["ew"])
    for name in ("loss", "loss_simple", "loss_vlb") + (("loss_gamma",) if c["learn"] else ()):
        err, bound = abs(float(got[name]) - float(c[name])), ro.scalar_bound(r, name, K)
        print(f"{name}: |got - F24| {err:.3e}  bound {bound:.3e}")
        assert err <= bound, name
    err = (got["d_pred"] - c["d_model_output"].double()).abs()
    print(f"d_pred: max err / bound {float((err / ro.d_pred_bound(r, Kd).clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= ro.d_pred_bound(r, Kd)).all())
    err = (got["d_logvar"] - c["d_logvar"].double()).abs()
    print(f"d_logvar: max err {float(err.max()):.3e}  bound at 417 {float(ro.d_logvar_bound(r, K)[417]):.3e}")
    assert bool((err <= ro.d_logvar_bound(r, K)).all())


@pytest.mark.parametrize("name", CASES)
def test_refs_reproduce_the_reference_p_losses(golden, name):
    c = f24_case(golden, name)
    B, n = 4, 120
    assert tuple(c["model_output"].shape) == (4, 4, 6, 5) and c["t"].tolist() == [0, 999, 417, 417]
    r = ro.objective(c["model_output"], c["target"], c["t"], c["logvar"], c["lvlb"], c["kind"], c["lsw"], c["ew"])
    check_against_f24(c, r, ro.k_ref(n, B) + ro.K_KERNEL, ro.K_REF_DPRED + ro.K_KERNEL_DPRED)
    # the reference leaves every logvar entry that t does not name without a gradient, and sums the duplicate
    assert sorted(np.flatnonzero(c["d_logvar"].numpy()).tolist()) == [0, 417, 999]
    assert sorted(np.flatnonzero(r["d_logvar"].numpy()).tolist()) == [0, 417, 999]
    if c["learn"]:
        assert c["logvar_mean"] == pytest.approx(c["lv0"], rel=1e-6)


@pytest.mark.parametrize("kind", [0, 1])
def test_refs_gradients_are_the_derivatives_of_the_refs_loss(kind):
    """d_pred and d_logvar of refs_objective against fp64 autograd over the same formula (duplicate timesteps, both signs of logvar)."""
    from tests.refs_bwd import normal
    B, T = 5, 12
    pred, target = normal((B, 3, 4, 5), 1, "p").double(), normal((B, 3, 4, 5), 1, "q").double()
    t = torch.tensor([3, 0, 3, 11, 3])
    lvlb = normal((T,), 1, "w").abs().double() + 0.1
    lv = (normal((T,), 1, "lv") * 0.5).double().requires_grad_(True)
    pg = pred.clone().requires_grad_(True)
    with torch.enable_grad():                 # (other test modules switch autograd off process-wide)
        d = target - pg
        ls = (d.abs() if kind == 0 else d * d).mean(dim=[1, 2, 3])
        loss = 0.3 * (ls / torch.exp(lv[t]) + lv[t]).mean() + 0.7 * (lvlb[t] * ls).mean()
        loss.backward()
    r = ro.objective(pred, target, t, lv.detach(), lvlb, kind, 0.3, 0.7, gscale=0.25)
    assert float(r["loss"]) == pytest.approx(float(loss.detach()), rel=1e-14)
    assert torch.allclose(r["d_pred"], 0.25 * pg.grad, rtol=1e-13, atol=0)
    assert torch.allclose(r["d_logvar"], 0.25 * lv.grad, rtol=1e-13, atol=1e-18)


def test_lvlb_weights_equal_the_reference_bit_for_bit(golden):
    from stedm_amd.schedule import lvlb_weights
    want = golden("f24_objective")["lvlb_weights"]
    got = lvlb_weights(1000, 0.0015, 0.0205)
    assert got.dtype == np.float32 and got.shape == (1000,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == got[1]


def _ld(**kw):
    from stedm_amd.latent_diffusion import LatentDiffusion
    return LatentDiffusion(torch.nn.Conv2d(4, 4, 1), linear_start=0.0015, linear_end=0.0205, image_size=8, channels=4,
                           conditioning_key="hybrid", **kw)


def test_lvlb_weights_is_a_non_persistent_buffer(golden):
    ld = _ld(loss_type="l1")
    assert np.array_equal(ld.lvlb_weights.numpy(), golden("f24_objective")["lvlb_weights"])
    assert "lvlb_weights" in dict(ld.named_buffers()) and "lvlb_weights" not in ld.state_dict()


def test_learned_logvar_is_a_parameter_under_the_same_key():
    ld = _ld(learn_logvar=True, logvar_init=0.3)
    assert isinstance(ld.logvar, torch.nn.Parameter) and ld.logvar.requires_grad and ld.learn_logvar is True
    assert tuple(ld.logvar.shape) == (1000,) and bool((ld.logvar.detach() == torch.tensor(0.3)).all())
    assert "logvar" in ld.state_dict() and "logvar" in dict(ld.named_parameters())
    assert ld.loss_type == "l2"                       # the constructor's default, as the reference's
    plain = _ld(loss_type="l1")
    assert not isinstance(plain.logvar, torch.nn.Parameter) and set(plain.state_dict()) == set(ld.state_dict())
    assert float(_ld(logvar_init=-0.7).logvar[5]) == pytest.approx(-0.7)


def test_objective_options_construct():
    ld = _ld(loss_type="l2", original_elbo_weight=0.5, l_simple_weight=0.25)
    assert (ld.loss_type, ld.original_elbo_weight, ld.l_simple_weight, ld.learn_logvar) == ("l2", 0.5, 0.25, False)
    obj = ld._objective()
    assert (obj.kind, obj.elbo_weight, obj.l_simple_weight, obj.learned, obj.plain) == ("l2", 0.5, 0.25, False, False)
    assert obj.logvar is ld.logvar and obj.lvlb is ld.lvlb_weights
    assert _ld(loss_type="l1")._objective().plain                         # the reference configs' point stays on the L1 kernel
    assert not _ld(loss_type="l1", logvar_init=0.1)._objective().plain
    assert not _ld(loss_type="l1", learn_logvar=True)._objective().plain


def test_unknown_loss_type_and_x0_are_refused():
    with pytest.raises((NotImplementedError, ValueError)):
        _ld(loss_type="huber")
    with pytest.raises((NotImplementedError, AssertionError)):
        _ld(loss_type="l1", parameterization="x0")


def test_learned_logvar_joins_the_optimizer_last():
    """configure_trainer appends logvar after the U-Net's (and the cond stage's) parameters: the reference's optimizer order."""
    ld = _ld(loss_type="l2", learn_logvar=True)
    ld.model.diffusion_model._buf = None              # (a stand-in U-Net: the trainer only stores it here)
    tr = ld.configure_trainer()
    assert tr.extra_params and tr.extra_params[-1] is ld.logvar
    assert tr._torch_param_order()[-1] is ld.logvar
    assert not ld._cond_stage_in_optimizer()
