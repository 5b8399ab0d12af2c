"""CPU tier: the learning-rate schedulers against the reference's recorded multipliers (tests/golden/f28_lr_schedules.npz, written by
tests/golden/make_golden_lr.py), scheduler_config / gradient_clip_* handling of LatentDiffusion, the device schedule's learning-rate column,
and the clipping references of tests/refs_clip.py against torch.nn.utils.clip_grad_norm_."""
import math

import numpy as np
import pytest
import torch

from tests import refs_clip
from tests.golden.make_golden_lr import CONFIGS

TINY = refs_clip.TINY


def _ld(**kw):
    from stedm_amd.latent_diffusion import LatentDiffusion
    from stedm_amd.unet import UNetModel
    return LatentDiffusion(UNetModel(precision="parity", **TINY).eval(), linear_start=0.0015, linear_end=0.0205, loss_type="l1", image_size=16,
                           channels=4, conditioning_key="hybrid", **kw)


LINEAR_CFG = {"target": "ldm.lr_scheduler.LambdaLinearScheduler",
              "params": {"warm_up_steps": [4], "f_min": [0.1], "f_max": [1.0], "f_start": [1e-6], "cycle_lengths": [1000]}}


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_scheduler_multipliers_equal_the_reference(golden, tag):
    """every n from 0 to past the last boundary (each warm-up end, each cycle boundary, past max_decay_steps): equal after rounding to fp32 (both
    sides compute in double; the learning rate reaches the kernels as an fp32)"""
    from stedm_amd import lr_scheduler
    cls, params, last = CONFIGS[tag]
    fx = golden("f28_lr_schedules")
    n, f = fx[f"{tag}_n"], fx[f"{tag}_f"]
    assert len(n) == last + 1 and f.dtype == np.float64
    bounds = [params["warm_up_steps"], params["max_decay_steps"]] if tag == "cosine" else \
        list(np.cumsum(params["cycle_lengths"])) + [c + w for c, w in zip([0] + list(np.cumsum(params["cycle_lengths"]))[:-1], params["warm_up_steps"])]
    assert all(b in n for b in bounds) and (tag != "cosine" or n[-1] > params["max_decay_steps"])
    sch = getattr(lr_scheduler, cls)(**params)
    for call in (sch.schedule, sch):
        got = np.asarray([call(int(k)) for k in n], dtype=np.float64)
        assert np.array_equal(got.astype(np.float32), f.astype(np.float32)), (tag, np.abs(got - f).max())
    # the mapped reference target builds the same object
    sch2 = lr_scheduler.instantiate_from_config({"target": f"ldm.lr_scheduler.{cls}", "params": params})
    assert type(sch2) is type(sch) and sch2.schedule(3) == sch.schedule(3)


def test_scheduler_config_is_instantiated_or_refused():
    from stedm_amd import lr_scheduler
    from stedm_amd.train import UNetTrainer
    ld = _ld()
    assert ld.use_scheduler is False and ld.lr_scheduler is None
    assert ld.configure_trainer(lr=1e-3).lr_lambda is None
    ld = _ld(scheduler_config=LINEAR_CFG)
    assert ld.use_scheduler is True and isinstance(ld.lr_scheduler, lr_scheduler.LambdaLinearScheduler)
    tr = ld.configure_trainer(lr=2e-4, gradient_clip_val=0.5)
    assert isinstance(tr, UNetTrainer) and tr.max_grad_norm == 0.5 and tr.lr == 2e-4
    assert tr.lr_lambda(2) == ld.lr_scheduler.schedule(2) == lr_scheduler.LambdaLinearScheduler(**LINEAR_CFG["params"]).schedule(2)
    # step s runs with base * f(s - 1); current_lr() is the rate of the next step; a resumed step count needs no scheduler state
    f = ld.lr_scheduler.schedule
    assert tr.current_lr() == ld.current_lr() == 2e-4 * f(0)
    tr.step_count = 7
    assert tr.current_lr() == 2e-4 * f(7) and tr._lr_at(7) == 2e-4 * f(6) and tr.lr == 2e-4
    with pytest.raises(NotImplementedError, match="no_such"):
        _ld(scheduler_config={"target": "ldm.lr_scheduler.no_such", "params": {}})
    with pytest.raises(NotImplementedError):
        _ld(scheduler_config={"target": "torch.optim.lr_scheduler.StepLR", "params": {}})
    with pytest.raises(KeyError, match="target"):
        _ld(scheduler_config={"params": LINEAR_CFG["params"]})


def test_gradient_clip_arguments():
    ld = _ld()
    with pytest.raises(NotImplementedError, match="value"):
        ld.configure_trainer(gradient_clip_val=0.5, gradient_clip_algorithm="value")
    with pytest.raises(ValueError):
        ld.configure_trainer(gradient_clip_val=0.5, gradient_clip_algorithm="median")
    with pytest.raises(ValueError):
        ld.configure_trainer(gradient_clip_val=-1.0)
    assert ld.configure_trainer().max_grad_norm is None and ld.last_grad_norm is None
    assert ld.configure_trainer(gradient_clip_val=0).max_grad_norm is None          # Lightning: 0 means no clipping
    assert ld.configure_trainer(gradient_clip_val=1.5, gradient_clip_algorithm="norm").max_grad_norm == 1.5


def test_ldm_module_hands_the_cfg_keys_to_the_trainer():
    """LDM_Diffusion reads Lightning's names from the cfg (optional) and the scheduler_config of cfg.diffusion; a cfg without them is as before"""
    from stedm_amd.ldm_module import LDM_Diffusion
    unet = dict(image_size=16, in_channels=7, model_channels=128, out_channels=4, num_res_blocks=1, attention_resolutions=[32, 16, 8],
                channel_mult=[1, 2], num_heads=4)

    def cfg(extra=None, scheduler=None):
        d = {"lr": 1e-3, "cfg_scale": 1.5, "ddim_steps": 4, "eta": 0.0, "data": {"patch_size": 64}, "style_sampling": {"name": "mp", "num_patches": 2},
             "style_agg": dict(name="svit", patch_size=8, dim=64, depth=1, heads=2, mlp_dim=64, pool="mean", channels=3, dropout=0.0, emb_dropout=0.0,
                               t_dim=64),
             "diffusion": dict(linear_start=0.0015, linear_end=0.0205, timesteps=1000, loss_type="l1", first_stage_key="image",
                               cond_stage_key="segmentation", image_size=16, channels=4, conditioning_key="hybrid",
                               unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(unet)})}
        d.update(extra or {})
        if scheduler is not None:
            d["diffusion"]["scheduler_config"] = scheduler
        return d

    def trainer(c):
        mod = LDM_Diffusion(c, accumulate_grad_batches=2)
        mod.configure_optimizers()
        return mod._model, mod._model.__dict__["_trainer"]

    model, tr = trainer(cfg())
    assert tr.max_grad_norm is None and tr.lr_lambda is None and model.use_scheduler is False and tr.accumulate_grad_batches == 2
    model, tr = trainer(cfg({"gradient_clip_val": 0.7, "gradient_clip_algorithm": "norm"}, LINEAR_CFG))
    assert tr.max_grad_norm == 0.7 and model.use_scheduler is True and tr.lr == 1e-3 and tr.current_lr() == 1e-3 * model.lr_scheduler.schedule(0)
    with pytest.raises(NotImplementedError, match="value"):
        trainer(cfg({"gradient_clip_val": 0.7, "gradient_clip_algorithm": "value"}))


def test_schedule_rows_carry_the_lambda():
    """column 3 of the captured step's device schedule is fp32(base * f(s - 1)) for the step s of each row; the other columns do not move"""
    from stedm_amd.lr_scheduler import LambdaLinearScheduler
    from stedm_amd.train import UNetTrainer
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision="parity", **TINY).eval()
    f = LambdaLinearScheduler(warm_up_steps=[4, 3], f_min=[0.1, 0.05], f_max=[1.0, 0.5], f_start=[1e-6, 0.01], cycle_lengths=[10, 4000]).schedule
    plain, sched = UNetTrainer(m, lr=3e-4), UNetTrainer(m, lr=3e-4, lr_lambda=f)
    for first, e, n in ((1, 1, 40), (9, 5, 7), (3000, 3000, 5)):
        a, b = plain._sched_rows(first, e, n), sched._sched_rows(first, e, n)
        assert a.shape == b.shape == (n, 4) and a.dtype == b.dtype == np.float32
        assert np.array_equal(a[:, :3], b[:, :3])
        assert np.array_equal(a[:, 3], np.full((n,), np.float32(3e-4)))
        want = np.asarray([np.float32(3e-4 * f(s - 1)) for s in range(first, first + n)], dtype=np.float32)
        assert np.array_equal(b[:, 3], want)
    assert len(set(sched._sched_rows(1, 1, 12)[:, 3].tolist())) == 12          # (the schedule really moves every step here)
    # row 0 of the first window stands for a step 0 that does not exist (never read): it repeats step 1's rate; _lr_at itself refuses it
    assert sched._sched_rows(0, 0, 2)[0, 3] == sched._sched_rows(0, 0, 2)[1, 3] == np.float32(3e-4 * f(0))
    with pytest.raises(ValueError):
        sched._lr_at(0)


@pytest.mark.parametrize("step_count", [0, 990, 1000])
def test_schedule_window_ends_where_a_finite_cycle_ends(step_count):
    """A scheduler whose cycles end (the reference's raise past the last one) with the default GRAPH_WINDOW of 4096 rows: the window is filled up
    to the last step the schedule defines (n = 1000, optimizer step 1001), the rows behind it are NaN and never reached — the refill bound is
    the count of usable rows — and the lambda's own error comes up only where the eager step would raise it: when the NEXT step has no rate."""
    from stedm_amd.lr_scheduler import LambdaLinearScheduler
    from stedm_amd.train import UNetTrainer
    from stedm_amd.unet import UNetModel
    f = LambdaLinearScheduler(**LINEAR_CFG["params"]).schedule          # cycle_lengths = [1000]
    tr = UNetTrainer(UNetModel(precision="parity", **TINY).eval(), lr=2e-4, lr_lambda=f)
    assert tr.GRAPH_WINDOW == 4096
    tr.step_count = tr.ema_updates = step_count
    rows, valid = tr._sched_rows(step_count, step_count, tr.GRAPH_WINDOW, with_valid=True)
    assert rows.shape == (4096, 4) and valid == 1001 - step_count + 1           # rows of steps step_count .. 1001
    for i in range(1, valid):
        assert rows[i, 3] == np.float32(2e-4 * f(step_count + i - 1))
    assert np.isnan(rows[valid:, 3]).all() and np.isfinite(rows[:, :3]).all()
    assert np.array_equal(tr._sched_rows(step_count, step_count, tr.GRAPH_WINDOW), rows, equal_nan=True)
    g = {"sched": torch.empty((tr.GRAPH_WINDOW, 4)), "idx": torch.ones((1,), dtype=torch.int32)}
    tr._graph_window(g)
    assert g["valid"] == valid and g["base"] == step_count and int(g["idx"]) == 0 and np.array_equal(g["sched"].numpy(), rows, equal_nan=True)
    # the row index of the next step, step_count + 1 - base, stays below the refill bound for every step the schedule defines
    assert min(tr.GRAPH_WINDOW, g["valid"]) == 1001 - step_count + 1
    tr.step_count = tr.ema_updates = 1001                                         # the schedule's last step has been taken
    with pytest.raises(ValueError, match="past the last cycle"):
        tr._graph_window(g)
    with pytest.raises(ValueError, match="past the last cycle"):
        tr._lr_at(1002)
    # without a lambda nothing changes: every row usable
    plain = UNetTrainer(UNetModel(precision="parity", **TINY).eval(), lr=2e-4)
    assert plain._sched_rows(1, 1, 5, with_valid=True)[1] == 5


def test_optimizer_state_dict_layout_under_a_schedule():
    """torch under LambdaLR: the param group holds lr (current) and initial_lr (base); the base rate comes back from initial_lr"""
    sd_group = dict(lr=5e-5, initial_lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    from stedm_amd.train import UNetTrainer
    from stedm_amd.unet import UNetModel
    tr = UNetTrainer(UNetModel(precision="parity", **TINY).eval(), lr=1e-3, lr_lambda=lambda n: 0.5)
    tr._opt = {"params": [], "m": [], "v": []}
    tr._torch_param_order = lambda: []
    tr._opt_resume = {"state": {}, "param_groups": [sd_group]}
    tr._apply_opt_resume()
    assert tr.lr == 2e-4 and tr.current_lr() == 1e-4
    g = tr.optimizer_state_dict()["param_groups"][0]
    assert g["lr"] == 1e-4 and g["initial_lr"] == 2e-4
    tr._opt_resume = {"state": {}, "param_groups": [dict(lr=7e-4)]}           # a checkpoint written without a scheduler
    tr._apply_opt_resume()
    assert tr.lr == 7e-4


CLIP_SHAPES = [(7, 5), (33,), (4, 3, 3), (1,)]


def _clip_case(kind):
    from stedm_amd.utils import prng
    gs = [prng.normal(3, f"clip.{i}", sh) * 0.7 for i, sh in enumerate(CLIP_SHAPES)]
    if kind == "inf":
        gs[1][5] = float("inf")
    if kind == "nan":
        gs[2][1, 2, 0] = float("nan")
    return gs


@pytest.mark.parametrize("kind,max_norm", [("finite", 0.5), ("finite", 1e3), ("inf", 0.5), ("nan", 0.5)])
def test_reference_clip_agrees_with_torch(kind, max_norm):
    """refs_clip (float64 norm rounded once to fp32, torch's fp32 coefficient) against torch.nn.utils.clip_grad_norm_ on fp32 tensors. torch sums
    the N = 81 squares in fp32: at most N + 2 roundings of 2^-24 each on the sum of squares (half of that on the root, bounded here by the whole),
    the same again through the coefficient into the clipped gradients. A non-finite entry: an inf norm makes the coefficient 0 (finite entries
    become 0, the inf one NaN), a NaN norm makes everything NaN, on both sides."""
    n_el = sum(int(np.prod(s)) for s in CLIP_SHAPES)
    tol = (n_el + 2) * 2.0 ** -24
    params = [torch.nn.Parameter(torch.zeros(s)) for s in CLIP_SHAPES]
    for p, g in zip(params, _clip_case(kind)):
        p.grad = g.clone()
    tn = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    mine = _clip_case(kind)
    norm, coef = refs_clip.clip_grads_(mine, max_norm)
    if kind == "finite":
        assert abs(float(norm) - tn) <= tol * tn
        assert (coef == 1.0) == (tn < max_norm)
        for p, g in zip(params, mine):
            assert torch.allclose(p.grad, g, rtol=2 * tol, atol=0.0)
    elif kind == "inf":
        assert math.isinf(tn) and math.isinf(float(norm)) and float(coef) == 0.0
        for p, g in zip(params, mine):
            assert torch.equal(torch.isnan(p.grad), torch.isnan(g)) and torch.equal(torch.nan_to_num(p.grad, nan=7.0), torch.nan_to_num(g, nan=7.0))
        assert int(sum(torch.isnan(g).sum() for g in mine)) == 1 and all(float(torch.nan_to_num(g, nan=0.0).abs().max()) == 0.0 for g in mine)
    else:
        assert math.isnan(tn) and math.isnan(float(norm)) and math.isnan(float(coef))
        assert all(bool(torch.isnan(p.grad).all()) and bool(torch.isnan(g).all()) for p, g in zip(params, mine))
    assert float(refs_clip.clip_coef32(np.float32(3.0), 0.0)) == 1.0 and float(refs_clip.clip_coef32(np.float32("nan"), 0.0)) == 1.0


def test_fp32_clipped_adamw_reference_stays_within_the_kernel_tolerances_of_float64():
    """The GPU test holds the clipped kernel steps to rtol 2e-6 / atol 2e-7 of the fp32 CPU reference (clip_grad_norm_ + the oracle's AdamW / EMA):
    that reference itself stays inside the same tolerances of its float64 twin on the same gradients, and step 1 is unclipped, steps 2 and 3
    clipped."""
    p32, e32, n32 = refs_clip.tiny_unet_clip_reference("float32")
    p64, e64, n64 = refs_clip.tiny_unet_clip_reference("float64")
    mx = refs_clip.clip_steps_max_norm([tuple(p.shape) for p in p32])
    assert n64[0] < mx < n64[2] < n64[1], (n64, mx)
    assert np.allclose(n32, n64, rtol=1e-5)
    worst = 0.0
    for a, b in zip(p32 + e32, p64 + e64):
        d = (a.double() - b).abs()
        worst = max(worst, float((d / (2e-7 + 2e-6 * b.abs())).max()))
        assert torch.allclose(a.double(), b, rtol=2e-6, atol=2e-7)
    print(f"fp32 reference vs float64 reference after three clipped steps: worst |d| / (atol + rtol |ref|) = {worst:.3f}")
