"""GPU tier (-m gpu): the general DPM-Solver (stedm_amd/dpm_solver.py: dpm_plan, stedm_dpm_update, stedm_dpm_threshold) on the HIP path.
  * stedm_dpm_update against its torch restatement bit for bit: every row kind, noise and data prediction, with and without CFG, the
    three modes, B = 1, an element count off the float4 grid, misaligned operands;
  * stedm_dpm_threshold: quantiles bit for bit equal to CPU torch.quantile, outputs equal to the restatement, ties included;
  * F22 on the HIP sampler with the closed-form eps model: eager == graphed bit for bit, both within 1e-4 of the reference;
  * the TINY U-Net through sample_log(sampler="dpm_solver", ...) against the CPU restatement over the oracle U-Net (3M + CFG 1.5,
    singlestep-3 with thresholding), eager == graphed;
  * predict_latents(sampler="dpm_solver", dpm_solver={...}) end to end and its shard invariance."""
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_dpm_solver_general_oracle import dpm_threshold_ref, dpm_update_ref, f22_case, plan_sample
from tests.test_dpm_solver_oracle import toy_eps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


def _plans():
    from oracle import ddim as od
    from stedm_amd.dpm_solver import dpm_plan
    ac = od.Schedule().alphas_cumprod
    return [dpm_plan(ac, 8, order=3), dpm_plan(ac, 8, order=3, predict_x0=False), dpm_plan(ac, 6, order=3, method="singlestep",
            solver_type="taylor"), dpm_plan(ac, 5, order=2, method="singlestep", predict_x0=False, denoise_to_zero=True)]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (3, 3, 5, 7)])
def test_dpm_update_kernel_matches_torch_bitwise(dev, shape):
    from stedm_amd import dpm_solver as D, ops
    n = 1
    for v in shape:
        n *= v
    kinds = set()
    for p in _plans():
        rows = p.rows.to(dev)
        for i in range(p.rows.shape[0]):
            row = p.rows[i]
            kinds.add(int(row[D.R_KIND]))
            g = lambda k: prng.normal(80 + i, k, shape)
            x, base, ec, eu = g("x"), g("b"), g("ec"), g("eu")
            sl = [g("s0"), g("s1"), g("s2")]
            step = torch.tensor([i], dtype=torch.int32, device=dev)
            for cfg in (False, True):
                s = 1.5 if cfg else 1.0
                want_sl = list(sl)
                want_x, want_b, want_p = dpm_update_ref(row, x, base, want_sl, ec, eu if cfg else None, s)
                # aligned, separate base
                xd, bd, sd, pd = x.to(dev), base.to(dev), torch.stack(sl).to(dev), torch.empty(shape, device=dev)
                ops.dpm_update(xd, bd, ec.to(dev), eu.to(dev) if cfg else None, sd, rows, step_idx=step, cfg_scale=s, pred_x0=pd)
                w = int(row[D.R_W])
                for got, want, nm in ((xd, want_x, "x"), (bd, want_b, "base"), (sd[w], want_sl[w], "slot"), (pd, want_p, "pred")):
                    assert torch.equal(got.cpu(), want), (i, cfg, nm, float((got.cpu() - want).abs().max()))
                # misaligned: every operand one float off the 16-byte grid, split into MODEL + COMBINE
                buf = torch.zeros(1 + 9 * n, device=dev)
                v = lambda k: buf[1 + k * n:1 + (k + 1) * n].view(shape)
                xm, bm, ecm, eum, pm = v(0), v(1), v(2), v(3), v(4)
                sm = buf[1 + 5 * n:1 + 8 * n].view((3,) + shape)
                xm.copy_(x.to(dev)); bm.copy_(base.to(dev)); ecm.copy_(ec.to(dev)); eum.copy_(eu.to(dev)); sm.copy_(torch.stack(sl).to(dev))
                ops.dpm_update(xm, bm, ecm, eum if cfg else None, sm, rows, step_idx=step, cfg_scale=s, mode=ops.DPMU_MODEL)
                assert torch.equal(sm[w].cpu(), want_sl[w]) and torch.equal(xm.cpu(), x)
                ops.dpm_update(xm, bm, None, None, sm, rows, step_idx=step, mode=ops.DPMU_COMBINE, pred_x0=pm)
                assert torch.equal(xm.cpu(), want_x) and torch.equal(bm.cpu(), want_b) and torch.equal(pm.cpu(), want_p), (i, cfg)
    assert kinds == {D.K_FIRST, D.K_DIFF, D.K_MS3, D.K_SS3T, D.K_COPY}
    # the default keywords (DPM-Solver++(2M)) as a multistep run has them: base IS x; rows 0 (first order), 2 (second order) and 4 (the
    # first-order final step) of a 5-step plan, against this file's restatement and against the 2M expression stated on its own
    from oracle import ddim as od
    from tests.test_dpm_solver_oracle import dpm_update_ref as dpm_2m_ref, rows_2m
    p = D.dpm_plan(od.Schedule().alphas_cumprod, 5)
    rows, coefs = p.rows.to(dev), rows_2m(p)
    assert p.orders == [1, 2, 2, 2, 1]
    g = lambda k: prng.normal(70, k, shape)
    x, ec, eu, x0_prev = g("k.x"), g("k.ec"), g("k.eu"), g("k.x0p")
    for i in (0, 2, 4):
        row, w = p.rows[i], i % 3
        step = torch.tensor([i], dtype=torch.int32, device=dev)
        sl = [torch.full(shape, float("nan"))] * 3          # a first-order row reads no stored slot, a second-order row slot (i - 1) mod 3
        if p.orders[i] == 2:
            sl[(i - 1) % 3] = x0_prev
        for cfg in (False, True):
            s = 1.5 if cfg else 1.0
            want_sl = list(sl)
            want_x, want_b, want_p = dpm_update_ref(row, x, x, want_sl, ec, eu if cfg else None, s)
            x_2m, x0_2m = dpm_2m_ref(x, ec, eu if cfg else None, x0_prev, coefs[i], s)
            assert torch.equal(want_x, x_2m) and torch.equal(want_sl[w], x0_2m) and want_b is want_x and torch.equal(want_p, x0_2m)
            xd, sd, pd = x.to(dev), torch.stack(sl).to(dev), torch.empty(shape, device=dev)
            ops.dpm_update(xd, xd, ec.to(dev), eu.to(dev) if cfg else None, sd, rows, step_idx=step, cfg_scale=s, pred_x0=pd)
            for got, want, nm in ((xd, x_2m, "x"), (sd[w], x0_2m, "slot"), (pd, x0_2m, "pred")):
                assert torch.equal(got.cpu(), want), (i, cfg, nm, float((got.cpu() - want).abs().max()))
            # pred_x0 aliasing the written slot, and e_c / e_u slices off the 16-byte grid (the elementwise form)
            buf = torch.cat([torch.zeros(1), ec.flatten(), eu.flatten()]).to(dev)
            ec_m, eu_m = buf[1:1 + n].view(shape), buf[1 + n:].view(shape)
            xd2, sd2 = x.to(dev), torch.stack(sl).to(dev)
            ops.dpm_update(xd2, xd2, ec_m, eu_m if cfg else None, sd2, rows, step_idx=step, cfg_scale=s, pred_x0=sd2[w])
            assert torch.equal(xd2, xd) and torch.equal(sd2[w], sd[w]), (i, cfg)


@pytest.mark.parametrize("n,B", [(256, 64), (2304, 3), (4096, 64), (65536, 1), (65536, 3)])
def test_dpm_threshold_kernel_quantile_bitwise(dev, n, B):
    from stedm_amd import ops
    x = prng.normal(90 + n, "th.x", (B, n)) * torch.linspace(0.2, 3.0, B)[:, None]
    x[0, : n // 3] = (x[0, : n // 3] * 4).round() / 4          # ties
    x[-1, ::5] = -0.0
    xd = x.to(dev)
    q = torch.empty(B, device=dev)
    ops.dpm_threshold(xd, 1.0, q_out=q)
    want_x, want_q = dpm_threshold_ref(x, 1.0)
    assert torch.equal(q.cpu(), torch.quantile(x.abs(), 0.995, dim=1))
    assert torch.equal(q.cpu(), want_q) and torch.equal(xd.cpu(), want_x)


def test_dpm_threshold_follows_the_row(dev):
    from stedm_amd import dpm_solver as D, ops
    from oracle import ddim as od
    p = D.dpm_plan(od.Schedule().alphas_cumprod, 5, order=2, predict_x0=False, thresholding=True, max_val=0.5, denoise_to_zero=True)
    rows = p.rows.to(dev)
    sl = prng.normal(91, "th.s", (3, 2, 4, 8, 8)) * 2
    for i in (0, 5):            # a noise-prediction row (no thresholding), the denoise_to_zero row (thresholds slot 0)
        sd = sl.to(dev)
        ops.dpm_threshold(sd, 0.5, rows=rows, step_idx=torch.tensor([i], dtype=torch.int32, device=dev))
        want = sl.clone()
        if i == 5:
            want[0] = dpm_threshold_ref(sl[0], 0.5)[0]
        assert torch.equal(sd.cpu(), want), i


# ------------------------------------------------------------------------------------------------ F22 through the HIP sampler
class GraphToy:
    """F22's closed-form eps model on the device, as in-place torch ops into preallocated buffers (capturable), with the model surface
    DPMSolverSampler reads (apply_model / apply_model_cfg with out= and uniform_t=)."""

    def __init__(self, dev, ac, shape):
        self.num_timesteps = 1000
        self.alphas_cumprod = ac.to(dev)
        self.parameterization = "eps"
        self.device = dev
        self.calls = 0
        B = shape[0]
        self.w1, self.w2 = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
        self.u, self.a, self.c, self.sn = (torch.empty((B, 1, 1, 1), device=dev) for _ in range(4))

    def _toy(self, x, t, bias, out):
        tf = t.view(-1, 1, 1, 1)
        torch.div(tf, 1000.0, out=self.u)
        torch.add(self.u, 0.5, out=self.a)
        torch.mul(x, self.a, out=self.w1)
        torch.add(self.w1, bias, out=self.w1)
        torch.tanh(self.w1, out=self.w1)
        torch.mul(self.u, 0.3, out=self.c)
        torch.add(self.c, 0.8, out=self.c)
        torch.mul(self.w1, self.c, out=self.w1)
        torch.mul(bias, 0.1, out=self.w2)
        torch.add(self.w1, self.w2, out=self.w1)
        torch.sin(tf, out=self.sn)
        torch.mul(self.sn, 0.05, out=self.sn)
        torch.add(self.w1, self.sn, out=out)
        return out

    def apply_model(self, x, t, c, out=None, uniform_t=False):
        self.calls += 1
        return self._toy(x, t, c["bias"], torch.empty_like(x) if out is None else out)

    def apply_model_cfg(self, x, t, c, uc, out=None, uniform_t=False):
        self.calls += 1
        B = x.shape[0]
        out = torch.empty((2 * B,) + tuple(x.shape[1:]), device=x.device) if out is None else out
        return self._toy(x, t, c["bias"], out[:B]), self._toy(x, t, uc["bias"], out[B:])


@pytest.mark.parametrize("name", ["ms3_cfg_s20", "ms3_noise_s10", "ss3_logsnr_s9", "ss3_taylor_cfg_s9", "ss2_noise_taylor_s7",
                                  "ssfixed3_quad_s9", "thr_ms2_cfg_s10", "thr_ss3_s10", "d2z_noise_thr_s8", "tse_ms3_s16"])
def test_f22_on_the_hip_sampler_eager_and_graph(dev, golden, name):
    from stedm_amd.dpm_solver import DPMSolverSampler
    c = f22_case(golden, name)
    cfg = c["scale"] != 1.0
    kw = dict(unconditional_guidance_scale=c["scale"], unconditional_conditioning={"bias": c["uncond"].to(dev)}) if cfg else {}
    outs = {}
    for g in (False, True):
        toy = GraphToy(dev, c["ac"], (2, 4, 8, 8))
        seen = []
        cb = {} if g else dict(img_callback=lambda p, i: seen.append(i))
        x, none = DPMSolverSampler(toy, device=dev, use_graph=g).sample(c["S"], 2, (4, 8, 8), {"bias": c["cond"].to(dev)},
                                                                        x_T=c["xT"].to(dev), **kw, **cb, **c["kw"])
        R = c["t"].shape[0]
        assert none is None and toy.calls == (2 if g and R > 1 else R)          # graphed: the warm-up NFE and the captured one
        if not g:
            assert seen == list(range(R))
        outs[g] = x.clone()
        err = rel(x, c["out"])
        print(f"[F22 {name} graph={g}] max|diff|/std vs the reference {err:.3e}")
        assert err < 1e-4
    assert torch.equal(outs[False], outs[True])


# ------------------------------------------------------------------------------------------------ TINY U-Net
RUNS = {"3m_cfg_s12": (12, dict(order=3)), "ss3_thr_s10": (10, dict(order=3, method="singlestep", thresholding=True, max_val=1.0))}


@pytest.mark.parametrize("name", list(RUNS))
def test_tiny_unet_general_vs_oracle_eager_graph(dev, name):
    from stedm_amd.dpm_solver import dpm_plan
    from tests.test_gpu_dpm_solver import _inputs, _ld, _oracle_unet
    S, kw = RUNS[name]
    xT, cc, ctx, ctx_u = _inputs()
    outs = {}
    for g in (False, True):
        ld = _ld(dev, g)
        cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
        unc = {"c_concat": [cc.to(dev).clone()], "c_crossattn": [ctx_u.to(dev)]}
        s, _ = ld.sample_log(cond, 2, True, S, sampler="dpm_solver", x_T=xT.to(dev), unconditional_conditioning=unc,
                             unconditional_guidance_scale=1.5, **kw)
        outs[g] = s.clone()
        ac = ld.alphas_cumprod.detach().cpu()
    assert torch.equal(outs[False], outs[True])
    ou, ocfg, plan, P = _oracle_unet()
    eps = lambda x, t, cx: ou.unet_forward(P, ocfg, torch.cat([x, cc], 1), t, cx, plan=plan)
    ref = plan_sample(dpm_plan(ac, S, **kw), eps, xT, 1.5, ctx, ctx_u)
    err = rel(outs[True], ref)
    print(f"[TINY U-Net {name} + CFG 1.5] rel err vs the oracle loop {err:.3e}")
    assert err < 1e-3


# ------------------------------------------------------------------------------------------------ prediction entry points
def test_predict_latents_dpm_solver_options_and_shard_invariance(dev):
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from tests.test_gpu_masked_sampler import B_PRED, SEED_PRED, _pred_batch, _pred_model
    model = _pred_model(dev)
    batch = _pred_batch(list(range(B_PRED)), dev)
    xT = prng.normal(SEED_PRED, "p.xT", (B_PRED, 4, 16, 16)).to(dev)
    opts = dict(order=3, method="singlestep", thresholding=True, max_val=1.5)
    run = lambda **kw: predict_latents(model, batch, 6, cfg_scale=1.5, style_sampling="mp", x_T=xT, **kw)
    a = run(sampler="dpm_solver", dpm_solver=opts)
    assert a.shape == (B_PRED, 4, 16, 16) and bool(torch.isfinite(a).all())
    assert torch.equal(a, run(sampler="dpm_solver", dpm_solver=opts))
    assert not torch.equal(a, run(sampler="dpm_solver"))
    with pytest.raises(ValueError):
        run(sampler="ddim", dpm_solver=opts)
    with pytest.raises(ValueError):
        run(sampler="dpm_solver", dpm_solver={"orders": 3})
    kw = dict(style_sampling="mp", sampler="dpm_solver", dpm_solver=opts, gather=False)
    full = predict_latents_sharded(model, batch, B_PRED, 6, cfg_scale=1.5, seed=SEED_PRED, rank=0, world=1, **kw)
    parts = []
    for r in range(2):
        lo, hi = par.shard_range(B_PRED, r, 2)
        parts.append(predict_latents_sharded(model, _pred_batch(list(range(lo, hi)), dev), B_PRED, 6, cfg_scale=1.5, seed=SEED_PRED,
                                             rank=r, world=2, **kw))
    got, ref = torch.cat(parts).double().cpu(), full.double().cpu()
    per = ((got - ref).flatten(1).abs().amax(1) / ref.flatten(1).std(1)).tolist()
    print(f"[DPM-Solver singlestep-3 + thresholding predict, 2 x 2 vs 1 x 4] worst sample max|diff|/std {max(per):.3e}")
    assert max(per) < 1e-3
