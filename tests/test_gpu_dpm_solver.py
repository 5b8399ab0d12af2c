"""GPU tier (-m gpu): DPM-Solver++(2M) sampling (stedm_amd/dpm_solver.py) on the HIP path.
  * stedm_dpm_step against its fp32 torch restatement (first, middle and final-order rows, with and without CFG, a 3x3x5x7 shape off the
    float4 grid, a misaligned operand, in-place aliasing);
  * the fp32-timestep time embedding against the oracle at fractional t; integer-valued float t gives the int64 path's bits;
  * the TINY U-Net at fractional timesteps against oracle.unet.unet_forward;
  * the sampler with F18's closed-form eps model against F18 (the reference's own DPMSolverSampler);
  * the TINY U-Net + CFG DPM-20 loop against the CPU restatement over the oracle U-Net, eager and hipGraph replay, graph == eager bit
    for bit, the fp16 / bf16 modes within the DDIM tests' budgets;
  * predict_latents(sampler="dpm_solver") end to end, and shard invariance of predict_latents_sharded."""
import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_dpm_solver_oracle import dpm_update_ref, f18_case, ref_dpm_sample, toy_eps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (3, 3, 5, 7)])
def test_dpm_step_kernel_matches_torch(dev, shape):
    from stedm_amd import ops
    from stedm_amd.dpm_solver import dpm_tables
    from oracle import ddim as od
    tb = dpm_tables(od.Schedule().alphas_cumprod, 5)            # rows 0 (first order), 2 (second order), 4 (first-order final step)
    coefs = tb.coefs.to(dev)
    x = prng.normal(70, "k.x", shape)
    e_c = prng.normal(70, "k.ec", shape)
    e_u = prng.normal(70, "k.eu", shape)
    x0_prev = prng.normal(70, "k.x0p", shape)
    worst, bitwise = 0.0, True
    for row in (0, 2, 4):
        for cfg in (False, True):
            s = 1.5 if cfg else 1.0
            want_x, want_x0 = dpm_update_ref(x, e_c, e_u if cfg else None, x0_prev, tb.coefs[row], s)
            xd = x.to(dev)
            pd = x0_prev.to(dev) if row != 0 else torch.full(shape, float("nan"), device=dev)    # a first-order row never reads x0_prev
            pred = torch.empty(shape, device=dev)
            step = torch.tensor([row], dtype=torch.int32, device=dev)
            ops.dpm_step(xd, e_c.to(dev), e_u.to(dev) if cfg else None, pd, coefs, step_idx=step, cfg_scale=s, pred_x0=pred)
            for got, want in ((xd, want_x), (pd, want_x0), (pred, want_x0)):
                err = float((got.cpu() - want).abs().max() / want.abs().max())
                worst = max(worst, err)
                bitwise = bitwise and torch.equal(got.cpu(), want)
                assert err <= 1e-6, (row, cfg, err)
            # in place with pred_x0 aliasing x0_prev, and e_u a slice off the 16-byte grid (the elementwise form)
            buf = torch.cat([torch.zeros(1), e_c.flatten(), e_u.flatten()]).to(dev)
            n = x.numel()
            ec_m, eu_m = buf[1:1 + n].view(shape), buf[1 + n:].view(shape)
            xd2 = x.to(dev)
            pd2 = x0_prev.to(dev)
            ops.dpm_step(xd2, ec_m, eu_m if cfg else None, pd2, coefs, step_idx=step, cfg_scale=s, pred_x0=pd2)
            assert torch.equal(xd2, xd) and torch.equal(pd2, pred), (row, cfg)
    print(f"[stedm_dpm_step {shape}] worst max|diff|/max|ref| vs torch {worst:.3e}, bit for bit: {bitwise}")


# ------------------------------------------------------------------------------------------------ fractional timesteps
def _tiny_unet(dev, precision="parity"):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, **TINY).eval()
    prng.fill_module_(m, seed=6)
    return m.to(dev)


def _oracle_unet():
    from oracle import unet as ou
    ocfg = ou.UNetConfig(image_size=16, in_channels=7, model_channels=32, out_channels=4, channel_mult=(1, 2, 4), num_heads=4)
    plan = ou.build_plan(ocfg)
    return ou, ocfg, plan, prng.fill_state_dict(plan.shapes, 6)


def test_float_time_embedding_vs_oracle_and_int_bits(dev):
    from oracle import unet as ou
    from stedm_amd import ops
    m = _tiny_unet(dev)
    m._prepare()
    c = m._consts
    mc, ted = 32, 128
    run = lambda t: ops.time_embed(t, c["freqs"], c["te_w0t"], c["te_b0"], c["te_w2t"], c["te_b2"], torch.empty((t.shape[0], ted), device=dev))
    t = torch.tensor([949.05, 0.5, 998.001, 17.25], dtype=torch.float32)
    got = run(t.to(dev)).cpu()
    te = ou.timestep_embedding(t, mc)
    l0, l2 = m.time_embed[0], m.time_embed[2]
    h = torch.nn.functional.silu(te @ l0.weight.detach().cpu().T + l0.bias.detach().cpu())
    want = h @ l2.weight.detach().cpu().T + l2.bias.detach().cpu()
    err = float((got - want).abs().max() / want.abs().max())
    print(f"[time_embed_f32 at fractional t] max|diff|/max|ref| vs oracle {err:.3e}")
    assert err < 1e-5
    ti = torch.tensor([0, 3, 501, 999], dtype=torch.int64, device=dev)
    assert torch.equal(run(ti.float()), run(ti))
    with pytest.raises(TypeError):
        run(ti.to(torch.float64))


def test_tiny_unet_at_fractional_timesteps_vs_oracle(dev):
    ou, ocfg, plan, P = _oracle_unet()
    m = _tiny_unet(dev)
    x = prng.normal(71, "u.x", (2, 7, 16, 16))
    ctx = prng.normal(71, "u.ctx", (2, 128))
    t = torch.tensor([949.05, 0.5], dtype=torch.float32)
    got = m(x.to(dev), t.to(dev), context=ctx.to(dev)).cpu()
    ref = ou.unet_forward(P, ocfg, x, t, ctx, plan=plan)
    err = rel(got, ref)
    trunc = rel(ou.unet_forward(P, ocfg, x, t.long(), ctx, plan=plan), ref)
    print(f"[TINY U-Net at t = 949.05, 0.5] rel err vs oracle {err:.3e} (truncated t would be off by {trunc:.3e})")
    assert err < 1e-3 and trunc > 5 * err
    # uniform_t (the samplers' path): the embedding row evaluated once at a fractional t
    tu = torch.full((2,), 949.05, dtype=torch.float32)
    got_u = m.forward_parts(x[:, :4].contiguous().to(dev), x[:, 4:].contiguous().to(dev), tu.to(dev), ctx.to(dev), uniform_t=True).cpu()
    assert rel(got_u, ou.unet_forward(P, ocfg, x, tu, ctx, plan=plan)) < 1e-3


# ------------------------------------------------------------------------------------------------ F18 through the HIP sampler
class GpuToy:
    """F18's closed-form eps model on the device with the model surface DPMSolverSampler reads; records every call's model time."""

    def __init__(self, dev, ac):
        self.num_timesteps = 1000
        self.alphas_cumprod = ac.to(dev)
        self.parameterization = "eps"
        self.device = dev
        self.ts = []

    def apply_model(self, x, t, c):
        self.ts.append(t.clone())
        return toy_eps(x, t, c["bias"])


@pytest.mark.parametrize("name", ["s20", "s5", "s2"])
def test_f18_on_the_hip_sampler(dev, golden, name):
    from stedm_amd.dpm_solver import DPMSolverSampler
    c = f18_case(golden, name)
    toy = GpuToy(dev, c["ac"])
    cfg = c["scale"] != 1.0
    kw = dict(unconditional_guidance_scale=c["scale"], unconditional_conditioning={"bias": c["uncond"].to(dev)}) if cfg else {}
    seen = []
    x, none = DPMSolverSampler(toy, device=dev).sample(c["S"], 2, (4, 8, 8), {"bias": c["cond"].to(dev)}, x_T=c["xT"].to(dev),
                                                       img_callback=lambda p, i: seen.append(i), **kw)
    assert none is None and seen == list(range(c["S"]))
    assert len(toy.ts) == c["S"] * (2 if cfg else 1)
    for k, t in enumerate(toy.ts):
        assert t.dtype == torch.float32 and torch.equal(t.cpu(), c["t"][k // (2 if cfg else 1)].expand(2))
    err = rel(x, c["out"])
    print(f"[F18 {name} on the HIP sampler] max|diff|/std {err:.3e}")
    assert err < 1e-4


# ------------------------------------------------------------------------------------------------ TINY U-Net loop
def _ld(dev, use_graph, precision="parity"):
    from stedm_amd.latent_diffusion import LatentDiffusion
    ld = LatentDiffusion(_tiny_unet(dev, precision), linear_start=0.0015, linear_end=0.0205, image_size=16, channels=4,
                         conditioning_key="hybrid", loss_type="l1", use_graph=use_graph)
    return ld.to(dev)


def _inputs(B=2):
    return (prng.normal(72, "l.xT", (B, 4, 16, 16)), prng.normal(72, "l.cc", (B, 3, 16, 16)) * 0.5,
            prng.normal(72, "l.ctx", (B, 128)), prng.normal(72, "l.ctxu", (B, 128)))


_REF = {}


def _oracle_dpm20(ac):
    if "ref" not in _REF:
        ou, ocfg, plan, P = _oracle_unet()
        xT, cc, ctx, ctx_u = _inputs()
        eps = lambda x, t, cx: ou.unet_forward(P, ocfg, torch.cat([x, cc.repeat(x.shape[0] // cc.shape[0], 1, 1, 1)], 1), t, cx, plan=plan)
        _REF["ref"] = ref_dpm_sample(eps, xT, ac, 20, 1.5, ctx, ctx_u)
    return _REF["ref"]


def _dpm20(dev, use_graph, precision):
    ld = _ld(dev, use_graph, precision)
    xT, cc, ctx, ctx_u = _inputs()
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    unc = {"c_concat": [cc.to(dev).clone()], "c_crossattn": [ctx_u.to(dev)]}     # equal content, different storage
    s, none = ld.sample_log(cond, 2, True, 20, sampler="dpm_solver", x_T=xT.to(dev), unconditional_conditioning=unc,
                            unconditional_guidance_scale=1.5)
    assert none is None
    return s.clone(), ld.alphas_cumprod.detach().cpu()


def test_tiny_unet_cfg_dpm20_vs_oracle_eager_graph_and_modes(dev):
    outs = {}
    for g in (False, True):
        outs[g], ac = _dpm20(dev, g, "parity")
        ref = _oracle_dpm20(ac)
        err = rel(outs[g], ref)
        print(f"[DPM-20 + CFG 1.5, TINY U-Net, graph={g}] rel err vs oracle loop: {err:.3e}")
        assert err < 1e-3
    assert torch.equal(outs[False], outs[True])
    f16, _ = _dpm20(dev, True, "f16")
    err16 = rel(f16, ref)
    bf16, _ = _dpm20(dev, True, "bf16")
    l2 = float((bf16.double().cpu() - outs[True].double().cpu()).norm() / outs[True].double().cpu().norm())
    print(f"[DPM-20 graph] f16 rel err vs oracle {err16:.3e}; bf16 vs parity rel-L2 {l2:.3e}")
    assert err16 < 1e-2 and l2 < 5e-3
    e16, _ = _dpm20(dev, False, "f16")
    assert torch.equal(e16, f16)


# ------------------------------------------------------------------------------------------------ prediction entry points
def test_predict_latents_dpm_solver_and_shard_invariance(dev):
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from tests.test_gpu_masked_sampler import B_PRED, SEED_PRED, _pred_batch, _pred_model
    model = _pred_model(dev)
    batch = _pred_batch(list(range(B_PRED)), dev)
    xT = prng.normal(SEED_PRED, "p.xT", (B_PRED, 4, 16, 16)).to(dev)
    run = lambda **kw: predict_latents(model, batch, 6, cfg_scale=1.5, style_sampling="mp", x_T=xT, **kw)
    a = run(sampler="dpm_solver")
    assert a.shape == (B_PRED, 4, 16, 16) and bool(torch.isfinite(a).all())
    assert torch.equal(a, run(sampler="dpm_solver"))
    assert not torch.equal(a, run())                                           # the default stays DDIM
    with pytest.raises(NotImplementedError):
        run(sampler="dpm_solver", eta=0.5)
    with pytest.raises(ValueError):
        run(sampler="euler")
    full = predict_latents_sharded(model, batch, B_PRED, 6, cfg_scale=1.5, seed=SEED_PRED, rank=0, world=1, gather=False,
                                   style_sampling="mp", sampler="dpm_solver")
    parts = []
    for r in range(2):
        lo, hi = par.shard_range(B_PRED, r, 2)
        parts.append(predict_latents_sharded(model, _pred_batch(list(range(lo, hi)), dev), B_PRED, 6, cfg_scale=1.5, seed=SEED_PRED,
                                             rank=r, world=2, gather=False, style_sampling="mp", sampler="dpm_solver"))
    got = torch.cat(parts).double().cpu()
    ref = full.double().cpu()
    per = ((got - ref).flatten(1).abs().amax(1) / ref.flatten(1).std(1)).tolist()
    print(f"[DPM-Solver predict, 2 x 2 vs 1 x 4, parity] worst sample max|diff|/std {max(per):.3e}")
    assert max(per) < 1e-3
