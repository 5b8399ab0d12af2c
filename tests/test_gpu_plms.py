"""GPU tier (-m gpu): PLMS sampling (stedm_amd/plms.py) on the HIP path.
  * stedm_plms_step against plms_update_ref bit for bit: every phase and order, with and without CFG, a 3x3x5x7 shape off the float4
    grid, a misaligned operand, outputs aliasing the eps operands;
  * the sampler with F19's closed-form eps model on the device against F19 (the reference's own PLMSSampler), all four cases. The masked
    case m10 passes F19's q_sample noises in (mask_noises), so it runs the eager loop with the noise given; the in-kernel noise draw and
    the graphed masked loop are covered by the consistency checks below (masked graph == masked eager, zero mask == unmasked, the same
    blended latent as DDIM at iteration 0), not by F19;
  * the TINY U-Net + CFG PLMS-20 loop against ref_plms_sample over the oracle U-Net: eager, graph == eager bit for bit, fp16 / bf16;
  * masked runs: zero mask == unmasked, masked graph == masked eager, PLMS and DDIM blend the same noise at iteration 0;
  * predict_latents(sampler="plms") with and without a mask, the default staying DDIM, and shard invariance."""
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_plms_oracle import f19_case, plms_update_ref, ref_plms_sample, toy_eps

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


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (3, 3, 5, 7)])
def test_plms_step_kernel_matches_torch_bitwise(dev, shape):
    from oracle import ddim as od
    from stedm_amd import ops
    from stedm_amd.schedule import make_ddim_tables
    tb = make_ddim_tables(od.Schedule().alphas_cumprod.numpy(), 10, 0.0)
    coefs_h = torch.from_numpy(tb.coef_table())
    coefs = coefs_h.to(dev)
    n = coefs.shape[0]
    x = prng.normal(80, "k.x", shape)
    e_c = prng.normal(80, "k.ec", shape)
    e_u = prng.normal(80, "k.eu", shape)
    ring0 = prng.normal(80, "k.ring", (4,) + shape)
    N = x.numel()
    # (phase, table index): EULER and HEUN at the first row, MULTISTEP at i = 1, 2, 3 (orders 1-3), i = 6 (order 3, slots wrapped) and
    # i = 0 (order 0: a plain DDIM step)
    for phase, index in ((0, n - 1), (1, n - 1), (2, n - 2), (2, n - 3), (2, n - 4), (2, n - 7), (2, n - 1)):
        for cfg in (False, True):
            s = 1.5 if cfg else 1.0
            ring_w, x_w, tmp_w, p_w = ring0.clone(), x.clone(), torch.zeros(shape), torch.zeros(shape)
            plms_update_ref(x_w, e_c, e_u if cfg else None, ring_w, coefs_h[index], s, phase, n, index, pred_x0=p_w, x_tmp=tmp_w)
            step = torch.tensor([index], dtype=torch.int32, device=dev)
            ring, xd, tmp, pd = ring0.to(dev), x.to(dev), torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
            ops.plms_step(xd, e_c.to(dev), e_u.to(dev) if cfg else None, ring, coefs, step, n, phase, s, pred_x0=pd, x_tmp=tmp)
            assert torch.equal(ring.cpu(), ring_w), (phase, index, cfg)
            assert torch.equal(xd.cpu(), x_w) and torch.equal(tmp.cpu(), tmp_w), (phase, index, cfg)
            if phase != 0:
                assert torch.equal(pd.cpu(), p_w), (phase, index, cfg)
            # operands off the 16-byte grid (the elementwise form), and the output written over the eps operand it reads
            buf = torch.cat([torch.zeros(1), e_c.flatten(), e_u.flatten()]).to(dev)
            ec_m, eu_m = buf[1:1 + N].view(shape), buf[1 + N:].view(shape)
            ring2, xd2 = ring0.to(dev), x.to(dev)
            if phase == 0:
                ops.plms_step(xd2, ec_m, eu_m if cfg else None, ring2, coefs, step, n, phase, s, x_tmp=ec_m)
                assert torch.equal(ec_m.cpu(), tmp_w) and torch.equal(xd2.cpu(), x), (phase, cfg)
            else:
                ops.plms_step(xd2, ec_m, eu_m if cfg else None, ring2, coefs, step, n, phase, s, pred_x0=ec_m)
                assert torch.equal(xd2.cpu(), x_w) and torch.equal(ec_m.cpu(), p_w), (phase, index, cfg)
            assert torch.equal(ring2.cpu(), ring_w), (phase, index, cfg)
    with pytest.raises(ValueError):
        ops.plms_step(x.to(dev), e_c.to(dev), None, ring0.to(dev), coefs, torch.zeros(1, dtype=torch.int32, device=dev), n, 0, 1.0)
    with pytest.raises(ValueError):
        ops.plms_step(x.to(dev), e_c.to(dev), None, ring0[:3].contiguous().to(dev), coefs, torch.zeros(1, dtype=torch.int32, device=dev), n, 2)


# ------------------------------------------------------------------------------------------------ F19 through the HIP sampler
class GpuToy:
    """F19's closed-form eps model on the device with the model surface PLMSSampler reads (no apply_model_cfg: two calls per
    evaluation); records every call's timesteps."""

    def __init__(self, dev):
        from oracle import ddim as od
        s = od.Schedule()
        self.num_timesteps = 1000
        self.alphas_cumprod = s.alphas_cumprod.to(dev)
        self.sqrt_alphas_cumprod = s.sqrt_alphas_cumprod.to(dev)
        self.sqrt_one_minus_alphas_cumprod = s.sqrt_one_minus_alphas_cumprod.to(dev)
        self.device = dev
        self.ts = []

    def apply_model(self, x, t, c):
        self.ts.append(t.clone())
        return toy_eps(x, t, c)


@pytest.mark.parametrize("name", ["s20c", "s4", "s1", "m10"])
def test_f19_on_the_hip_sampler(dev, golden, name):
    from stedm_amd.plms import PLMSSampler
    c = f19_case(golden, name)
    toy = GpuToy(dev)
    cfg = c["scale"] != 1.0
    kw = dict(unconditional_guidance_scale=c["scale"], unconditional_conditioning=c["uncond"].to(dev)) if cfg else {}
    if c["mask"] is not None:
        kw.update(mask=c["mask"].to(dev), x0=c["x0"].to(dev), mask_noises=c["q_noises"])
    x, inter = PLMSSampler(toy).sample(c["S"], 2, (4, 8, 8), c["cond"].to(dev), x_T=c["xT"].to(dev),
                                       log_every_t=5 if name == "s20c" else 100, **kw)
    n_eval = c["t"].shape[0]
    assert len(toy.ts) == n_eval * (2 if cfg else 1)
    for k, t in enumerate(toy.ts):
        assert torch.equal(t.cpu(), c["t"][k // (2 if cfg else 1)].expand(2))
    err = rel(x, c["out"])
    print(f"[F19 {name} on the HIP sampler] max|diff|/std {err:.3e}")
    assert err < 1e-4
    if name == "s20c":
        assert len(inter["x_inter"]) == 6
        n = n_eval - 1
        for a, i in zip(inter["x_inter"][1:], c["log_iters"]):
            assert rel(a, c["out"] if i == n - 1 else c["call_x"][i + 2]) < 1e-4


# ------------------------------------------------------------------------------------------------ TINY U-Net loop
def _oracle_unet():
    from oracle import unet as ou
    ocfg = ou.UNetConfig(image_size=16, in_channels=7, model_channels=32, out_channels=4, channel_mult=(1, 2, 4), num_heads=4)
    plan = ou.build_plan(ocfg)
    return ou, ocfg, plan, prng.fill_state_dict(plan.shapes, 6)


def _inputs(B=2):
    return (prng.normal(81, "l.xT", (B, 4, 16, 16)), prng.normal(81, "l.cc", (B, 3, 16, 16)) * 0.5,
            prng.normal(81, "l.ctx", (B, 128)), prng.normal(81, "l.ctxu", (B, 128)))


def _plms(dev, use_graph, precision, S=20, mask=None, x0=None, mask_seed=None):
    from tests.test_gpu_sampler import make
    xT, cc, ctx, ctx_u = _inputs()
    ld = make(dev, use_graph, precision)
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    unc = {"c_concat": [cc.to(dev).clone()], "c_crossattn": [ctx_u.to(dev)]}
    kw = {} if mask is None else dict(mask=mask.to(dev), x0=x0.to(dev), mask_seed=mask_seed)
    s, inter = ld.sample_log(cond, 2, True, S, sampler="plms", x_T=xT.to(dev), unconditional_conditioning=unc,
                             unconditional_guidance_scale=1.5, log_every_t=5, **kw)
    assert isinstance(inter, dict) and len(inter["x_inter"]) == len(inter["pred_x0"])
    return s.clone(), inter


def test_tiny_unet_cfg_plms20_vs_oracle_eager_graph_and_modes(dev):
    ou, ocfg, plan, P = _oracle_unet()
    xT, cc, ctx, ctx_u = _inputs()
    eps = lambda x, t, cx: ou.unet_forward(P, ocfg, torch.cat([x, cc.repeat(x.shape[0] // cc.shape[0], 1, 1, 1)], 1), t, cx, plan=plan)
    ref, _ = ref_plms_sample(eps, xT, 20, 1.5, ctx, ctx_u)
    outs = {}
    for g in (False, True):
        outs[g], inter = _plms(dev, g, "parity")
        err = rel(outs[g], ref)
        print(f"[PLMS-20 + CFG 1.5, TINY U-Net, graph={g}] rel err vs oracle loop: {err:.3e}")
        assert err < 1e-3
        assert len(inter["x_inter"]) == 6 and torch.equal(inter["x_inter"][-1], outs[g])
    assert torch.equal(outs[False], outs[True])
    f16, _ = _plms(dev, True, "f16")
    err16 = rel(f16, ref)
    bf16, _ = _plms(dev, True, "bf16")
    l2 = float((bf16.double().cpu() - outs[True].double().cpu()).norm() / outs[True].double().cpu().norm())
    print(f"[PLMS-20 graph] f16 rel err vs oracle {err16:.3e}; bf16 vs parity rel-L2 {l2:.3e}")
    assert err16 < 1e-2 and l2 < 5e-3


# ------------------------------------------------------------------------------------------------ masked sampling
def _mask_inputs(B=2):
    x0 = prng.normal(82, "m.x0", (B, 4, 16, 16))
    mask = torch.zeros(B, 1, 16, 16)
    mask[..., :8] = 1.0                                                 # keep the left half
    return mask, x0


def test_masked_plms_zero_mask_and_graph_equal_eager(dev):
    mask, x0 = _mask_inputs()
    plain, pi = _plms(dev, True, "f16", S=5)
    zero, zi = _plms(dev, True, "f16", S=5, mask=torch.zeros_like(mask), x0=x0, mask_seed=5)
    assert torch.equal(plain, zero)
    assert all(torch.equal(a, b) for a, b in zip(pi["x_inter"], zi["x_inter"]))
    eager, _ = _plms(dev, False, "f16", S=5, mask=mask, x0=x0, mask_seed=99)
    graph, _ = _plms(dev, True, "f16", S=5, mask=mask, x0=x0, mask_seed=99)
    assert torch.equal(eager, graph)
    assert not torch.equal(graph, plain)
    other, _ = _plms(dev, True, "f16", S=5, mask=mask, x0=x0, mask_seed=100)
    assert not torch.equal(other, graph)                                # the seed reaches the replayed draw


def test_plms_and_ddim_blend_the_same_noise_at_iteration_0(dev):
    from tests.test_gpu_sampler import make
    mask, x0 = _mask_inputs()
    xT, cc, ctx, ctx_u = _inputs()
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    unc = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx_u.to(dev)]}
    first = {}
    for sampler in ("ddim", "plms"):
        ld = make(dev, False, "f16")
        inner = ld.apply_model_cfg

        def spy(x, *a, **k):
            first.setdefault(sampler, x.clone())
            return inner(x, *a, **k)

        ld.apply_model_cfg = spy
        ld.sample_log(cond, 2, True, 5, sampler=sampler, x_T=xT.to(dev), unconditional_conditioning=unc, unconditional_guidance_scale=1.5,
                      mask=mask.to(dev), x0=x0.to(dev), mask_seed=2024)
    assert torch.equal(first["ddim"], first["plms"])
    kept = mask.to(dev).expand_as(first["plms"]) == 1
    assert not torch.equal(first["plms"][kept], xT.to(dev)[kept])        # the blend ran before the first call


# ------------------------------------------------------------------------------------------------ prediction entry points
def test_predict_latents_plms_and_shard_invariance(dev):
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from tests.test_gpu_masked_sampler import B_PRED, SEED_PRED, _pred_batch, _pred_model
    model = _pred_model(dev)
    batch = _pred_batch(list(range(B_PRED)), dev)
    xT = prng.normal(SEED_PRED, "p.xT", (B_PRED, 4, 16, 16)).to(dev)
    run = lambda **kw: predict_latents(model, batch, 4, cfg_scale=1.5, style_sampling="mp", x_T=xT, **kw)
    a = run(sampler="plms")
    assert a.shape == (B_PRED, 4, 16, 16) and bool(torch.isfinite(a).all())
    assert torch.equal(a, run(sampler="plms"))
    assert not torch.equal(a, run())                                           # the default stays DDIM
    im = torch.zeros(B_PRED, 64, 64, device=dev)
    im[:, :, :32] = 1.0
    m = run(sampler="plms", mask=im, mask_seed=7)
    assert bool(torch.isfinite(m).all()) and not torch.equal(m, a)
    with pytest.raises(ValueError):
        run(sampler="plms", eta=0.5)
    with pytest.raises(NotImplementedError):
        run(sampler="plms", noises=[xT] * 4)
    full = predict_latents_sharded(model, batch, B_PRED, 4, cfg_scale=1.5, seed=SEED_PRED, rank=0, world=1, gather=False,
                                   style_sampling="mp", sampler="plms", mask=im)
    parts = []
    for r in range(2):
        lo, hi = par.shard_range(B_PRED, r, 2)
        parts.append(predict_latents_sharded(model, _pred_batch(list(range(lo, hi)), dev), B_PRED, 4, cfg_scale=1.5, seed=SEED_PRED,
                                             rank=r, world=2, gather=False, style_sampling="mp", sampler="plms", mask=im))
    got = torch.cat(parts).double().cpu()
    ref = full.double().cpu()
    per = ((got - ref).flatten(1).abs().amax(1) / ref.flatten(1).std(1)).tolist()
    print(f"[PLMS predict (masked), 2 x 2 vs 1 x 4, parity] worst sample max|diff|/std {max(per):.3e}")
    assert max(per) < 1e-3
