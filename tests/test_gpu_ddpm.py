"""GPU tier (-m gpu): ancestral DDPM sampling (stedm_amd/ancestral.py) on the HIP path.
  * stedm_ddpm_step against ddpm_update_ref bit for bit: a shape off the float4 grid (HW % 4 != 0), B = 1, [16, 3, 128, 128]; clamp on
    and off; t = 0 and t > 0; noise given, and the in-kernel draw equal to ops.philox_normal at stream 0x10000 + t; the fused mask blend
    equal to the step followed by ops.ddim_mask_blend bit for bit, with a broadcast mask (that kernel's compiled arithmetic fuses one
    product of each sum into an FMA, so the blended elements agree with torch's unfused expression to an ulp); an operand off the
    16-byte grid at HW % 4 == 0 (the scalar form chosen by the alignment test) gives the aligned call's bits in stedm_ddpm_step,
    stedm_ddpm_step_ex and stedm_ddim_mask_blend; the three wrappers refuse the same bad mask operands;
  * the sampler with F20's closed-form eps model on the device and F20's recorded noise against F20 (the reference's own chain);
  * the TINY U-Net, timesteps = 50, against ref_ddpm_sample over the oracle U-Net with the kernel's noise: parity, f16 and bf16;
    graphed equal to eager bit for bit;
  * masked runs: a zero mask equals the unmasked run bit for bit, graphed equals eager;
  * predict_latents(sampler="ddpm") end to end, and two shards against the unsharded run per sample."""
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_ddpm_oracle import BUFFERS, SHAPE, ddpm_update_ref, f20_buffers, f20_case, ref_ddpm_sample, toy_eps

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


def _table():
    from stedm_amd.schedule import PosteriorSchedule, ddpm_step_table
    ps = PosteriorSchedule.make(1000, 0.0015, 0.0205)
    return torch.from_numpy(ddpm_step_table(ps.sqrt_recip_alphas_cumprod, ps.sqrt_recipm1_alphas_cumprod, ps.posterior_mean_coef1,
                                            ps.posterior_mean_coef2, ps.posterior_log_variance_clipped))


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 4, 8, 8), (16, 3, 128, 128)])
def test_ddpm_step_kernel_matches_torch_bitwise(dev, shape):
    from oracle import ddim as od
    from stedm_amd import ops
    tab = _table()
    tab_d = tab.to(dev)
    s = od.Schedule()
    sa, s1 = s.sqrt_alphas_cumprod.to(dev), s.sqrt_one_minus_alphas_cumprod.to(dev)
    B = shape[0]
    x = prng.normal(90, "k.x", shape) * 1.5          # x0 leaves [-1, 1] often: the clamp matters
    e = prng.normal(90, "k.e", shape)
    z = prng.normal(90, "k.z", shape)
    zb = prng.normal(90, "k.zb", shape)
    x0 = prng.normal(90, "k.x0", shape)
    masks = [(prng.uniform(90, "k.m", (B, 1) + shape[2:]) > 0).float(), prng.uniform(90, "k.mb", (1, shape[1]) + shape[2:], lo=0., hi=1.)]
    seed, first = 1234, 7
    for t in (0, 1, 537, 999):
        step = torch.tensor([t], dtype=torch.int32, device=dev)
        for clip in (True, False):
            # noise given
            want = ddpm_update_ref(x.clone(), e, tab[t], clip, z)
            got = ops.ddpm_step(x.to(dev), e.to(dev), tab_d, step, clip, noise=z.to(dev))
            assert torch.equal(got.cpu(), want), (t, clip)
            # the in-kernel draw: row first + b of philox_normal, stream 0x10000 + t
            zk = ops.philox_normal(B, shape[1:], seed, 0x10000 + t, dev, first_id=first)
            want_k = ddpm_update_ref(x.clone(), e, tab[t], clip, zk.cpu())
            got_k = ops.ddpm_step(x.to(dev), e.to(dev), tab_d, step, clip, seed=seed, first_id=first)
            assert torch.equal(got_k.cpu(), want_k), (t, clip)
            for m in masks:
                # fused blend == step, then ddim_mask_blend at index t (both draws in the kernel)
                fused = ops.ddpm_step(x.to(dev), e.to(dev), tab_d, step, clip, seed=seed, first_id=first, mask=m.to(dev), x0=x0.to(dev),
                                      mask_seed=99, sqrt_ac=sa, sqrt_1mac=s1)
                two = ops.ddpm_step(x.to(dev), e.to(dev), tab_d, step, clip, seed=seed, first_id=first)
                ops.ddim_mask_blend(two, x0.to(dev), m.to(dev), torch.full((B,), t, dtype=torch.int64, device=dev), sa, s1, step_idx=step,
                                    seed=99, first_id=first)
                assert torch.equal(fused, two), (t, clip, tuple(m.shape))
                # given blend noise against torch: the blend rounds as stedm_ddim_mask_blend's compiled code (one FMA per sum), so it
                # agrees with torch's unfused expression to an ulp, and bit for bit where the mask is 0 (the step's own result)
                want_m = ddpm_update_ref(x.clone(), e, tab[t], clip, z, mask=m, x0=x0, zb=zb, ca=s.sqrt_alphas_cumprod[t],
                                         cn=s.sqrt_one_minus_alphas_cumprod[t])
                got_m = ops.ddpm_step(x.to(dev), e.to(dev), tab_d, step, clip, noise=z.to(dev), mask=m.to(dev), x0=x0.to(dev),
                                      mask_noise=zb.to(dev), sqrt_ac=sa, sqrt_1mac=s1).cpu()
                off = m.expand(shape) == 0
                assert torch.equal(got_m[off], want_m[off]) and torch.equal(got_m[off], want[off]), (t, clip, tuple(m.shape))
                assert float((got_m - want_m).abs().max()) <= 4e-7 * float(want_m.abs().max()), (t, clip, tuple(m.shape))
    # a step index outside the table writes nothing
    xd = x.to(dev)
    ops.ddpm_step(xd, e.to(dev), tab_d, torch.tensor([1000], dtype=torch.int32, device=dev), True, noise=z.to(dev))
    assert torch.equal(xd.cpu(), x)
    with pytest.raises(ValueError):
        ops.ddpm_step(x.to(dev), e.to(dev), tab_d[:, :4].contiguous(), step)
    with pytest.raises(ValueError):
        ops.ddpm_step(x.to(dev), e.to(dev), tab_d, step, mask=masks[0].to(dev))


def _off16(src, dev):
    """src on the device as a contiguous view one float into a larger buffer: 4 bytes past a 16-byte boundary"""
    buf = torch.empty(src.numel() + 1, device=dev)
    v = buf[1:].view(src.shape)
    v.copy_(src)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_misaligned_operand_takes_the_scalar_form_with_the_same_bits(dev):
    """HW % 4 == 0 with one operand off the 16-byte grid: the entries' alignment test, not the shape, selects the scalar form."""
    from oracle import ddim as od
    from stedm_amd import ops
    shape = (2, 4, 8, 8)
    tab = _table()
    tab_d = tab.to(dev)
    s = od.Schedule()
    sa, s1 = s.sqrt_alphas_cumprod.to(dev), s.sqrt_one_minus_alphas_cumprod.to(dev)
    x, e, z = prng.normal(93, "a.x", shape) * 1.5, prng.normal(93, "a.e", shape), prng.normal(93, "a.z", shape)
    zb, x0 = prng.normal(93, "a.zb", shape), prng.normal(93, "a.x0", shape)
    m = prng.uniform(93, "a.m", (1, 1, 8, 8), lo=0., hi=1.).to(dev)
    on = lambda v: v.to(dev)
    for t in (0, 537):
        step = torch.tensor([t], dtype=torch.int32, device=dev)
        want = ddpm_update_ref(x.clone(), e, tab[t], True, z)
        mk = dict(mask=m, x0=on(x0), mask_noise=on(zb), sqrt_ac=sa, sqrt_1mac=s1)
        want_m = ops.ddpm_step(on(x), on(e), tab_d, step, True, noise=on(z), **mk)
        for which in ("x", "eps"):
            xd = lambda: _off16(x, dev) if which == "x" else on(x)
            ed = _off16(e, dev) if which == "eps" else on(e)
            assert torch.equal(ops.ddpm_step(xd(), ed, tab_d, step, True, noise=on(z)).cpu(), want), (t, which)
            assert torch.equal(ops.ddpm_step(xd(), ed, tab_d, step, True, noise=on(z), **mk), want_m), (t, which)
        out = _off16(torch.zeros(shape), dev)
        ops.ddpm_step_ex(on(x), on(e), tab_d, step_idx=step, noise=on(z), x_out=out, **mk)
        assert torch.equal(out, want_m), t
        tb = torch.full((2,), t, dtype=torch.int64, device=dev)
        blend = lambda img: ops.ddim_mask_blend(img, on(x0), m, tb, sa, s1, noise=on(zb))
        assert torch.equal(blend(_off16(x, dev)), blend(on(x))), t


def test_mask_operand_checks_are_the_same_in_the_three_wrappers(dev):
    from oracle import ddim as od
    from stedm_amd import ops
    shape = (2, 4, 8, 8)
    tab = _table().to(dev)
    s = od.Schedule()
    sa, s1 = s.sqrt_alphas_cumprod.to(dev), s.sqrt_one_minus_alphas_cumprod.to(dev)
    x, e, x0 = (torch.zeros(shape, device=dev) for _ in range(3))
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    tb = torch.zeros(2, dtype=torch.int64, device=dev)
    good = dict(mask=torch.ones((1, 1, 8, 8), device=dev), x0=x0, sqrt_ac=sa, sqrt_1mac=s1)
    calls = {"ddpm_step": lambda **kw: ops.ddpm_step(x, e, tab, step, **kw),
             "ddpm_step_ex": lambda **kw: ops.ddpm_step_ex(x, e, tab, step_idx=step, x_out=x, **kw),
             "ddim_mask_blend": lambda **kw: ops.ddim_mask_blend(x, kw["x0"], kw["mask"], tb, kw["sqrt_ac"], kw["sqrt_1mac"], step_idx=step)}
    bad = {"mask rank": dict(mask=torch.ones((1, 8, 8), device=dev)), "mask batch": dict(mask=torch.ones((3, 1, 8, 8), device=dev)),
           "mask plane": dict(mask=torch.ones((1, 1, 8, 4), device=dev)), "no x0": dict(x0=None), "no sqrt_ac": dict(sqrt_ac=None),
           "no sqrt_1mac": dict(sqrt_1mac=None)}
    for call in calls.values():
        call(**good)
        for kw in bad.values():
            with pytest.raises(ValueError):
                call(**{**good, **kw})
    for name in ("ddpm_step", "ddpm_step_ex"):                    # the blend has no step table: its t indexes the buffers directly
        for kw in (dict(sqrt_ac=sa[:999].contiguous()), dict(sqrt_1mac=s1[:999].contiguous())):
            with pytest.raises(ValueError):
                calls[name](**{**good, **kw})


# ------------------------------------------------------------------------------------------------ F20 through the HIP sampler
class GpuToy:
    """F20's closed-form eps model on the device with the surface AncestralSampler reads; records every call's t."""

    def __init__(self, dev, clip):
        from oracle import ddim as od
        from stedm_amd.schedule import PosteriorSchedule
        s = od.Schedule()
        ps = PosteriorSchedule.make(1000, 0.0015, 0.0205)
        for b in BUFFERS:
            setattr(self, b, torch.from_numpy(getattr(ps, b)).to(dev))
        self.sqrt_alphas_cumprod = s.sqrt_alphas_cumprod.to(dev)
        self.sqrt_one_minus_alphas_cumprod = s.sqrt_one_minus_alphas_cumprod.to(dev)
        self.num_timesteps, self.clip_denoised, self.log_every_t = 1000, clip, 100
        self.channels, self.image_size = 4, 8
        self.device = dev
        self.ts = []

    def apply_model(self, x, t, c):
        self.ts.append(t)
        return toy_eps(x, t, c)


@pytest.mark.parametrize("name", ["full", "short", "masked"])
def test_f20_on_the_hip_sampler(dev, golden, name):
    from stedm_amd.ancestral import AncestralSampler
    c = f20_case(golden, name)
    toy = GpuToy(dev, c["clip"])
    kw = {} if c["mask"] is None else dict(mask=c["mask"].to(dev), x0=c["x0"].to(dev), mask_noises=c["q_noises"])
    x, inter = AncestralSampler(toy).sample(c["cond"].to(dev), 2, return_intermediates=True, x_T=c["xT"].to(dev),
                                            timesteps=None if name == "full" else c["T"], noises=c["noises"], **kw)
    assert [int(t[0]) for t in toy.ts] == list(range(c["T"] - 1, -1, -1))
    err = rel(x, c["out"])
    print(f"[F20 {name} on the HIP sampler] max|diff|/std {err:.3e}")
    assert err < 1e-4
    assert len(inter) == c["n_inter"]
    if name == "full":
        assert max(rel(a, b) for a, b in zip(inter, c["inter"])) < 1e-4


# ------------------------------------------------------------------------------------------------ TINY U-Net loop
def _oracle_unet():
    from oracle import unet as ou
    ocfg = ou.UNetConfig(image_size=16, in_channels=7, model_channels=32, out_channels=4, channel_mult=(1, 2, 4), num_heads=4)
    plan = ou.build_plan(ocfg)
    return ou, ocfg, plan, prng.fill_state_dict(plan.shapes, 6)


def _inputs(B=2):
    return prng.normal(91, "l.xT", (B, 4, 16, 16)), prng.normal(91, "l.cc", (B, 3, 16, 16)) * 0.5, prng.normal(91, "l.ctx", (B, 128))


T_TINY, SEED_TINY = 50, 4242


def _ddpm(dev, use_graph, precision, mask=None, x0=None, mask_seed=None):
    from tests.test_gpu_sampler import make
    xT, cc, ctx = _inputs()
    ld = make(dev, use_graph, precision)
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    kw = {} if mask is None else dict(mask=mask.to(dev), x0=x0.to(dev), mask_seed=mask_seed)
    s, inter = ld.sample_log(cond, 2, False, 0, x_T=xT.to(dev), timesteps=T_TINY, noise_seed=SEED_TINY, **kw)
    assert isinstance(inter, list) and len(inter) == 3          # x_T, t = 49, t = 0 (log_every_t 100)
    return s.clone(), inter


def test_tiny_unet_ddpm50_vs_oracle_eager_graph_and_modes(dev, golden):
    from stedm_amd import ops
    ou, ocfg, plan, P = _oracle_unet()
    xT, cc, ctx = _inputs()
    eps = lambda x, t, cx: ou.unet_forward(P, ocfg, torch.cat([x, cc], 1), t, cx, plan=plan)
    noises = [ops.philox_normal(2, (4, 16, 16), SEED_TINY, 0x10000 + (T_TINY - 1 - k), dev).cpu() for k in range(T_TINY)]
    ref, _ = ref_ddpm_sample(eps, xT, T_TINY, f20_buffers(golden), True, ctx, noises)
    outs = {}
    for g in (False, True):
        outs[g], inter = _ddpm(dev, g, "parity")
        err = rel(outs[g], ref)
        print(f"[DDPM-{T_TINY}, TINY U-Net, graph={g}] rel err vs oracle loop: {err:.3e}")
        assert err < 1e-3
        assert torch.equal(inter[-1], outs[g])
    assert torch.equal(outs[False], outs[True])
    f16, _ = _ddpm(dev, True, "f16")
    e16, _ = _ddpm(dev, False, "f16")
    assert torch.equal(e16, f16)
    err16 = rel(f16, ref)
    bf16, _ = _ddpm(dev, True, "bf16")
    l2 = float((bf16.double().cpu() - outs[True].double().cpu()).norm() / outs[True].double().cpu().norm())
    print(f"[DDPM-{T_TINY} graph] f16 rel err vs oracle {err16:.3e}; bf16 vs parity rel-L2 {l2:.3e}")
    assert err16 < 2e-2 and l2 < 2e-2


# ------------------------------------------------------------------------------------------------ masked sampling
def test_masked_ddpm_zero_mask_and_graph_equal_eager(dev):
    x0 = prng.normal(92, "m.x0", (2, 4, 16, 16))
    mask = torch.zeros(2, 1, 16, 16)
    mask[..., :8] = 1.0
    plain, pi = _ddpm(dev, True, "f16")
    zero, zi = _ddpm(dev, True, "f16", mask=torch.zeros_like(mask), x0=x0, mask_seed=5)
    assert torch.equal(plain, zero) and all(torch.equal(a, b) for a, b in zip(pi, zi))
    eager, _ = _ddpm(dev, False, "f16", mask=mask, x0=x0, mask_seed=99)
    graph, _ = _ddpm(dev, True, "f16", mask=mask, x0=x0, mask_seed=99)
    assert torch.equal(eager, graph)
    assert not torch.equal(graph, plain)
    other, _ = _ddpm(dev, True, "f16", mask=mask, x0=x0, mask_seed=100)
    assert not torch.equal(other, graph)                                # the seed reaches the replayed draw


# ------------------------------------------------------------------------------------------------ prediction entry points
def test_predict_latents_ddpm_and_shard_invariance(dev):
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from tests.test_gpu_masked_sampler import B_PRED, SEED_PRED, _pred_batch, _pred_model
    model = _pred_model(dev)
    batch = _pred_batch(list(range(B_PRED)), dev)
    xT = prng.normal(SEED_PRED, "p.xT", (B_PRED, 4, 16, 16)).to(dev)
    run = lambda **kw: predict_latents(model, batch, 4, cfg_scale=1.0, style_sampling="mp", x_T=xT, **kw)
    a = run(sampler="ddpm", noise_seed=3)
    assert a.shape == (B_PRED, 4, 16, 16) and bool(torch.isfinite(a).all())
    assert torch.equal(a, run(sampler="ddpm", noise_seed=3))
    assert not torch.equal(a, run(sampler="ddpm", noise_seed=4))
    assert not torch.equal(a, run())                                           # the default stays DDIM
    with pytest.raises(NotImplementedError):
        predict_latents(model, batch, 4, cfg_scale=1.5, style_sampling="mp", sampler="ddpm")
    kw = dict(cfg_scale=1.0, seed=SEED_PRED, gather=False, style_sampling="mp", sampler="ddpm")
    full = predict_latents_sharded(model, batch, B_PRED, 4, rank=0, world=1, **kw)
    parts = []
    for r in range(2):
        lo, hi = par.shard_range(B_PRED, r, 2)
        parts.append(predict_latents_sharded(model, _pred_batch(list(range(lo, hi)), dev), B_PRED, 4, rank=r, world=2, **kw))
    got = torch.cat(parts).double().cpu()
    ref = full.double().cpu()
    per = ((got - ref).flatten(1).abs().amax(1) / ref.flatten(1).std(1)).tolist()
    same = sum(bool(torch.equal(got[i], ref[i])) for i in range(B_PRED))
    print(f"[DDPM predict, 2 x 2 vs 1 x 4, parity] worst sample max|diff|/std {max(per):.3e}; bitwise equal samples {same}/{B_PRED}")
    assert max(per) < 1e-3
