"""GPU tier (-m gpu): the ancestral step with options (stedm_ddpm_step_ex) and what runs on it: progressive_denoising, quantize_denoised,
p_sample / p_mean_variance (stedm_amd/ancestral.py, LatentDiffusion).
Kernel, at [3, 4, 32, 32] (float4 form), [2, 3, 40, 40] and [2, 4, 8, 8], t in {0, 1, 500, 999}, clamp on and off, t from the device
counter and per sample:
  * options off: stedm_ddpm_step's bits; the in-kernel draw: the given-noise path fed ops.philox_normal at stream 0x10000 + t;
  * temperature and dropout: the noise term ((z T) keep) scale from the numpy keep mask bit for bit (a table row {0, 0, 0, 0, 1} makes the
    sample the noise term itself; with the schedule's rows the sample equals mean_out + sigma n bit for bit), the sample within
    4e-7 max|ref| of the torch restatement (the bound of test_gpu_ddpm.py:86 / test_gpu_ddim_options.py:112);
  * quantisation: indices and x0 equal to ops.vq_nearest on the clamped x0 bit for bit, with duplicated rows and latents on entries;
  * the mask blend: stedm_ddpm_step's bits; the kept fraction at batch 64 within 5 binomial standard deviations;
  * a t outside the table writes nothing for that sample.
Loops: graphed equal to eager bit for bit (plain, masked, quantised; parity and f16); F25 through the HIP sampler; the tiny U-Net against
the CPU oracle loop fed the kernel's noises and keep masks; shard invariance; LatentDiffusion's single steps against F25 (d)."""
import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_ddim_options_oracle import drop_scale, keep_mask
from tests.test_ddpm_oracle import F20_TOL, f20_buffers, rel_max, toy_eps
from tests.test_progressive_oracle import SEED as F25_SEED
from tests.test_progressive_oracle import SHAPE as F25_SHAPE
from tests.test_progressive_oracle import f25_case, kernel_keeps, ref_progressive

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(3, 4, 32, 32), (2, 3, 40, 40), (2, 4, 8, 8)]
TS = (0, 1, 500, 999)
K_SEED, K_FIRST = 1234, 7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sched(dev):
    """(the step table, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod) on the device, built once"""
    from oracle import ddim as od
    from tests.test_gpu_ddpm import _table
    s = od.Schedule()
    return _table().to(dev), s.sqrt_alphas_cumprod.to(dev), s.sqrt_one_minus_alphas_cumprod.to(dev)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.std())


def _ops(dev, shape, tag="k"):
    g = lambda n, s=1.0: (prng.normal(95, f"{tag}.{n}.{shape}", shape) * s).to(dev)
    return g("x", 1.5), g("e"), g("z")          # x0 leaves [-1, 1] often: the clamp matters


def _t_forms(dev, B, t):
    """the two ways to name the timestep: the device counter, and one (equal) entry per sample"""
    return [dict(step_idx=torch.tensor([t], dtype=torch.int32, device=dev)), dict(t=torch.full((B,), t, dtype=torch.int64, device=dev))]


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("shape", SHAPES)
def test_options_off_equals_ddpm_step_and_the_draw_equals_philox_rows(dev, sched, shape):
    from stedm_amd import ops
    tab, sa, s1 = sched
    B = shape[0]
    x, e, z = _ops(dev, shape)
    for t in TS:
        step = torch.tensor([t], dtype=torch.int32, device=dev)
        zk = ops.philox_normal(B, shape[1:], K_SEED, 0x10000 + t, dev, first_id=K_FIRST)
        for clip in (True, False):
            want = ops.ddpm_step(x.clone(), e, tab, step, clip, noise=z)
            want_k = ops.ddpm_step(x.clone(), e, tab, step, clip, seed=K_SEED, first_id=K_FIRST)
            for tf in _t_forms(dev, B, t):
                got = torch.empty_like(x)
                ops.ddpm_step_ex(x, e, tab, clip_denoised=clip, noise=z, x_out=got, **tf)
                assert torch.equal(got, want), (t, clip, list(tf))
                inplace = x.clone()
                ops.ddpm_step_ex(inplace, e, tab, clip_denoised=clip, noise=z, x_out=inplace, **tf)
                assert torch.equal(inplace, want), (t, clip, list(tf))
                drawn = torch.empty_like(x)
                ops.ddpm_step_ex(x, e, tab, clip_denoised=clip, seed=K_SEED, first_id=K_FIRST, x_out=drawn, **tf)
                given = torch.empty_like(x)
                ops.ddpm_step_ex(x, e, tab, clip_denoised=clip, noise=zk, x_out=given, **tf)
                assert torch.equal(drawn, given) and torch.equal(drawn, want_k), (t, clip, list(tf))


@pytest.mark.parametrize("shape", SHAPES)
def test_per_sample_t_takes_one_table_row_per_sample(dev, sched, shape):
    """A non-uniform t equals one stedm_ddpm_step per sample at its own t (noise, keep bits and blend noise keyed by sample id and t);
    a t outside [0, T) leaves that sample alone."""
    from stedm_amd import ops
    tab, sa, s1 = sched
    B = shape[0]
    x, e, _ = _ops(dev, shape, "ps")
    x0 = (prng.normal(95, f"ps.x0.{shape}", shape)).to(dev)
    m = (prng.uniform(95, f"ps.m.{shape}", (B, 1) + shape[2:]) > 0).float().to(dev)
    ts = [999, 0, 500][:B]
    t = torch.tensor(ts, dtype=torch.int64, device=dev)
    for masked in (False, True):
        kw = dict(mask=m, x0=x0, mask_seed=99, sqrt_ac=sa, sqrt_1mac=s1) if masked else {}
        got = torch.empty_like(x)
        ops.ddpm_step_ex(x, e, tab, t=t, seed=K_SEED, first_id=K_FIRST, x_out=got, **kw)
        for b in range(B):
            kb = dict(kw, mask=m[b:b + 1].contiguous(), x0=x0[b:b + 1].contiguous()) if masked else {}
            one = ops.ddpm_step(x[b:b + 1].clone(), e[b:b + 1].contiguous(), tab, torch.tensor([ts[b]], dtype=torch.int32, device=dev), True,
                                seed=K_SEED, first_id=K_FIRST + b, **kb)
            assert torch.equal(got[b:b + 1], one), (b, masked)
    out = torch.full_like(x, 7.0)
    x0o, mo = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    t_bad = t.clone()
    t_bad[0] = 1000
    ops.ddpm_step_ex(x, e, tab, t=t_bad, seed=K_SEED, first_id=K_FIRST, x_out=out, x0_out=x0o, mean_out=mo)
    assert bool((out[0] == 7).all()) and bool((x0o[0] == 7).all()) and bool((mo[0] == 7).all())
    plain = torch.empty_like(x)
    ops.ddpm_step_ex(x, e, tab, t=t, seed=K_SEED, first_id=K_FIRST, x_out=plain)
    assert torch.equal(out[1:], plain[1:])
    step_bad = torch.tensor([-1], dtype=torch.int32, device=dev)
    out.fill_(7.0)
    ops.ddpm_step_ex(x, e, tab, step_idx=step_bad, seed=K_SEED, x_out=out)
    assert bool((out == 7).all())
    with pytest.raises(ValueError):
        ops.ddpm_step_ex(x, e, tab, step_idx=step_bad, t=t, x_out=out)
    with pytest.raises(ValueError):
        ops.ddpm_step_ex(x, e, tab, t=t)


@pytest.mark.parametrize("shape", SHAPES)
def test_temperature_and_dropout_match_the_restatement(dev, sched, shape):
    from stedm_amd import ops
    tab, sa, s1 = sched
    B, n = shape[0], int(np.prod(shape[1:]))
    x, e, _ = _ops(dev, shape, "td")
    unit = torch.zeros_like(tab)
    unit[:, 4] = 1.0                                                   # mean = 0, sigma = 1: the sample is the noise term itself
    worst = 0.0
    for t in TS:
        z = ops.philox_normal(B, shape[1:], K_SEED, 0x10000 + t, dev, first_id=K_FIRST)
        for T, p in ((0.7, 0.0), (1.0, 0.25), (0.6, 0.2), (1.0, 1e-6)):     # p < 2^-17: every element kept, still scaled
            temps = torch.ones(1000, device=dev)
            temps[t] = T                                               # only row t: an index other than t would read 1
            keep = torch.from_numpy(keep_mask(K_SEED, range(K_FIRST, K_FIRST + B), n, t, p)).view(shape).to(dev)
            ks = torch.where(keep, torch.tensor(drop_scale(p), device=dev), torch.tensor(0.0, device=dev)) if p > 0 else torch.ones_like(x)
            nz = (z * torch.tensor(T, device=dev)) * ks
            for tf in _t_forms(dev, B, t):
                got_n = torch.empty_like(x)
                ops.ddpm_step_ex(x, e, unit, temperature=temps, noise_dropout=p, seed=K_SEED, first_id=K_FIRST, x_out=got_n, **tf)
                assert torch.equal(got_n, nz), (t, T, p, list(tf))
                for clip in (True, False):
                    got, mean, x0o = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
                    ops.ddpm_step_ex(x, e, tab, clip_denoised=clip, temperature=temps, noise_dropout=p, seed=K_SEED, first_id=K_FIRST,
                                     x_out=got, x0_out=x0o, mean_out=mean, **tf)
                    sr, srm1, c1, c2, sig = tab[t]
                    q = sr * x - srm1 * e
                    q = q.clamp(-1., 1.) if clip else q
                    ref = (c1 * q + c2 * x) + sig * nz
                    worst = max(worst, float((got - ref).abs().max()) / float(ref.abs().max()))
                    assert float((got - ref).abs().max()) <= 4e-7 * float(ref.abs().max()), (t, T, p, clip)
                    assert torch.equal(x0o, q) and torch.equal(mean, c1 * q + c2 * x), (t, T, p, clip)
                    assert torch.equal(got, mean + sig * nz), (t, T, p, clip)              # the noise term, read back through mean_out
    print(f"[ddpm_step_ex {shape}] worst max|diff|/max|ref| against the torch restatement: {worst:.3e}")


@pytest.mark.parametrize("E,n_e", [(3, 8192), (4, 300), (8, 64)])
@pytest.mark.parametrize("hw", [(16, 16), (9, 9)])                      # the float4 form; HW % 4 != 0
def test_quantisation_equals_vq_nearest(dev, sched, E, n_e, hw):
    from stedm_amd import ops
    tab, sa, s1 = sched
    shape = (3, E) + hw
    B = shape[0]
    x, e, z = _ops(dev, shape, f"q{n_e}")
    cb = (prng.normal(95, f"q.cb.{E}.{n_e}", (n_e, E)) * 0.6).to(dev)
    cb[5] = cb[3]                                                       # a tie: the first index wins
    ident = tab.clone()
    ident[:, 0], ident[:, 1] = 1.0, 0.0                                 # x0 = 1 x - 0 eps = x: latents can sit exactly on entries
    xi = x.clone()
    rows = torch.arange(hw[0] * hw[1], device=dev) % n_e
    xi[0] = cb[rows].t().reshape(E, *hw)                                # sample 0: every pixel is an entry (rows 3 and 5 among them)
    for table, xin, clip in ((tab, x, True), (tab, x, False), (ident, xi, False)):
        for t in (0, 500):
            for tf in _t_forms(dev, B, t):
                x0c = torch.empty_like(x)
                ops.ddpm_step_ex(xin, e, table, clip_denoised=clip, x0_out=x0c, **tf)              # the clamped x0, no codebook
                idx_ref, zq_ref = ops.vq_nearest(x0c, cb)
                got, x0q, mean = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
                idx = torch.empty((B,) + hw, dtype=torch.int64, device=dev)
                ops.ddpm_step_ex(xin, e, table, clip_denoised=clip, noise=z, codebook=cb, x_out=got, x0_out=x0q, mean_out=mean, idx_out=idx,
                                 **tf)
                assert torch.equal(idx, idx_ref) and torch.equal(x0q, zq_ref), (t, clip, list(tf))
                c1, c2, sig = table[t, 2], table[t, 3], table[t, 4]
                ref = c1 * zq_ref + c2 * xin
                assert float((mean - ref).abs().max()) <= 4e-7 * float(ref.abs().max())
                assert torch.equal(got, mean + sig * z)
                only = torch.empty_like(x)                                                         # p_mean_variance's form: no sample
                ops.ddpm_step_ex(xin, e, table, clip_denoised=clip, codebook=cb, x0_out=only, **tf)
                assert torch.equal(only, zq_ref)
        if table is ident:
            assert torch.equal(idx_ref[0].reshape(-1), torch.where(rows == 5, torch.tensor(3, device=dev), rows))
            assert float((zq_ref[0] - xi[0]).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        ops.ddpm_step_ex(x, e, tab, step_idx=torch.zeros(1, dtype=torch.int32, device=dev), codebook=cb, x_out=torch.empty_like(x))


@pytest.mark.parametrize("shape", SHAPES)
def test_mask_blend_is_ddpm_steps(dev, sched, shape):
    from stedm_amd import ops
    tab, sa, s1 = sched
    B = shape[0]
    x, e, z = _ops(dev, shape, "mb")
    x0 = prng.normal(95, f"mb.x0.{shape}", shape).to(dev)
    zb = prng.normal(95, f"mb.zb.{shape}", shape).to(dev)
    masks = [(prng.uniform(95, "mb.m", (B, 1) + shape[2:]) > 0).float().to(dev),
             prng.uniform(95, "mb.mb", (1, shape[1]) + shape[2:], lo=0., hi=1.).to(dev)]
    for t in TS:
        step = torch.tensor([t], dtype=torch.int32, device=dev)
        for m in masks:
            kw = dict(mask=m, x0=x0, sqrt_ac=sa, sqrt_1mac=s1)
            want = ops.ddpm_step(x.clone(), e, tab, step, True, seed=K_SEED, first_id=K_FIRST, mask_seed=99, **kw)
            want_g = ops.ddpm_step(x.clone(), e, tab, step, True, noise=z, mask_noise=zb, **kw)
            for tf in _t_forms(dev, B, t):
                got, got_g = torch.empty_like(x), torch.empty_like(x)
                ops.ddpm_step_ex(x, e, tab, seed=K_SEED, first_id=K_FIRST, mask_seed=99, x_out=got, **kw, **tf)
                ops.ddpm_step_ex(x, e, tab, noise=z, mask_noise=zb, x_out=got_g, **kw, **tf)
                assert torch.equal(got, want) and torch.equal(got_g, want_g), (t, tuple(m.shape), list(tf))


def test_kept_fraction_at_batch_64_is_binomial(dev, sched):
    from stedm_amd import ops
    tab, _, _ = sched
    shape = (64, 4, 32, 32)
    x, e, _ = _ops(dev, shape, "frac")
    unit = torch.zeros_like(tab)
    unit[:, 4] = 1.0
    step = torch.tensor([2], dtype=torch.int32, device=dev)
    for p in (0.1, 0.3):
        nout = torch.empty_like(x)
        ops.ddpm_step_ex(x, e, unit, step_idx=step, noise_dropout=p, seed=7, x_out=nout)
        kept = float((nout != 0).double().mean())
        sd = np.sqrt(p * (1 - p) / nout.numel())
        assert abs(kept - (1 - p)) < 5 * sd, (p, kept)
        assert np.array_equal((nout != 0).cpu().numpy().reshape(64, -1), keep_mask(7, range(64), 4 * 32 * 32, 2, p))


# ------------------------------------------------------------------------------------------------ loops (tiny U-Net)
T_TINY, SEED_TINY = 12, 4242
RAMP = [0.5 + 0.04 * i for i in range(T_TINY)]


def _tiny_inputs(B=2):
    g = lambda n, s, k=1.0: prng.normal(96, n, s) * k
    x0 = g("l.x0", (B, 4, 16, 16))
    mask = torch.zeros(B, 1, 16, 16)
    mask[..., :8] = 1.0
    return g("l.xT", (B, 4, 16, 16)), g("l.cc", (B, 3, 16, 16), 0.5), g("l.ctx", (B, 128)), x0, mask


def _tiny(dev, use_graph, precision, quant):
    from tests.test_gpu_ddim_options import _FS
    from tests.test_gpu_sampler import make
    ld = make(dev, use_graph, precision)
    if quant:
        ld.first_stage_model = _FS(prng.normal(96, "l.cb", (512, 4)) * 0.8).to(dev)
    return ld


def _progressive(dev, use_graph, precision, variant, T=T_TINY, temperature=RAMP, p=0.1):
    xT, cc, ctx, x0, mask = _tiny_inputs()
    ld = _tiny(dev, use_graph, precision, variant == "quantised")
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    kw = dict(mask=mask.to(dev), x0=x0.to(dev), mask_seed=5) if variant == "masked" else {}
    x, inter = ld.progressive_denoising(cond, (2, 4, 16, 16), quantize_denoised=variant == "quantised", temperature=temperature,
                                        noise_dropout=p, x_T=xT.to(dev), start_T=T, log_every_t=4, noise_seed=SEED_TINY, **kw)
    return x.clone(), inter


@pytest.mark.parametrize("precision", ["parity", "f16"])
@pytest.mark.parametrize("variant", ["plain", "masked", "quantised"])
def test_graph_replay_equals_eager_loop(dev, precision, variant):
    eager, ei = _progressive(dev, False, precision, variant)
    graph, gi = _progressive(dev, True, precision, variant)
    assert torch.equal(graph, eager)
    assert len(gi) == len(ei) == 4 and all(torch.equal(a, b) for a, b in zip(gi, ei))       # x0 of t = 11, 8, 4, 0
    assert bool(torch.isfinite(graph).all())
    if variant == "quantised":
        cb = (prng.normal(96, "l.cb", (512, 4)) * 0.8).to(dev).double()
        px = gi[-1].permute(0, 2, 3, 1).reshape(-1, 4).double()
        assert float(torch.cdist(px, cb).min(dim=1).values.max()) < 1e-5                     # the logged x0 are codebook rows


def test_tiny_unet_progressive_vs_the_cpu_oracle_loop(dev, golden):
    """parity mode, temperature ramp and dropout, no quantisation (a 1e-3 U-Net deviation may flip a near-tie index): against the CPU
    loop over the oracle U-Net fed the kernel's noises and keep masks."""
    from stedm_amd import ops
    from tests.test_gpu_ddpm import _oracle_unet
    T, p = 20, 0.2
    ramp = [0.5 + 0.025 * i for i in range(T)]
    ou, ocfg, plan, P = _oracle_unet()
    xT, cc, ctx, _, _ = _tiny_inputs()
    eps = lambda x, t, cx: ou.unet_forward(P, ocfg, torch.cat([x, cc], 1), t, cx, plan=plan)
    noises = [ops.philox_normal(2, (4, 16, 16), SEED_TINY, 0x10000 + (T - 1 - k), dev).cpu() for k in range(T)]
    keeps = kernel_keeps(SEED_TINY, [0, 1], T, p, (2, 4, 16, 16))
    ref, ref_i, _ = ref_progressive(eps, xT, T, f20_buffers(golden), True, ctx, noises, ramp, keeps, log_every_t=4)
    got, got_i = _progressive(dev, True, "parity", "plain", T=T, temperature=ramp, p=p)
    err = rel(got, ref)
    err_i = max(rel(a, b) for a, b in zip(got_i, ref_i))
    print(f"[progressive-{T}, TINY U-Net, graph] max|diff|/std vs oracle loop: {err:.3e}; logged x0: {err_i:.3e}")
    assert len(got_i) == len(ref_i) == 6
    assert err < 1e-3 and err_i < 1e-3


# ------------------------------------------------------------------------------------------------ F25 through the HIP sampler
def _gpu_toy(dev, clip, codebook=None):
    from tests.test_gpu_ddim_options import _FS
    from tests.test_gpu_ddpm import GpuToy
    toy = GpuToy(dev, clip)
    if codebook is not None:
        toy.first_stage_model = _FS(codebook).to(dev)
    return toy


F25_NOISE_SEED = 6          # case (a)'s tie margin along the chain fed this seed's keep masks is 7.5e-4 (CPU restated loop)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_f25_on_the_hip_sampler(dev, golden, name):
    """The recorded noises given as `noises`; the dropout case is keyed by noise_seed, so the CPU restated loop is fed the kernel's keep
    masks (numpy restatement) instead of the recorded ones."""
    from stedm_amd.ancestral import AncestralSampler
    c = f25_case(golden, name)
    toy = _gpu_toy(dev, c["clip"], c["codebook"])
    T = c["T"]
    kw = dict(mask=c["mask"].to(dev), x0=c["x0"].to(dev), mask_noises=c["q_noises"]) if c["mask"] is not None else {}
    shape_kw = dict(shape=F25_SHAPE[1:], batch_size=2) if c.get("batch_form") else dict(shape=F25_SHAPE)
    x, inter = AncestralSampler(toy).progressive_denoising(c["cond"].to(dev), quantize_denoised=c["codebook"] is not None,
                                                           temperature=c["temps"], noise_dropout=c["p"], x_T=c["xT"].to(dev), start_T=T,
                                                           log_every_t=c["log_every_t"], noises=c["noises"], noise_seed=F25_NOISE_SEED,
                                                           verbose=False, **shape_kw, **kw)
    assert [int(t[0]) for t in toy.ts] == list(range(T - 1, -1, -1))
    stats = {}
    keeps = kernel_keeps(F25_NOISE_SEED, [0, 1], T, c["p"]) if c["p"] > 0 else None
    ref, ref_i, _ = ref_progressive(toy_eps, c["xT"], T, f20_buffers(golden), c["clip"], c["cond"], c["noises"], c["temps"], keeps,
                                    c["codebook"], c["mask"], c["x0"], c["q_noises"], c["log_every_t"], stats=stats)
    if c["codebook"] is not None:
        assert stats["gap"] >= 1e-4                                    # no near-tie along this chain: the indices cannot flip
    err = rel_max(x.cpu(), ref)
    err_i = max(rel_max(a.cpu(), b) for a, b in zip(inter, ref_i))
    print(f"[F25 {name} on the HIP sampler] max|diff|/max|ref| {err:.3e}; logged x0 {err_i:.3e}")
    assert len(inter) == len(ref_i) == c["inter"].shape[0]
    assert err <= F20_TOL and err_i <= F20_TOL
    if c["p"] == 0:
        assert rel_max(x.cpu(), c["out"]) <= F20_TOL
        assert max(rel_max(a.cpu(), b) for a, b in zip(inter, c["inter"])) <= F20_TOL


def test_shard_invariance_with_dropout_quantisation_and_mask(dev, golden):
    """Samples 3..4 of a B = 5 run equal a B = 2 run with sample_id0 = 3 bit for bit: step noise, blend noise and keep bits are keyed by the
    global sample id (the closed-form eps model is elementwise, so the model call does not depend on the batch either)."""
    from stedm_amd.ancestral import AncestralSampler
    c = f25_case(golden, "a")
    toy = _gpu_toy(dev, True, c["codebook"])
    shape5 = (5,) + F25_SHAPE[1:]
    xT, cond, x0 = (prng.normal(97, n, shape5).to(dev) for n in ("sh.xT", "sh.c", "sh.x0"))
    mask = (prng.uniform(97, "sh.m", (5, 1, 8, 8)) > 0).float().to(dev)
    run = lambda sl, id0: AncestralSampler(toy).progressive_denoising(
        cond[sl] * 0.3, (sl.stop - sl.start,) + F25_SHAPE[1:], quantize_denoised=True, temperature=c["temps"], noise_dropout=0.2, x_T=xT[sl],
        start_T=20, log_every_t=5, noise_seed=31, sample_id0=id0, mask=mask[sl], x0=x0[sl], mask_seed=32)
    full, fi = run(slice(0, 5), 0)
    part, pi = run(slice(3, 5), 3)
    assert torch.equal(full[3:], part) and all(torch.equal(a[3:], b) for a, b in zip(fi, pi))
    other, _ = run(slice(3, 5), 0)
    assert not torch.equal(other, part)


def test_latent_diffusion_single_steps_and_quantised_sample_log(dev, golden):
    f = golden("f25_progressive")
    g = lambda k: torch.from_numpy(np.asarray(f[k]))
    x, t, cond, cb = g("d_x").to(dev), g("d_t").to(dev), g("cond").to(dev), g("codebook")
    z = prng.normal(F25_SEED, "prog.d.n0", F25_SHAPE).to(dev)
    ld = _tiny(dev, False, "parity", False)
    from tests.test_gpu_ddim_options import _FS
    ld.first_stage_model = _FS(cb).to(dev)
    unet_call = ld.apply_model
    ld.apply_model = lambda xx, tt, cc, **kw: toy_eps(xx, tt, cc)
    x_in = x.clone()
    xs, x0s = ld.p_sample(x_in, cond, t, clip_denoised=True, quantize_denoised=True, return_x0=True, temperature=0.8, _noise=z)
    assert torch.equal(x_in, x)
    e1, e2 = rel_max(xs.cpu(), g("d_sample")), rel_max(x0s.cpu(), g("d_sample_x0"))
    out = ld.p_mean_variance(x, cond, t, clip_denoised=True, return_x0=True)
    e3, e4 = rel_max(out[0].cpu(), g("d_mean")), rel_max(out[3].cpu(), g("d_x_recon"))
    print(f"[F25 d on LatentDiffusion] p_sample {e1:.3e} x0 {e2:.3e}; p_mean_variance mean {e3:.3e} x_recon {e4:.3e}")
    assert max(e1, e2, e3, e4) <= F20_TOL
    assert out[1].shape == out[2].shape == (2, 1, 1, 1)
    assert torch.equal(out[1].cpu(), g("d_var")) and torch.equal(out[2].cpu(), g("d_logvar"))
    pm, pv, plv = ld.q_posterior(x_start=g("x0").to(dev), x_t=x, t=t)
    assert rel_max(pm.cpu(), g("d_qpost_mean")) <= F20_TOL and torch.equal(pv, out[1])
    # the in-kernel draw of a single step: the philox row of each sample's own t
    from stedm_amd import ops
    drawn = ld.p_sample(x, cond, t, clip_denoised=True, noise_seed=9, sample_id0=2)
    rows = torch.cat([ops.philox_normal(1, F25_SHAPE[1:], 9, 0x10000 + int(t[b]), dev, first_id=2 + b) for b in range(2)])
    assert torch.equal(drawn, ld.p_sample(x, cond, t, clip_denoised=True, _noise=rows))
    # sample_log(ddim=False, quantize_denoised=True) over the U-Net: the chain ends on codebook rows (at t = 0 the mean is c1 x0, c1 = 1)
    ld.apply_model = unet_call
    ld.first_stage_model = _FS(prng.normal(96, "l.cb", (512, 4)) * 0.8).to(dev)
    xT, cc, ctx, _, _ = _tiny_inputs()
    cnd = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    s, inter = ld.sample_log(cnd, 2, False, 0, x_T=xT.to(dev), timesteps=8, quantize_denoised=True, noise_seed=3)
    assert isinstance(inter, list) and bool(torch.isfinite(s).all())
    px = s.permute(0, 2, 3, 1).reshape(-1, 4).double()
    assert float(torch.cdist(px, ld.first_stage_model.quantize.embedding.weight.double()).min(dim=1).values.max()) < 1e-5
