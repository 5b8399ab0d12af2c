"""GPU tier (-m gpu): DDIM with the step noise drawn in the kernel, temperature, noise_dropout and quantize_x0 (stedm_ddim_step_ex,
stedm_ddim_quantize_x0). The kernels against stedm_ddim_step / stedm_vq_nearest and torch restatements, the sampler's graphed loop against
its eager loop and against the CPU loop of tests/test_ddim_options_oracle.py, F21 on the HIP sampler, and the sharded prediction path."""
import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_ddim_options_oracle import F21_CASES, F21_S, F21_SEED, ddim_opts_sample, drop_scale, f21_case, keep_mask, toy_eps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.std())


def _table(dev, S=20, eta=1.0):
    from oracle import ddim as od
    ds = od.DDIMSchedule(od.Schedule(), S, eta)
    n = ds.ddim_timesteps.shape[0]
    return torch.tensor([ds.scalars(i) for i in range(n)], dtype=torch.float32, device=dev), n


def _operands(dev, shape, tag):
    x = prng.normal(8, f"k.{tag}.x", shape).to(dev)
    e_c = prng.normal(8, f"k.{tag}.ec", shape).to(dev)
    e_u = (prng.normal(8, f"k.{tag}.eu", shape) * 0.9).to(dev)
    return x, e_c, e_u


# ------------------------------------------------------------------------------------------------ the update kernel
@pytest.mark.parametrize("shape", [(3, 4, 32, 32), (2, 3, 40, 40)])       # register-resident form; generic form (256 % 40 != 0)
def test_in_kernel_draw_equals_ddim_step_fed_philox_rows(dev, shape):
    from stedm_amd import ops
    coefs, n = _table(dev)
    x, e_c, e_u = _operands(dev, shape, shape[2])
    step = torch.tensor([7], dtype=torch.int32, device=dev)
    it = n - 1 - 7
    for cfg in (None, e_u):
        z = ops.philox_normal(shape[0], shape[1:], 1234, 1 + it, dev, first_id=5)
        ref = torch.empty_like(x); ref_x0 = torch.empty_like(x)
        ops.ddim_step(x, e_c, cfg, coefs, ref, pred_x0=ref_x0, noise=z, step_idx=step, cfg_scale=1.5)
        got = torch.empty_like(x); got_x0 = torch.empty_like(x)
        ops.ddim_step_ex(x, e_c, cfg, coefs, got, pred_x0=got_x0, draw=True, step_idx=step, n_iters=n, cfg_scale=1.5, seed=1234, first_id=5)
        assert torch.equal(got, ref) and torch.equal(got_x0, ref_x0)
        got2 = torch.empty_like(x)                                         # given noise through the new entry: the same bits too
        ops.ddim_step_ex(x, e_c, cfg, coefs, got2, noise=z, step_idx=step, n_iters=n, cfg_scale=1.5)
        assert torch.equal(got2, ref)


@pytest.mark.parametrize("shape", [(3, 4, 32, 32), (2, 3, 40, 40), (2, 3, 64, 64)])    # register form; generic forms (vq-f4's 3 channels)
def test_ddim_step_rounds_each_product_and_fuses_only_the_noise(dev, shape):
    """stedm_ddim_step's arithmetic, pinned against a restatement: x_prev = (sqrt(a_prev) x0 + dir e) with both products rounded, then
    fma(sigma, z, .) for the noise term - in every kernel form, with and without the noise, through both entries."""
    from stedm_amd import ops
    coefs, n = _table(dev)
    x, e_c, _ = _operands(dev, shape, f"r{shape[2]}")
    z = prng.normal(8, f"k.r{shape[2]}.z", shape).to(dev)
    r = n // 2
    tab0 = coefs.clone()
    tab0[:, 2] = 0.0                                                       # sigma = 0 (eta = 0): dir = sqrt(1 - a_prev) exactly
    for tab in (tab0, coefs):
        step = torch.tensor([r], dtype=torch.int32, device=dev)
        a_prev, sigma = tab[r, 1], tab[r, 2]
        base, x0 = torch.empty_like(x), torch.empty_like(x)
        ops.ddim_step(x, e_c, None, tab, base, pred_x0=x0, step_idx=step)
        if float(sigma) == 0.0:
            ref = torch.sqrt(a_prev) * x0 + torch.sqrt(1.0 - a_prev) * e_c
            assert torch.equal(base, ref)
        got = torch.empty_like(x)
        ops.ddim_step(x, e_c, None, tab, got, noise=z, step_idx=step)
        ref = (sigma.double() * z.double() + base.double()).float()       # fma: the product exact in f64, one rounding (to f32)
        assert torch.equal(got, ref)
        got_ex = torch.empty_like(x)
        ops.ddim_step_ex(x, e_c, None, tab, got_ex, noise=z, step_idx=step, n_iters=n)
        assert torch.equal(got_ex, got)


@pytest.mark.parametrize("shape", [(3, 4, 32, 32), (2, 3, 40, 40)])
def test_temperature_and_dropout_match_the_torch_restatement(dev, shape):
    from stedm_amd import ops
    coefs, n = _table(dev)
    x, e_c, e_u = _operands(dev, shape, f"t{shape[2]}")
    step = torch.tensor([4], dtype=torch.int32, device=dev)
    it = n - 1 - 4
    sigma = float(coefs[4, 2])
    assert sigma > 0
    B, C, H, W = shape
    z = ops.philox_normal(B, shape[1:], 99, 1 + it, dev, first_id=3)
    base = torch.empty_like(x)
    ops.ddim_step(x, e_c, e_u, coefs, base, step_idx=step, cfg_scale=2.0)          # sqrt(a_prev) x0 + dir (no noise term)
    eps_ref = torch.empty_like(x)
    for T, p in ((0.7, 0.0), (1.0, 0.25), (0.6, 0.2), (1.0, 1e-6)):     # p < 2^-17: every element kept, still scaled
        keep = torch.from_numpy(keep_mask(99, range(3, 3 + B), C * H * W, it, p)).view(shape).to(dev)
        ks = torch.where(keep, torch.tensor(drop_scale(p), device=dev), torch.tensor(0.0, device=dev))
        nz = ((torch.tensor(sigma, device=dev) * z) * T) * ks
        ref = base + nz
        got = torch.empty_like(x); nout = torch.empty_like(x); eps = torch.empty_like(x)
        ops.ddim_step_ex(x, e_c, e_u, coefs, got, draw=True, step_idx=step, n_iters=n, cfg_scale=2.0, temperature=T, noise_dropout=p,
                         seed=99, first_id=3, eps_out=eps, noise_out=nout)
        assert torch.equal(got, ref), (T, p, float((got - ref).abs().max()))      # every instantiation computes the base term alike
        assert torch.equal(nout, nz)
        if p == 0.0:
            eps_ref = eps.clone()
        assert torch.equal(eps, eps_ref)
    # the guided eps is what stedm_ddim_step combines: x0 recovered from it matches
    x0 = torch.empty_like(x)
    ops.ddim_step(x, e_c, e_u, coefs, torch.empty_like(x), pred_x0=x0, step_idx=step, cfg_scale=2.0)
    a_t, sq1m = float(coefs[4, 0]), float(coefs[4, 3])
    assert rel((x - sq1m * eps_ref) / np.float32(np.sqrt(a_t)), x0) < 1e-5


def test_kept_fraction_at_batch_64_is_binomial(dev):
    from stedm_amd import ops
    coefs, n = _table(dev)
    shape = (64, 4, 32, 32)
    x, e_c, _ = _operands(dev, shape, "frac")
    step = torch.tensor([2], dtype=torch.int32, device=dev)
    for p in (0.1, 0.3):
        nout = torch.empty_like(x)
        ops.ddim_step_ex(x, e_c, None, coefs, torch.empty_like(x), draw=True, step_idx=step, n_iters=n, noise_dropout=p, seed=7,
                         noise_out=nout)
        kept = float((nout != 0).double().mean())
        sd = np.sqrt(p * (1 - p) / nout.numel())
        assert abs(kept - (1 - p)) < 5 * sd, (p, kept)
        ref = keep_mask(7, range(64), 4 * 32 * 32, n - 1 - 2, p)
        assert np.array_equal((nout != 0).cpu().numpy().reshape(64, -1), ref)


# ------------------------------------------------------------------------------------------------ quantize_x0
@pytest.mark.parametrize("E,n_e", [(3, 8192), (4, 300), (8, 64)])
def test_quantize_kernel_against_vq_nearest_and_torch(dev, E, n_e):
    from stedm_amd import ops
    coefs, n = _table(dev)
    shape = (4, E, 16, 16)
    x0 = prng.normal(9, f"q.x0.{E}", shape).to(dev)
    eps = prng.normal(9, f"q.e.{E}", shape).to(dev)
    nz = (prng.normal(9, f"q.n.{E}", shape) * 0.1).to(dev)
    cb = (prng.normal(9, f"q.cb.{E}", (n_e, E)) * 0.7).to(dev)
    cb[5] = cb[3]                                                          # a tie: the first index wins
    idx_ref, zq_ref = ops.vq_nearest(x0, cb)
    step = torch.tensor([6], dtype=torch.int32, device=dev)
    for noise in (nz, None):
        px = x0.clone(); xp = torch.empty_like(x0)
        idx = torch.empty((4, 16, 16), dtype=torch.int64, device=dev)
        ops.ddim_quantize_x0(px, eps, coefs, cb, xp, noise=noise, step_idx=step, idx=idx)
        assert torch.equal(idx, idx_ref)
        assert torch.equal(px, zq_ref)                                    # z + (e - z), as vq_nearest returns it
        assert float((px - cb[idx].permute(0, 3, 1, 2)).abs().max()) < 1e-5
        a_prev, sigma = float(coefs[6, 1]), float(coefs[6, 2])
        ref = np.float32(np.sqrt(a_prev)) * px + np.float32(np.sqrt(np.float32(1.0 - a_prev - sigma * sigma))) * eps
        if noise is not None:
            ref = ref + noise
        assert rel(xp, ref) < 1e-6


# ------------------------------------------------------------------------------------------------ sampler loops (tiny U-Net)
class _FS(torch.nn.Module):
    def __init__(self, cb):
        super().__init__()
        self.quantize = torch.nn.Module()
        self.quantize.embedding = torch.nn.Embedding(cb.shape[0], cb.shape[1])
        self.quantize.embedding.weight.data.copy_(cb)


def _tiny(dev, use_graph, precision, quant=False):
    from tests.test_gpu_sampler import make
    ld = make(dev, use_graph, precision)
    if quant:
        ld.first_stage_model = _FS(prng.normal(31, "l.cb", (512, 4)) * 0.8).to(dev)
    return ld


def _loop(ld, dev, eta, cfg, masked, S=5, **kw):
    from tests.test_gpu_masked_sampler import _tiny_inputs
    xT, cc, ctx, ctx_u, x0, mask = _tiny_inputs()
    cond = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}
    unc = {"c_concat": [cc.to(dev)], "c_crossattn": [ctx_u.to(dev)]}
    if cfg:
        kw.update(unconditional_conditioning=unc, unconditional_guidance_scale=1.5)
    if masked:
        kw.update(mask=mask.to(dev), x0=x0.to(dev), mask_seed=5)
    out, _ = ld.sample_log(cond, batch_size=2, ddim=True, ddim_steps=S, eta=eta, x_T=xT.to(dev), **kw)
    return out


LOOPS = [(1.0, True, False, "parity"), (0.5, False, True, "f16"), (1.0, True, True, "bf16"), (0.5, True, False, "f16")]


@pytest.mark.parametrize("eta,cfg,masked,precision", LOOPS)
def test_graph_replay_equals_eager_loop(dev, eta, cfg, masked, precision):
    opts = dict(noise_seed=4242, sample_id0=3, temperature=0.8, noise_dropout=0.1)
    eager = _loop(_tiny(dev, False, precision), dev, eta, cfg, masked, **opts)
    graph = _loop(_tiny(dev, True, precision), dev, eta, cfg, masked, **opts)
    assert torch.equal(graph, eager)
    plain = _loop(_tiny(dev, True, precision), dev, eta, cfg, masked, noise_seed=4242, sample_id0=3)
    assert not torch.equal(plain, graph)
    # the in-kernel draw = the explicit philox rows of stream 1 + iteration (what predict_latents_sharded used to build)
    from stedm_amd import ops
    n = 5
    noises = [ops.philox_normal(2, (4, 16, 16), 4242, 1 + i, dev, first_id=3) for i in range(n)]
    given = _loop(_tiny(dev, False, precision), dev, eta, cfg, masked, noises=noises, sample_id0=3)
    assert torch.equal(given, plain)


def test_graph_replay_with_quantize_x0(dev):
    for eta in (0.0, 1.0):
        kw = dict(quantize_x0=True, noise_seed=11, temperature=0.9)
        eager = _loop(_tiny(dev, False, "parity", True), dev, eta, True, False, **kw)
        graph = _loop(_tiny(dev, True, "parity", True), dev, eta, True, False, **kw)
        assert torch.equal(graph, eager), eta
    # eta = 0 ignores temperature / dropout / noise_seed: the plain loop's bits
    a = _loop(_tiny(dev, True, "parity"), dev, 0.0, True, True)
    b = _loop(_tiny(dev, True, "parity"), dev, 0.0, True, True, temperature=0.5, noise_dropout=0.3, noise_seed=9)
    assert torch.equal(a, b)


@pytest.mark.parametrize("eta,cfg", [(1.0, True), (0.5, False)])
def test_loop_matches_the_cpu_oracle_loop(dev, eta, cfg):
    """The HIP loop (parity mode, noise drawn in the kernel, temperature and dropout) against the CPU loop fed the same noises and masks."""
    from oracle import ddim as od
    from oracle import unet as ou
    from stedm_amd import ops
    from tests.test_gpu_sampler import inputs
    S, T, p = 5, 0.8, 0.2
    got = _loop(_tiny(dev, True, "parity"), dev, eta, cfg, False, noise_seed=77, sample_id0=0, temperature=T, noise_dropout=p)
    n = 5
    noises = [ops.philox_normal(2, (4, 16, 16), 77, 1 + i, dev).cpu() for i in range(n)]
    keeps = [torch.from_numpy(keep_mask(77, range(2), 4 * 16 * 16, i, p)).view(2, 4, 16, 16) for i in range(n)]
    cfgu = ou.UNetConfig(image_size=16, in_channels=7, model_channels=32, out_channels=4, channel_mult=(1, 2, 4), num_heads=4)
    plan = ou.build_plan(cfgu)
    P = prng.fill_state_dict(plan.shapes, 6)
    am = lambda x, t, c: ou.unet_forward(P, cfgu, torch.cat([x, c["c_concat"][0]], 1), t, c["c_crossattn"][0], plan=plan)
    xT, cc, ctx, ctx_u = inputs(2)
    cond = {"c_concat": [cc], "c_crossattn": [ctx]}
    unc = {"c_concat": [cc], "c_crossattn": [ctx_u]} if cfg else None
    ref, _ = ddim_opts_sample(am, od.Schedule(), xT, cond, S, eta, uncond=unc, scale=1.5 if cfg else 1.0, noises=noises, temperature=T,
                              keeps=keeps, p=p)
    err = rel(got, ref)
    print(f"[ddim options loop vs CPU oracle, eta {eta}, cfg {cfg}] max|diff|/std {err:.3e}")
    assert err < 1e-3


def test_f21_on_the_hip_sampler(dev, golden):
    """F21's cases through DDIMSampler.sample on the GPU: the recorded noises given as `noises`; dropout cases keyed by noise_seed, so the
    CPU loop is fed the kernel's keep masks (numpy restatement) instead of the recorded ones."""
    from stedm_amd.ddim import DDIMSampler
    from tests.test_gpu_masked_sampler import GpuToy
    fx = golden("f21_ddim_opts")
    from oracle import ddim as od
    for case, o in F21_CASES.items():
        kw = f21_case(fx, case)
        toy = GpuToy(dev)
        if o.get("quantize_x0"):
            toy.first_stage_model = _FS(kw["codebook"]).to(dev)
        extra = {}
        if "keeps" in kw:
            kw["keeps"] = [torch.from_numpy(keep_mask(5, range(2), 3 * 64, i, kw["p"])).view(2, 3, 8, 8) for i in range(F21_S)]
            extra["noise_seed"] = 5
        dc = lambda c: {"bias": c["bias"].to(dev)}
        gk = dict(unconditional_guidance_scale=kw["scale"], unconditional_conditioning=dc(kw["uncond"])) if "uncond" in kw else {}
        got, _ = DDIMSampler(toy).sample(F21_S, 2, (3, 8, 8), dc(kw["cond"]), verbose=False, eta=kw["eta"], x_T=kw["x_T"].to(dev),
                                         temperature=o.get("temperature", 1.0), noise_dropout=o.get("noise_dropout", 0.0),
                                         quantize_x0=o.get("quantize_x0", False), noises=[n.to(dev) for n in kw["noises"]], **gk, **extra)
        ref, _ = ddim_opts_sample(toy_eps, od.Schedule(), **kw)
        err = rel(got, ref)
        print(f"[F21 {case} on the HIP sampler] max|diff|/std {err:.3e}")
        assert err < 1e-4, case
        if "keeps" not in kw:
            assert rel(got, torch.from_numpy(fx[f"{case}_out"])) < 1e-4, case


# ------------------------------------------------------------------------------------------------ sharded prediction
def test_sharded_eta1_equals_the_explicit_noises_path(dev):
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from stedm_amd.schedule import make_ddim_timesteps
    from tests.test_gpu_sharded import GLOBAL_B, SEED, STEPS, _batch, _model
    model = _model(dev)
    n_iter = int(make_ddim_timesteps(STEPS, model.num_timesteps).shape[0])
    for rank, world in ((0, 1), (1, 2)):
        lo, hi = par.shard_range(GLOBAL_B, rank, world)
        batch = _batch(list(range(lo, hi)), dev)
        got = predict_latents_sharded(model, batch, GLOBAL_B, STEPS, eta=1.0, cfg_scale=1.5, seed=SEED, rank=rank, world=world, gather=False)
        x_T = par.per_sample_normal_device(SEED, lo, hi - lo, (4, 32, 32), 0, dev)
        noises = [par.per_sample_normal_device(SEED, lo, hi - lo, (4, 32, 32), 1 + i, dev) for i in range(n_iter)]
        ref = predict_latents(model, batch, STEPS, eta=1.0, cfg_scale=1.5, x_T=x_T, noises=noises)
        assert torch.equal(got, ref), (rank, world)
