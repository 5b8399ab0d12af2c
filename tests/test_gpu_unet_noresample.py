"""GPU tier (-m gpu): the HIP U-Net with conv_resample=False (Downsample = 2 x 2 average pool, Upsample = bare nearest x2;
openaimodel.py:113-132, 156-173) against fixtures the reference itself produced on the CPU (tests/golden/make_golden_noresample.py:
TINY + conv_resample=False, B = 2, 16 x 16, seed 6, t = [951, 21]; and the same with use_scale_shift_norm=True) - forward, the
CFG / uniform_t / graphed-sampler forms, and the training backward, eager and captured.

The project's thresholds for this net, unchanged (test_gpu_unet.py / test_gpu_unet_film.py: parity 1e-3, f16 6e-3, bf16 5e-2, max error / std;
the backward's bounds of _check_grads). Each test prints what it measured; the figures of the MI355X run are in DESIGN.md section 4.5."""
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
TAGS = {False: "noconv_tiny", True: "noconv_film_tiny"}
MODE_TOL = {"parity": 1e-3, "f16": 6e-3, "bf16": 5e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(dev, precision="parity", film=False):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, conv_resample=False, use_scale_shift_norm=film, **TINY).eval()
    prng.fill_module_(m, seed=SEED)
    return m.to(dev)


def inputs(dev, film=False):
    tag = TAGS[film]
    x = prng.normal(SEED, f"unet.{tag}.x", (B, 7, HW, HW)).to(dev)
    ctx = prng.normal(SEED, f"unet.{tag}.ctx", (B, 128)).to(dev)
    target = prng.normal(SEED, f"unet.{tag}.target", (B, 4, HW, HW)).to(dev)
    return x, ctx, target


def rel(a, b):
    a = a.double().cpu(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max()) / (float(b.std()) + 1e-12)


@pytest.mark.parametrize("film", [False, True])
def test_noconv_parity_forward_vs_reference_golden(dev, golden, film):
    fx = golden(f"f31_unet_{TAGS[film]}")
    m = build(dev, film=film)
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    x, ctx, _ = inputs(dev, film)
    t = torch.from_numpy(fx["t"]).to(dev)
    y = m(x, t, context=ctx)
    m.check_f16_range()
    err = rel(y, fx["y"])
    print(f"[{TAGS[film]}] parity-mode max err / std vs reference golden: {err:.3e}")
    assert err < 1e-3
    y2 = m.forward_parts(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_noconv_single_product_forward(dev, golden, precision):
    fx = golden("f31_unet_noconv_tiny")
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    y = m(x, torch.from_numpy(fx["t"]).to(dev), context=ctx)
    err = rel(y, fx["y"])
    print(f"[noconv tiny {precision}] max err / std vs reference golden: {err:.3e} (threshold {MODE_TOL[precision]:.0e})")
    assert err < MODE_TOL[precision]


@pytest.mark.parametrize("precision", ["parity", "f16", "bf16"])
def test_noconv_forward_cfg_equals_two_forwards(dev, precision):
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.noconv_tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    ya = m.forward_parts(xl, cc, t, ctx).clone()
    yb = m.forward_parts(xl, cc, t, ctx_u).clone()
    e_c, e_u = m.forward_cfg(xl, cc, t, ctx, ctx_u)
    ea, eb = rel(e_c, ya.cpu()), rel(e_u, yb.cpu())
    print(f"[noconv cfg {precision}] cond {ea:.3e} uncond {eb:.3e}")
    assert ea < MODE_TOL[precision] and eb < MODE_TOL[precision]
    assert rel(ya, yb.cpu()) > 1e-2, "the two style vectors must give different outputs"


@pytest.mark.parametrize("precision", ["parity", "bf16"])
def test_noconv_uniform_t_equals_equal_timesteps_bitwise(dev, precision):
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.noconv_tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([437, 437], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    a = m.forward_parts(xl, cc, t, ctx).clone()
    b = m.forward_parts(xl, cc, t, ctx, uniform_t=True).clone()
    assert torch.equal(a, b)
    c1, u1 = [v.clone() for v in m.forward_cfg(xl, cc, t, ctx, ctx_u)]
    c2, u2 = m.forward_cfg(xl, cc, t, ctx, ctx_u, uniform_t=True)
    assert torch.equal(c1, c2) and torch.equal(u1, u2)


def test_noconv_ddim_cfg_graphed_equals_eager(dev):
    from stedm_amd.latent_diffusion import LatentDiffusion
    outs = []
    for use_graph in (False, True):
        ld = LatentDiffusion(build(dev), linear_start=0.0015, linear_end=0.0205, image_size=16, channels=4, conditioning_key="hybrid",
                             loss_type="l1", use_graph=use_graph).to(dev)
        xT = prng.normal(30, "s.xT", (B, 4, 16, 16)).to(dev)
        cc = (prng.normal(30, "s.cc", (B, 3, 16, 16)) * 0.5).to(dev)
        cond = {"c_concat": [cc], "c_crossattn": [prng.normal(30, "s.ctx", (B, 128)).to(dev)]}
        unc = {"c_concat": [cc.clone()], "c_crossattn": [prng.normal(30, "s.ctxu", (B, 128)).to(dev)]}
        s, _ = ld.sample_log(cond, B, True, 4, eta=0.0, x_T=xT, unconditional_conditioning=unc, unconditional_guidance_scale=1.5, log_every_t=1000)
        assert bool(torch.isfinite(s).all())
        outs.append(s.clone())
    assert torch.equal(outs[0], outs[1])


def test_noconv_ns32_modes_and_cfg_routes(dev):
    """The bench-sized net (128 .. 1024 channels) at batch 8 with conv_resample=False: the pool and the nearest x2 at the shipped widths,
    forward_cfg with every admissible shared-skip site forced on and off (pooled skip tensors are read modulo B like any other), and the
    16-bit concat hand-offs of a batch >= 8 in the blocks that end with a ResBlock. No reference fixture at this size: the single-product
    modes against the parity mode of the same weights, at the modes' thresholds."""
    from stedm_amd.unet import UNetModel
    NS32 = dict(image_size=32, in_channels=7, model_channels=128, out_channels=4, num_res_blocks=2,
                attention_resolutions=[32, 16, 8], channel_mult=[1, 4, 8], num_heads=8)
    m = UNetModel(precision="parity", conv_resample=False, **NS32).eval()
    prng.fill_module_(m, seed=0)
    m = m.to(dev)
    Bn = 8
    x = prng.normal(0, "unet.noconv_ns32.x", (Bn, 4, 32, 32)).to(dev)
    cc = prng.normal(0, "unet.noconv_ns32.cc", (Bn, 3, 32, 32)).to(dev)
    ctx = prng.normal(0, "unet.noconv_ns32.ctx", (Bn, 512)).to(dev)
    ctx_u = prng.normal(0, "unet.noconv_ns32.ctxu", (Bn, 512)).to(dev)
    t = torch.full((Bn,), 437, dtype=torch.long, device=dev)
    ref_c = m.forward_parts(x, cc, t, ctx).cpu().clone()
    ref_u = m.forward_parts(x, cc, t, ctx_u).cpu().clone()
    m.check_f16_range()
    for mode in ("f16", "bf16"):
        m.set_precision(mode)
        e1 = rel(m.forward_parts(x, cc, t, ctx), ref_c)
        print(f"[noconv ns32 {mode}] forward_parts vs parity {e1:.3e}")
        assert e1 < MODE_TOL[mode]
        for shared in (False, True):
            m.cfg_shared_skip = shared
            e_c, e_u = m.forward_cfg(x, cc, t, ctx, ctx_u, uniform_t=True)
            ea, eb = rel(e_c, ref_c), rel(e_u, ref_u)
            print(f"[noconv ns32 {mode} shared_skip={shared}] cond {ea:.3e} uncond {eb:.3e}")
            assert ea < MODE_TOL[mode] and eb < MODE_TOL[mode]
        m.cfg_shared_skip = None
        m.check_f16_range()


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


@pytest.mark.parametrize("film", [False, True])
def test_noconv_backward_vs_reference_golden(dev, golden, film):
    from stedm_amd.train import UNetTrainer
    tag = TAGS[film]
    fx = golden(f"f31_grads_{tag}")
    m = build(dev, film=film)
    tr = UNetTrainer(m)
    x, ctx, target = inputs(dev, film)
    t = torch.from_numpy(fx["t"]).to(dev)
    loss, dx, dctx = tr.loss_and_backward(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
    ref_c = torch.from_numpy(fx["dctx"]).double()
    err_c = float((dctx.double().cpu() - ref_c).norm() / ref_c.norm())
    err_l = abs(float(loss) - float(fx["loss"])) / float(fx["loss"])
    print(f"[{tag}] loss {float(loss):.6f} (rel {err_l:.2e})  dctx rel-L2 {err_c:.2e}")
    assert err_l < 1e-4
    check_summary(dx, fx, "dx", 2e-3, tag)
    worst = _check_grads(m, fx, 1e-3, tag)
    print(f"[{tag}] worst param grad {worst[0]:.2e} at {worst[1]}")
    assert err_c < 1e-3
    names = [n for n, _ in m.named_parameters()]
    assert not any(".op." in n or ".conv." in n for n in names), "the resampling layers have no parameters"
    # two calls give the same bits
    g1 = [p.grad.clone() for p in m.parameters()]
    tr.loss_and_backward(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, m.parameters()))


def test_noconv_train_steps_reduce_the_loss(dev):
    from stedm_amd.train import UNetTrainer
    m = build(dev, "bf16")
    tr = UNetTrainer(m, lr=2e-4, weight_decay=0.0)
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    losses = [float(tr.train_step(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)) for _ in range(6)]
    print("losses", ["%.4f" % v for v in losses])
    assert losses[-1] < losses[0] - 0.01


def test_noconv_captured_train_step_equals_the_eager_step_bitwise(dev):
    """train_step_graphed serves a conv_resample=False model with no special case: six steps with a different batch each (three eager,
    then the captured step replayed) against train_step() on a second copy: losses and parameters bit for bit."""
    from stedm_amd.train import UNetTrainer
    runs = []
    for graphed in (True, False):
        m = build(dev, "bf16")
        tr = UNetTrainer(m, lr=2e-4, weight_decay=0.01)
        losses = []
        for step in range(6):
            x = prng.normal(SEED + step, f"unet.noconv_tiny.cap{step}.x", (B, 7, HW, HW)).to(dev)
            ctx = prng.normal(SEED + step, f"unet.noconv_tiny.cap{step}.ctx", (B, 128)).to(dev)
            target = prng.normal(SEED + step, f"unet.noconv_tiny.cap{step}.target", (B, 4, HW, HW)).to(dev)
            t = torch.tensor([951 - 7 * step, 21 + step], device=dev)
            a = (x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
            losses.append(float(tr.train_step_graphed(*a) if graphed else tr.train_step(*a)))
        torch.cuda.synchronize()
        if graphed:
            assert tr._graph is not None and tr.step_count == 6
        runs.append((losses, [p.detach().clone() for p in m.parameters()]))
    (la, pa), (lb, pb) = runs
    print("losses", ["%.5f" % v for v in la])
    assert la == lb, (la, lb)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
