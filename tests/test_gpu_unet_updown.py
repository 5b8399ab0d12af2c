"""GPU tier (-m gpu): the HIP U-Net with resblock_updown=True (every resolution change is a ResBlock(up / down) whose two branches are
resampled without parameters; openaimodel.py:220-229, 268-275, 596-613, 709-724) against fixtures the reference itself produced on the CPU
(tests/golden/make_golden_updown.py: TINY + resblock_updown=True, B = 2, 16 x 16, seed 6, t = [951, 21]; and the same with
use_scale_shift_norm=True) - forward, the CFG / uniform_t / graphed-sampler forms, and the training backward, eager and captured.

The project's thresholds for this net, taken unchanged from tests/test_gpu_unet_noresample.py (parity 1e-3, f16 6e-3, bf16 5e-2, max error /
std; the backward's bounds of _check_grads). Each test prints what it measured; the figures of the MI355X run are in DESIGN.md section 4.6."""
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
TAGS = {False: "updown_tiny", True: "updown_film_tiny"}
MODE_TOL = {"parity": 1e-3, "f16": 6e-3, "bf16": 5e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(dev, precision="parity", film=False, updown=True):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, resblock_updown=updown, use_scale_shift_norm=film, **TINY).eval()
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


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the new pass (ops.gn_apply16c_resample)"""
    from stedm_amd import ops
    n = {"n": 0}
    real = ops.gn_apply16c_resample

    def counted(*a, **k):
        n["n"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "gn_apply16c_resample", counted)
    return n


@pytest.mark.parametrize("film", [False, True])
def test_updown_parity_forward_vs_reference_golden(dev, golden, calls, film):
    fx = golden(f"f32_unet_{TAGS[film]}")
    m = build(dev, film=film)
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    x, ctx, _ = inputs(dev, film)
    t = torch.from_numpy(fx["t"]).to(dev)
    y = m(x, t, context=ctx)
    m.check_f16_range()
    assert calls["n"] == 4, "one pass per up / down block"
    err = rel(y, fx["y"])
    print(f"[{TAGS[film]}] parity-mode max err / std vs reference golden: {err:.3e}")
    assert err < 1e-3
    y2 = m.forward_parts(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_updown_single_product_forward(dev, golden, precision, film):
    fx = golden(f"f32_unet_{TAGS[film]}")
    m = build(dev, precision, film)
    x, ctx, _ = inputs(dev, film)
    y = m(x, torch.from_numpy(fx["t"]).to(dev), context=ctx)
    m.check_f16_range()
    err = rel(y, fx["y"])
    print(f"[{TAGS[film]} {precision}] max err / std vs reference golden: {err:.3e} (threshold {MODE_TOL[precision]:.0e})")
    assert err < MODE_TOL[precision]


def test_resblock_updown_false_takes_the_route_it_takes_today(dev, calls):
    """a model built without the option never calls the new pass: forward, forward_cfg and a training step"""
    from stedm_amd.train import UNetTrainer
    m = build(dev, "bf16", updown=False)
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    m.forward_parts(xl, cc, t, ctx)
    m.forward_cfg(xl, cc, t, ctx, ctx)
    UNetTrainer(m).loss_and_backward(xl, cc, t, ctx, target)
    assert calls["n"] == 0
    m2 = build(dev, "bf16")
    UNetTrainer(m2).loss_and_backward(xl, cc, t, ctx, target)
    assert calls["n"] == 4, "bf16 training keeps the forward's planes: no second pass in the backward"


@pytest.mark.parametrize("precision", ["parity", "f16", "bf16"])
def test_updown_forward_cfg_equals_two_forwards_bitwise(dev, precision):
    """forward_cfg = two forward_parts calls, bit for bit, with cfg_shared_skip forced off and on (the pooled encoder outputs are ordinary
    skip tensors; the up blocks run at 2B like any decoder ResBlock without a skip input). In parity mode both settings are bit-equal (the
    shared-skip pair is a single-product form). In f16 / bf16, bit-equal with the pair off; with it forced on, the decoder concat
    convolutions sum their skip channels in a separate launch - another order of fp32 additions by design (_in_conv; DESIGN.md section
    10.11), for this model as for the default one - so that setting is held to the mode's threshold, as tests/test_gpu_unet_noresample.py
    holds it (measured on the MI355X: f16 2.0e-3, bf16 1.6e-2)."""
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.updown_tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    ya = m.forward_parts(xl, cc, t, ctx).clone()
    yb = m.forward_parts(xl, cc, t, ctx_u).clone()
    assert rel(ya, yb.cpu()) > 1e-2, "the two style vectors must give different outputs"
    for shared in (False, True):
        m.cfg_shared_skip = shared
        e_c, e_u = m.forward_cfg(xl, cc, t, ctx, ctx_u)
        ea, eb = rel(e_c, ya.cpu()), rel(e_u, yb.cpu())
        print(f"[updown cfg {precision} shared_skip={shared}] cond {ea:.3e} uncond {eb:.3e}")
        if precision == "parity" or not shared:
            assert torch.equal(e_c, ya) and torch.equal(e_u, yb), f"shared_skip={shared}"
        else:
            assert ea < MODE_TOL[precision] and eb < MODE_TOL[precision]
    m.cfg_shared_skip = None


@pytest.mark.parametrize("precision", ["parity", "bf16"])
def test_updown_uniform_t_equals_equal_timesteps_bitwise(dev, precision):
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.updown_tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([437, 437], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    a = m.forward_parts(xl, cc, t, ctx).clone()
    b = m.forward_parts(xl, cc, t, ctx, uniform_t=True).clone()
    assert torch.equal(a, b)
    c1, u1 = [v.clone() for v in m.forward_cfg(xl, cc, t, ctx, ctx_u)]
    c2, u2 = m.forward_cfg(xl, cc, t, ctx, ctx_u, uniform_t=True)
    assert torch.equal(c1, c2) and torch.equal(u1, u2)


def test_updown_ddim_cfg_graphed_equals_eager(dev):
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


def test_updown_ns32_modes_and_cfg_routes(dev):
    """The bench-sized net (128 .. 1024 channels) at batch 8 with resblock_updown=True: the pass at the shipped widths (pool 32^2 x 128 and
    16^2 x 512, nearest 8^2 x 1024 and 16^2 x 512 at the decoder batch), forward_cfg with every admissible shared-skip site forced on and off,
    and the 16-bit concat hand-off of the up blocks that end a decoder block at a batch >= 8. No reference fixture at this size: the
    single-product modes against the parity mode of the same weights, at the modes' thresholds."""
    from stedm_amd.unet import UNetModel
    NS32 = dict(image_size=32, in_channels=7, model_channels=128, out_channels=4, num_res_blocks=2,
                attention_resolutions=[32, 16, 8], channel_mult=[1, 4, 8], num_heads=8)
    m = UNetModel(precision="parity", resblock_updown=True, **NS32).eval()
    prng.fill_module_(m, seed=0)
    m = m.to(dev)
    Bn = 8
    x = prng.normal(0, "unet.updown_ns32.x", (Bn, 4, 32, 32)).to(dev)
    cc = prng.normal(0, "unet.updown_ns32.cc", (Bn, 3, 32, 32)).to(dev)
    ctx = prng.normal(0, "unet.updown_ns32.ctx", (Bn, 512)).to(dev)
    ctx_u = prng.normal(0, "unet.updown_ns32.ctxu", (Bn, 512)).to(dev)
    t = torch.full((Bn,), 437, dtype=torch.long, device=dev)
    ref_c = m.forward_parts(x, cc, t, ctx).cpu().clone()
    ref_u = m.forward_parts(x, cc, t, ctx_u).cpu().clone()
    m.check_f16_range()
    for mode in ("f16", "bf16"):
        m.set_precision(mode)
        e1 = rel(m.forward_parts(x, cc, t, ctx), ref_c)
        print(f"[updown ns32 {mode}] forward_parts vs parity {e1:.3e}")
        assert e1 < MODE_TOL[mode]
        for shared in (False, True):
            m.cfg_shared_skip = shared
            e_c, e_u = m.forward_cfg(x, cc, t, ctx, ctx_u, uniform_t=True)
            ea, eb = rel(e_c, ref_c), rel(e_u, ref_u)
            print(f"[updown ns32 {mode} shared_skip={shared}] cond {ea:.3e} uncond {eb:.3e}")
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
def test_updown_backward_vs_reference_golden(dev, golden, film):
    from stedm_amd.train import UNetTrainer
    tag = TAGS[film]
    fx = golden(f"f32_grads_{tag}")
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
    assert not any(".op." in n or ".conv." in n or "_upd" in n for n in names), "the resampling layers have no parameters"
    # two calls give the same bits
    g1 = [p.grad.clone() for p in m.parameters()]
    tr.loss_and_backward(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, m.parameters()))


def test_updown_train_steps_reduce_the_loss(dev):
    from stedm_amd.train import UNetTrainer
    m = build(dev, "bf16")
    tr = UNetTrainer(m, lr=2e-4, weight_decay=0.0)
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    losses = [float(tr.train_step(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)) for _ in range(6)]
    print("losses", ["%.4f" % v for v in losses])
    assert losses[-1] < losses[0] - 0.01


@pytest.mark.parametrize("film", [False, True])
def test_updown_captured_train_step_equals_the_eager_step_bitwise(dev, film):
    """train_step_graphed serves a resblock_updown=True model with no special case: six steps with a different batch each (three eager,
    then the captured step replayed) against train_step() on a second copy: losses and parameters bit for bit."""
    from stedm_amd.train import UNetTrainer
    runs = []
    for graphed in (True, False):
        m = build(dev, "bf16", film)
        tr = UNetTrainer(m, lr=2e-4, weight_decay=0.01)
        losses = []
        for step in range(6):
            x = prng.normal(SEED + step, f"unet.updown_tiny.cap{step}.x", (B, 7, HW, HW)).to(dev)
            ctx = prng.normal(SEED + step, f"unet.updown_tiny.cap{step}.ctx", (B, 128)).to(dev)
            target = prng.normal(SEED + step, f"unet.updown_tiny.cap{step}.target", (B, 4, HW, HW)).to(dev)
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


def test_updown_autograd_bridge(dev):
    """the autograd bridge of latent_diffusion.py (p_losses in train(): `loss.backward()` runs the HIP backward) carries an up / down model:
    one bridged backward leaves the gradients of p_losses_backward, bit for bit; two accumulate to twice those"""
    from stedm_amd.latent_diffusion import LatentDiffusion
    unet = build(dev)
    ld = LatentDiffusion(unet, linear_start=0.0015, linear_end=0.0205, image_size=16, channels=4, conditioning_key="hybrid", loss_type="l1").to(dev)
    ld.train()
    x, ctx, noise = inputs(dev)
    x0, cond, t = x[:, :4].contiguous(), {"c_concat": [x[:, 4:].contiguous()], "c_crossattn": [ctx]}, torch.tensor([951, 21], device=dev)
    loss_d = ld.p_losses_backward(x0, cond, t, noise)[0]
    direct = [p.grad.clone() for p in unet.parameters()]

    def backward_n(k):
        ld.zero_grad(set_to_none=True)
        for _ in range(k):
            with torch.enable_grad():
                loss, _ = ld.p_losses(x0, cond, t, noise)
                assert loss.requires_grad
                loss.backward()
        return float(loss), [p.grad.clone() for p in unet.parameters()]

    l1, g1 = backward_n(1)
    _, g2 = backward_n(2)
    assert l1 == float(loss_d)
    assert all(torch.equal(a, b) for a, b in zip(direct, g1))
    assert all(torch.equal(b, 2 * a) for a, b in zip(g1, g2))
    named = dict(zip([n for n, _ in unet.named_parameters()], g1))
    for blk in ("input_blocks.3.0", "input_blocks.6.0", "output_blocks.2.1", "output_blocks.5.1"):
        assert float(named[blk + ".in_layers.0.weight"].abs().sum()) > 0 and float(named[blk + ".in_layers.2.weight"].abs().sum()) > 0
