"""GPU tier (-m gpu): the HIP U-Net with use_new_attention_order=True (the middle AttentionBlock as QKVAttention, openaimodel.py:401-428:
the qkv convolution's channels split into q | k | v first, heads second) against fixtures the reference itself produced on the CPU
(tests/golden/make_golden_attn_order.py: TINY + use_new_attention_order=True, B = 2, seed 6, t = [951, 21]; at 16 x 16 - 16 tokens -, at
32 x 32 - 64 tokens, the 64-token forms - and at 16 x 16 with two heads of 64) - forward, the CFG / uniform_t / graphed-sampler forms, and the
training backward, eager and captured.

The state dict is the same in both orders, so only the numbers tell a swapped layout: every fixture stores order_gap, the difference of
the two orders' outputs on the same weights (max / std), and every forward test asserts it above twice its own tolerance.
Thresholds: tests/test_gpu_unet_updown.py's, unchanged (parity 1e-3, f16 6e-3, bf16 5e-2, max error / std; the backward's bounds of
_check_grads). Each test prints what it measured; the figures of the MI355X run are in DESIGN.md section 4.7."""
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
B, SEED = 2, 6
# tag -> (constructor arguments on top of TINY, input height / width, tokens and heads x width of the middle attention)
TAGS = {"neworder_tiny": (dict(), 16, (16, 4, 32)),
        "neworder_t64": (dict(image_size=32), 32, (64, 4, 32)),
        "neworder_nhc_tiny": (dict(num_heads=-1, num_head_channels=64), 16, (16, 2, 64))}
MODE_TOL = {"parity": 1e-3, "f16": 6e-3, "bf16": 5e-2}
ENTRIES = ("stedm_attn_legacy", "stedm_attn_legacy16", "stedm_attn_legacy_bwd", "stedm_attn_qkv", "stedm_attn_qkv16", "stedm_attn_qkv_bwd")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(dev, precision="parity", tag="neworder_tiny", new=True):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, use_new_attention_order=new, **dict(TINY, **TAGS[tag][0])).eval()
    prng.fill_module_(m, seed=SEED)
    return m.to(dev)


def inputs(dev, tag="neworder_tiny"):
    HW = TAGS[tag][1]
    x = prng.normal(SEED, f"unet.{tag}.x", (B, 7, HW, HW)).to(dev)
    ctx = prng.normal(SEED, f"unet.{tag}.ctx", (B, 128)).to(dev)
    target = prng.normal(SEED, f"unet.{tag}.target", (B, 4, HW, HW)).to(dev)
    return x, ctx, target


def rel(a, b):
    a = a.double().cpu(); b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max()) / (float(b.std()) + 1e-12)


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the six attention entries of the library and records the `order` argument of the three new ones"""
    from stedm_amd import _lib
    L = _lib.lib()
    n = {e: 0 for e in ENTRIES}
    n["orders"] = []
    pos = {"stedm_attn_qkv": 6, "stedm_attn_qkv16": 8, "stedm_attn_qkv_bwd": 7}

    def wrap(name):
        real = getattr(L, name)

        def counted(*a):
            n[name] += 1
            if name in pos:
                n["orders"].append(int(a[pos[name]]))
            return real(*a)
        monkeypatch.setattr(L, name, counted)
    for e in ENTRIES:
        wrap(e)
    return n


@pytest.mark.parametrize("tag", list(TAGS))
def test_new_order_parity_forward_vs_reference_golden(dev, golden, calls, tag):
    fx = golden(f"f33_unet_{tag}")
    m = build(dev, tag=tag)
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    ab = m.middle_block[2]
    x, ctx, _ = inputs(dev, tag)
    assert (x.shape[2] * x.shape[3] // 16, ab.num_heads, ab.channels // ab.num_heads) == TAGS[tag][2] and ab.attn_order == 1
    t = torch.from_numpy(fx["t"]).to(dev)
    y = m(x, t, context=ctx)
    m.check_f16_range()
    assert calls["stedm_attn_qkv"] == 1 and calls["orders"] == [1] and calls["stedm_attn_legacy"] == calls["stedm_attn_legacy16"] == 0
    err, gap = rel(y, fx["y"]), float(fx["order_gap"])
    print(f"[{tag}] parity-mode max err / std vs reference golden: {err:.3e} (the other order would be off by {gap:.3f})")
    assert gap > 2 * MODE_TOL["parity"]
    assert err < MODE_TOL["parity"]
    y2 = m.forward_parts(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx)
    assert torch.equal(y, y2)
    # the same weights in the legacy order are the other function, by about the fixture's gap
    e_old = rel(build(dev, tag=tag, new=False)(x, t, context=ctx), fx["y"])
    assert e_old > 0.5 * gap, e_old


@pytest.mark.parametrize("tag", list(TAGS))
@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_new_order_single_product_forward(dev, golden, calls, precision, tag):
    fx = golden(f"f33_unet_{tag}")
    m = build(dev, precision, tag)
    x, ctx, _ = inputs(dev, tag)
    y = m(x, torch.from_numpy(fx["t"]).to(dev), context=ctx)
    m.check_f16_range()
    assert calls["stedm_attn_qkv16"] == 1 and calls["orders"] == [1] and calls["stedm_attn_legacy"] == calls["stedm_attn_legacy16"] == 0
    err, gap = rel(y, fx["y"]), float(fx["order_gap"])
    print(f"[{tag} {precision}] max err / std vs reference golden: {err:.3e} (threshold {MODE_TOL[precision]:.0e}, order gap {gap:.3f})")
    assert gap > 2 * MODE_TOL[precision]
    assert err < MODE_TOL[precision]


def test_legacy_order_takes_the_route_it_takes_today(dev, calls):
    """a model built without the option issues the attention launches it always did - the 16-bit entry in the forwards, the fp32 entry and
    its backward in a training step - and none of the new entry points; with the option, the same counts on the new entries, order 1"""
    from stedm_amd.train import UNetTrainer
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()

    def run(m):
        m.forward_parts(xl, cc, t, ctx)
        m.forward_cfg(xl, cc, t, ctx, ctx)
        UNetTrainer(m).loss_and_backward(xl, cc, t, ctx, target)
    run(build(dev, "bf16", new=False))
    assert (calls["stedm_attn_legacy16"], calls["stedm_attn_legacy"], calls["stedm_attn_legacy_bwd"]) == (2, 1, 1)
    assert calls["stedm_attn_qkv"] == calls["stedm_attn_qkv16"] == calls["stedm_attn_qkv_bwd"] == 0 and calls["orders"] == []
    run(build(dev, "bf16"))
    assert (calls["stedm_attn_qkv16"], calls["stedm_attn_qkv"], calls["stedm_attn_qkv_bwd"]) == (2, 1, 1) and calls["orders"] == [1] * 4
    assert (calls["stedm_attn_legacy16"], calls["stedm_attn_legacy"], calls["stedm_attn_legacy_bwd"]) == (2, 1, 1)


def test_legacy_order_calls_the_ops_with_their_original_arguments(dev, monkeypatch):
    """bench.py's AttnTimer replaces ops.attn_legacy16 by a function of its four original positional arguments (and tools may do the same
    with the other two): a model in the default order must go on calling them that way - forward, forward_cfg and a training step"""
    from stedm_amd import ops
    from stedm_amd.train import UNetTrainer
    seen = {"attn_legacy": 0, "attn_legacy16": 0, "attn_legacy_bwd": 0}
    real = {k: getattr(ops, k) for k in seen}

    def fwd(qkv, out, heads):
        seen["attn_legacy"] += 1
        return real["attn_legacy"](qkv, out, heads)

    def fwd16(qkv, out16, heads, prec):
        seen["attn_legacy16"] += 1
        return real["attn_legacy16"](qkv, out16, heads, prec)

    def bwd(qkv, d_out, d_qkv, heads):
        seen["attn_legacy_bwd"] += 1
        return real["attn_legacy_bwd"](qkv, d_out, d_qkv, heads)
    monkeypatch.setattr(ops, "attn_legacy", fwd)
    monkeypatch.setattr(ops, "attn_legacy16", fwd16)
    monkeypatch.setattr(ops, "attn_legacy_bwd", bwd)
    m = build(dev, "bf16", new=False)
    x, ctx, target = inputs(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    m.forward_parts(xl, cc, t, ctx)
    m.forward_cfg(xl, cc, t, ctx, ctx)
    UNetTrainer(m).loss_and_backward(xl, cc, t, ctx, target)
    assert seen == {"attn_legacy": 1, "attn_legacy16": 2, "attn_legacy_bwd": 1}


@pytest.mark.parametrize("precision", ["parity", "f16", "bf16"])
def test_new_order_forward_cfg_equals_two_forwards_bitwise(dev, precision):
    """forward_cfg = two forward_parts calls, bit for bit (cfg_shared_skip off: the forced-on pair sums the skip channels in a separate launch,
    another order of fp32 additions by design, which tests/test_gpu_unet_updown.py holds to the mode's threshold; in parity mode both settings)"""
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.neworder_tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([951, 21], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    ya = m.forward_parts(xl, cc, t, ctx).clone()
    yb = m.forward_parts(xl, cc, t, ctx_u).clone()
    assert rel(ya, yb.cpu()) > 1e-2, "the two style vectors must give different outputs"
    for shared in ((False, True) if precision == "parity" else (False,)):
        m.cfg_shared_skip = shared
        e_c, e_u = m.forward_cfg(xl, cc, t, ctx, ctx_u)
        assert torch.equal(e_c, ya) and torch.equal(e_u, yb), f"shared_skip={shared}"
    m.cfg_shared_skip = None


@pytest.mark.parametrize("precision", ["parity", "bf16"])
def test_new_order_uniform_t_equals_equal_timesteps_bitwise(dev, precision):
    m = build(dev, precision)
    x, ctx, _ = inputs(dev)
    ctx_u = prng.normal(SEED, "unet.neworder_tiny.ctxu", (B, 128)).to(dev)
    t = torch.tensor([437, 437], device=dev)
    xl, cc = x[:, :4].contiguous(), x[:, 4:].contiguous()
    a = m.forward_parts(xl, cc, t, ctx).clone()
    b = m.forward_parts(xl, cc, t, ctx, uniform_t=True).clone()
    assert torch.equal(a, b)
    c1, u1 = [v.clone() for v in m.forward_cfg(xl, cc, t, ctx, ctx_u)]
    c2, u2 = m.forward_cfg(xl, cc, t, ctx, ctx_u, uniform_t=True)
    assert torch.equal(c1, c2) and torch.equal(u1, u2)


def test_new_order_ddim_cfg_graphed_equals_eager(dev):
    from stedm_amd.latent_diffusion import LatentDiffusion
    outs = []
    for new, use_graph in ((True, False), (True, True), (False, True)):
        ld = LatentDiffusion(build(dev, new=new), linear_start=0.0015, linear_end=0.0205, image_size=16, channels=4, conditioning_key="hybrid",
                             loss_type="l1", use_graph=use_graph).to(dev)
        xT = prng.normal(30, "s.xT", (B, 4, 16, 16)).to(dev)
        cc = (prng.normal(30, "s.cc", (B, 3, 16, 16)) * 0.5).to(dev)
        cond = {"c_concat": [cc], "c_crossattn": [prng.normal(30, "s.ctx", (B, 128)).to(dev)]}
        unc = {"c_concat": [cc.clone()], "c_crossattn": [prng.normal(30, "s.ctxu", (B, 128)).to(dev)]}
        s, _ = ld.sample_log(cond, B, True, 4, eta=0.0, x_T=xT, unconditional_conditioning=unc, unconditional_guidance_scale=1.5, log_every_t=1000)
        assert bool(torch.isfinite(s).all())
        outs.append(s.clone())
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[1], outs[2]), "the captured graph of the other order samples something else"


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


@pytest.mark.parametrize("tag", ["neworder_tiny", "neworder_t64"])
def test_new_order_backward_vs_reference_golden(dev, golden, calls, tag):
    """16 tokens: attn_legacy_bwd_kernel<1> (LDS-resident); 64 tokens of 32-wide heads: attn64_bwd_mfma_kernel<1>"""
    from stedm_amd.train import UNetTrainer
    fx = golden(f"f33_grads_{tag}")
    m = build(dev, tag=tag)
    tr = UNetTrainer(m)
    x, ctx, target = inputs(dev, tag)
    t = torch.from_numpy(fx["t"]).to(dev)
    loss, dx, dctx = tr.loss_and_backward(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
    assert calls["stedm_attn_qkv_bwd"] == 1 and calls["stedm_attn_qkv"] == 1 and calls["orders"] == [1, 1] and calls["stedm_attn_legacy_bwd"] == 0
    ref_c = torch.from_numpy(fx["dctx"]).double()
    err_c = float((dctx.double().cpu() - ref_c).norm() / ref_c.norm())
    err_l = abs(float(loss) - float(fx["loss"])) / float(fx["loss"])
    print(f"[{tag}] loss {float(loss):.6f} (rel {err_l:.2e})  dctx rel-L2 {err_c:.2e}  (qkv weight gradient of the other order off by "
          f"{float(fx['qkv_grad_gap']):.2f})")
    assert float(fx["qkv_grad_gap"]) > 0.1 and float(fx["order_gap"]) > 0.1
    assert err_l < 1e-4
    check_summary(dx, fx, "dx", 2e-3, tag)
    worst = _check_grads(m, fx, 1e-3, tag)
    print(f"[{tag}] worst param grad {worst[0]:.2e} at {worst[1]}")
    assert err_c < 1e-3
    # two calls give the same bits
    g1 = [p.grad.clone() for p in m.parameters()]
    tr.loss_and_backward(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
    assert all(torch.equal(a, p.grad) for a, p in zip(g1, m.parameters()))


def test_new_order_captured_train_step_equals_the_eager_step_bitwise(dev):
    """train_step_graphed serves a use_new_attention_order=True model with no special case: five steps (three eager, the capture, one replay) with a different batch each against
    train_step() on a second copy: losses and parameters bit for bit"""
    from stedm_amd.train import UNetTrainer
    runs = []
    for graphed in (True, False):
        m = build(dev, "bf16")
        tr = UNetTrainer(m, lr=2e-4, weight_decay=0.01)
        losses = []
        for step in range(5):
            x = prng.normal(SEED + step, f"unet.neworder_tiny.cap{step}.x", (B, 7, 16, 16)).to(dev)
            ctx = prng.normal(SEED + step, f"unet.neworder_tiny.cap{step}.ctx", (B, 128)).to(dev)
            target = prng.normal(SEED + step, f"unet.neworder_tiny.cap{step}.target", (B, 4, 16, 16)).to(dev)
            t = torch.tensor([951 - 7 * step, 21 + step], device=dev)
            a = (x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
            losses.append(float(tr.train_step_graphed(*a) if graphed else tr.train_step(*a)))
        torch.cuda.synchronize()
        if graphed:
            assert tr._graph is not None and tr.step_count == 5
        runs.append((losses, [p.detach().clone() for p in m.parameters()]))
    (la, pa), (lb, pb) = runs
    print("losses", ["%.5f" % v for v in la])
    assert la == lb, (la, lb)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
