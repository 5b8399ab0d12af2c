"""GPU tier (-m gpu): UNetModel.cfg_shared_front - under forward_cfg the style block (middle_block[1], ResBlockStyle, openaimodel.py:636-643)
keeps its front at batch B: the shared tensor is not replicated, in_layers' GroupNorm rides on middle_block[0]'s tail convolution, in_layers'
3x3 runs once per CFG pair and leaves its K-share partials, the finish pass at 2B adds bias and each sample's style row
(stedm_conv_finish, ws_bmod = B), and the tail convolution at 2B reads the shared tensor as its residual modulo B (UNetModel._res_front).

NS32 at B = 4 (decoder batch 8), cfg_shared_front True (wherever admissible) against False (never), cfg_shared_skip at its default:
  both against the CPU oracle on the same samples, with the bounds of tests/test_gpu_unet_shared_skip.py
    (f16: rel-L2 < 1e-3, max/std < 5.5e-3; bf16: 1.5e-2 / 8e-2);
  on against off with that file's plan-versus-plan bound (f16 2e-3, bf16 1.5e-2: the batch-B launch may take another K split than the 2B one);
  two runs give equal bits; a permuted batch gives the permuted rows, bitwise.
In `parity` the route does not exist (torch.equal). A DDIM-5 StepGraph run with the route on equals its eager run bit for bit. TINY on
24 x 24 latents (the im2col form) routes nothing. With the default policy (None) at B = 3 nothing is routed and forward_cfg equals two
sequential forwards bitwise (the contract of tests/test_gpu_sampler.py::test_cfg_pass_equals_two_sequential_forwards, on its model)."""
import pytest
import torch

from stedm_amd.utils import prng

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
NS32 = dict(image_size=32, in_channels=7, model_channels=128, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 4, 8], num_heads=8)
B = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ns32(dev):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision="parity", **NS32).eval()
    prng.fill_module_(m, seed=0)
    return m.to(dev)


@pytest.fixture(scope="module")
def data():
    return dict(x=prng.normal(13, "ss.x", (B, 4, 32, 32)), cc=prng.normal(13, "ss.cc", (B, 3, 32, 32)),
                ctx_c=prng.normal(13, "ss.ctx", (B, 512)), ctx_u=prng.normal(13, "ss.ctxu", (B, 512)))


@pytest.fixture(scope="module")
def oracle_rows(data):
    """the CPU oracle's cond and uncond forwards of the B samples, computed once"""
    from oracle import unet as ou
    cfg = ou.UNetConfig()
    plan = ou.build_plan(cfg)
    P = prng.fill_state_dict(plan.shapes, 0)
    t = torch.full((B,), 951, dtype=torch.long)
    xc = torch.cat([data["x"], data["cc"]], 1)
    return torch.cat([ou.unet_forward(P, cfg, xc, t, data["ctx_c"], plan=plan), ou.unet_forward(P, cfg, xc, t, data["ctx_u"], plan=plan)])


def dev2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm()), float((a - b).abs().max() / b.std())


def routed(m):
    """the share counts UNetModel._shared_front filed since the model's last (re)pack, for the shapes it routed"""
    return [v for k, v in m._consts.items() if isinstance(k, tuple) and k and k[0] == "sfront" and v]


def asked(m):
    return [k for k in m._consts if isinstance(k, tuple) and k and k[0] == "sfront"]


def run(m, dev, data, on, perm=None):
    m.cfg_shared_front = on
    g = (lambda t_: t_.to(dev)) if perm is None else (lambda t_: t_[perm].contiguous().to(dev))
    t = torch.full((B,), 951, dtype=torch.long, device=dev)
    ec, eu = m.forward_cfg(g(data["x"]), g(data["cc"]), t, g(data["ctx_c"]), g(data["ctx_u"]), uniform_t=True)
    m.check_f16_range()
    return torch.cat([ec, eu]).clone()


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_shared_front_on_and_off_vs_cpu_oracle(dev, ns32, data, oracle_rows, precision):
    m = ns32
    try:
        m.set_precision(precision)
        off = run(m, dev, data, False)
        assert not routed(m)
        on = run(m, dev, data, True)
        assert len(routed(m)) == 1, "cfg_shared_front = True did not route the style block of NS32"
        tol_l2, tol_max = {"f16": (1e-3, 5.5e-3), "bf16": (1.5e-2, 8e-2)}[precision]
        d_off, d_on, d_oo = dev2(off, oracle_rows), dev2(on, oracle_rows), dev2(on, off)
        print(f"\n[NS32 B={B} CFG, {precision}] vs CPU oracle: off rel-L2 {d_off[0]:.3e} max/std {d_off[1]:.3e}; on ({routed(m)[0]} partials) rel-L2 {d_on[0]:.3e} "
              f"max/std {d_on[1]:.3e}; on vs off rel-L2 {d_oo[0]:.3e}")
        assert d_off[0] < tol_l2 and d_off[1] < tol_max
        assert d_on[0] < tol_l2 and d_on[1] < tol_max
        assert d_oo[0] < {"f16": 2e-3, "bf16": 1.5e-2}[precision]
        assert torch.equal(run(m, dev, data, True), on), "the second run differs from the first"
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(1))
        pp = run(m, dev, data, True, perm)
        assert torch.equal(pp, torch.cat([on[:B][perm.to(dev)], on[B:][perm.to(dev)]])), "rows are not independent"
    finally:
        m.cfg_shared_front = None


def test_shared_front_does_not_exist_in_parity(dev, ns32, data):
    m = ns32
    try:
        m.set_precision("parity")
        off = run(m, dev, data, False)
        on = run(m, dev, data, True)
        assert not routed(m)
        assert torch.equal(on, off)
    finally:
        m.cfg_shared_front = None


def test_shared_front_step_graph_equals_eager_bits(dev, ns32):
    from stedm_amd.latent_diffusion import LatentDiffusion
    m = ns32
    xT = prng.normal(14, "ssg.xT", (2, 4, 32, 32)).to(dev)
    cc = (prng.normal(14, "ssg.cc", (2, 3, 32, 32)) > 0).float().to(dev)
    ctx, ctx_u = prng.normal(14, "ssg.ctx", (2, 512)).to(dev), prng.normal(14, "ssg.ctxu", (2, 512)).to(dev)
    try:
        m.set_precision("f16")
        m.cfg_shared_front = True
        outs = []
        for g in (False, True):
            ld = LatentDiffusion(m, linear_start=0.0015, linear_end=0.0205, image_size=32, channels=4, conditioning_key="hybrid", loss_type="l1",
                                 use_graph=g).to(dev)
            s, _ = ld.sample_log({"c_concat": [cc], "c_crossattn": [ctx]}, 2, True, 5, eta=0.0, x_T=xT,
                                 unconditional_conditioning={"c_concat": [cc], "c_crossattn": [ctx_u]}, unconditional_guidance_scale=1.5)
            outs.append(s.clone())
            assert len(routed(m)) >= 1, "the sampling loop did not route the style block"
        assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    finally:
        m.cfg_shared_front = None


def test_shared_front_routes_nothing_on_the_im2col_path(dev):
    from stedm_amd.unet import UNetModel
    size = 24
    m = UNetModel(precision="f16", **dict(TINY, image_size=size, num_res_blocks=1)).eval()
    prng.fill_module_(m, seed=9)
    m = m.to(dev)
    x = prng.normal(15, "ssi.x", (2, 4, size, size)).to(dev); cc = prng.normal(15, "ssi.cc", (2, 3, size, size)).to(dev)
    ctx_c, ctx_u = prng.normal(15, "ssi.ctx", (2, 128)).to(dev), prng.normal(15, "ssi.ctxu", (2, 128)).to(dev)
    t = torch.full((2,), 500, dtype=torch.long, device=dev)
    outs = {}
    for on in (False, True):
        m.cfg_shared_front = on
        ec, eu = m.forward_cfg(x, cc, t, ctx_c, ctx_u, uniform_t=True)
        m.check_f16_range()
        outs[on] = torch.cat([ec, eu]).clone()
        assert not routed(m)
    assert torch.equal(outs[True], outs[False])


def test_default_policy_at_batch_3_routes_nothing_and_keeps_the_bitwise_contract(dev):
    """the model and batch of tests/test_gpu_sampler.py::test_cfg_pass_equals_two_sequential_forwards (TINY, f16, B = 3)"""
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision="f16", **TINY).eval()
    prng.fill_module_(m, seed=6)
    m = m.to(dev)
    assert m.cfg_shared_front is None
    Bs = 3
    x = prng.normal(30, "s.xT", (Bs, 4, 16, 16)).to(dev); cc = (prng.normal(30, "s.cc", (Bs, 3, 16, 16)) * 0.5).to(dev)
    ctx_c, ctx_u = prng.normal(30, "s.ctx", (Bs, 128)).to(dev), prng.normal(30, "s.ctxu", (Bs, 128)).to(dev)
    t = torch.full((Bs,), 951, dtype=torch.long, device=dev)
    ec, eu = m.forward_cfg(x, cc, t, ctx_c, ctx_u)
    ec, eu = ec.clone(), eu.clone()
    assert asked(m) and not routed(m), "the default rule was expected to be asked and to answer no at decoder batch 6"
    o_c = m.forward_parts(x, cc, t, ctx_c).clone()
    o_u = m.forward_parts(x, cc, t, ctx_u).clone()
    m.check_f16_range()
    assert torch.equal(ec, o_c) and torch.equal(eu, o_u)
