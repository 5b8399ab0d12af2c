"""CPU tier: the formulas the kernels of csrc/svit_bwd.hip implement, and the host logic of the opt-in style-encoder training.

tests/refs_svit_bwd.py restates the set-ViT's backward layer by layer with explicit formulas (no autograd); run in fp64 it reproduces the f34
golden gradients (the reference's own module under fp32 autograd, tests/golden/make_golden_svit_grads.py). Bound, per tensor, on max-abs
error over max-abs golden: 4 x the same metric of torch's fp32 autograd against torch's fp64 autograd on the reference module itself -
reference against reference, computed here from the two recorded gradient sets (f34_svit_grads.npz, and the fp64 - fp32 differences of
f34_svit_grads_f64.npz), not a literal."""
import os

import numpy as np
import pytest
import torch

from tests import refs_svit_bwd as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#        tag              image ns B depth heads mlp  pool    dropout
CASES = {"i16_ns2_d2":    (16,  2, 2, 2,    3,   64,  "mean", 0.1),
         "i64_ns1_d1_p0": (64,  1, 1, 1,    2,   128, "cls",  0.0)}
SVIT = dict(name="svit", patch_size=8, dim=64, depth=1, heads=2, mlp_dim=64, pool="mean", channels=3, dropout=0.0, emb_dropout=0.0, t_dim=256)
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[32], channel_mult=[1, 2],
            num_heads=4)


def _module(tag):
    from stedm_amd.style import sViT
    from stedm_amd.utils import prng
    img, ns, B, depth, heads, mlp, pool, p = CASES[tag]
    m = sViT(image_size=img, patch_size=8, num_classes=32, dim=64, depth=depth, heads=heads, mlp_dim=mlp, pool=pool, dropout=p, emb_dropout=p, ns=ns)
    with torch.no_grad():
        prng.fill_module_(m, seed=34)
        for l, (attn, _ff) in enumerate(m.transformer.layers):
            attn.fn.temperature.fill_(float(np.log(64 ** -0.5)) + 0.05 * l)
    return m


@pytest.mark.parametrize("tag", list(CASES))
def test_explicit_backward_reproduces_the_golden_gradients(tag):
    Z, Z64 = np.load(os.path.join(GOLD, "f34_svit_grads.npz")), np.load(os.path.join(GOLD, "f34_svit_grads_f64.npz"))
    img, ns, B, depth, heads, mlp, pool, p = CASES[tag]
    P = {k: v.detach().double() for k, v in _module(tag).named_parameters()}
    cfg = dict(patch=8, heads=heads, pool=pool, p_emb=p, p_drop=p)
    keeps = R.make_keeps(B, (img // 8) ** 2 + 2, 64, mlp, heads, depth, p, p, int(Z["seed"][0]))
    with torch.no_grad():
        out, tape = R.forward(P, torch.from_numpy(Z[tag + ".img"]).double(), cfg, keeps)
        G = R.backward(P, tape, torch.from_numpy(Z[tag + ".g"]).double(), cfg, keeps)
    assert R.rel_err(out, torch.from_numpy(Z[tag + ".out"])) < 1e-5
    assert sorted(G) == sorted(P)
    for k in P:
        g32 = torch.from_numpy(Z[f"{tag}.grad.{k}"])
        g64 = g32.double() + torch.from_numpy(Z64[f"{tag}.grad.{k}"].astype(np.float64)) * float(Z64[f"{tag}.grad.{k}.scale"][0])
        bound = 4.0 * R.rel_err(g32, g64)                 # torch fp32 autograd against torch fp64 autograd, the reference module
        err = R.rel_err(G[k].reshape(g32.shape), g32)
        print(f"{tag} {k:52s} error {err:.2e} bound {bound:.2e}")
        assert err <= bound, f"{k}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("p", [0.0, 0.25])
@torch.enable_grad()
def test_lsa_backward_formulas_against_autograd(p):
    """dS = P o (keep / (1 - p) dP - D), the masked diagonal contributing nothing, d temperature = sum dS o dots"""
    g = torch.Generator().manual_seed(5)
    B, h, T = 2, 2, 9
    q, k, v, d_att = (torch.randn(B, h, T, 64, generator=g, dtype=torch.float64) for _ in range(4))
    temp = torch.tensor(float(np.log(64 ** -0.5)) + 0.1, dtype=torch.float64)
    keep = torch.rand(B, h, T, T, generator=g) >= p
    qa, ka, va, ta = (t.clone().requires_grad_(True) for t in (q, k, v, temp))
    dots = (qa @ ka.transpose(-1, -2)) * ta.exp()
    prob = dots.masked_fill(torch.eye(T, dtype=torch.bool), -torch.finfo(dots.dtype).max).softmax(-1)
    if p > 0:
        prob = prob * (keep.double() / (1.0 - p))
    ((prob @ va) * d_att).sum().backward()
    dq, dk, dv, dt = R.lsa_bwd(q, k, v, temp, d_att, keep, p)
    for a, b in ((dq, qa.grad), (dk, ka.grad), (dv, va.grad), (dt, ta.grad)):
        assert R.rel_err(a, b) < 1e-12


@torch.enable_grad()
def test_building_blocks_against_autograd():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 5, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(16, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(16, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(3, 5, 16, generator=g, dtype=torch.float64)
    (torch.nn.functional.layer_norm(x, (16,), w, b, R.EPS) * dy).sum().backward()
    dx, dg, db = R.ln_bwd(x.detach(), dy, w.detach())
    assert R.rel_err(dx, x.grad) < 1e-12 and R.rel_err(dg, w.grad) < 1e-12 and R.rel_err(db, b.grad) < 1e-12
    pre = torch.randn(100, generator=g, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.gelu(pre).sum().backward()
    assert R.rel_err(R.gelu_grad(pre.detach()), pre.grad) < 1e-12
    for pool in ("mean", "cls"):
        xx = torch.randn(2, 5, 16, generator=g, dtype=torch.float64).requires_grad_(True)
        lw, lb = (torch.randn(16, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(2))
        hw = torch.randn(7, 16, generator=g, dtype=torch.float64).requires_grad_(True)
        hb = torch.zeros(7, dtype=torch.float64, requires_grad=True)
        d_out = torch.randn(2, 7, generator=g, dtype=torch.float64)
        pooled = xx.mean(1) if pool == "mean" else xx[:, 0]
        ((torch.nn.functional.layer_norm(pooled, (16,), lw, lb, R.EPS) @ hw.t() + hb) * d_out).sum().backward()
        got = R.head_bwd(xx.detach(), pool, lw.detach(), lb.detach(), hw.detach(), d_out)
        for a, ref in zip(got, (xx.grad, lw.grad, lb.grad, hw.grad, hb.grad)):
            assert R.rel_err(a, ref) < 1e-12
    img = torch.randn(2, 3, 16, 24, 3, generator=g)
    from einops import rearrange
    ref = rearrange(img.permute(0, 1, 4, 2, 3).permute(0, 2, 1, 3, 4).contiguous().view(2, 9, 16, 24), "b c (h p1) (w p2) -> b (h w) (p1 p2 c)", p1=8, p2=8)
    assert torch.equal(R.patch_rows(img, 8), ref)


# ---------------------------------------------------------------------------------------------------- host logic
def _zm(train=None, agg=None, sampling=None, embedder=None, **kw):
    from stedm_amd.latent_diffusion import S_ZSS_DM
    from stedm_amd.unet import UNetModel
    kwargs = dict(conditioning_key="hybrid", image_size=16, channels=4, cond_stage_key="segmentation", cond_stage_trainable=True,
                  cond_stage_config={"target": "ldm.modules.encoders.modules.SpatialRescaler", "params": {"n_stages": 2, "in_channels": 2, "out_channels": 3}})
    kwargs.update(kw)
    if train is not None:
        kwargs["train_style_encoder"] = train
    return S_ZSS_DM("swin_v2_t", sampling or {"name": "mp", "num_patches": 2}, agg or dict(SVIT), {"data": {"patch_size": 16}}, UNetModel(**TINY),
                    embedder=embedder, **kwargs)


def test_switch_defaults_off_and_extra_params_are_what_they_were():
    zm = _zm()
    assert zm.train_style_encoder is False and zm.agg_block.keep_for_backward is False
    tr = zm.configure_trainer()
    assert [id(p) for p in tr.extra_params] == [id(zm.cond_stage_model.channel_mapper.weight)]
    assert zm._cond_stage_in_optimizer()
    zm = _zm(train=False)
    assert [id(p) for p in zm.configure_trainer().extra_params] == [id(zm.cond_stage_model.channel_mapper.weight)]


def test_switch_on_appends_the_svit_parameters_after_logvar():
    zm = _zm(train=True, loss_type="l2", learn_logvar=True)
    tr = zm.configure_trainer()
    svit = list(zm.agg_block.parameters())
    assert len(svit) == 24
    assert [id(p) for p in tr.extra_params] == [id(zm.cond_stage_model.channel_mapper.weight), id(zm.logvar)] + [id(p) for p in svit]
    assert zm._cond_stage_in_optimizer()
    # without a trainable cond stage the encoder's parameters do not pass for the cond stage's
    zm = _zm(train=True, cond_stage_trainable=False)
    tr = zm.configure_trainer()
    assert [id(p) for p in tr.extra_params] == [id(p) for p in zm.agg_block.parameters()] and not zm._cond_stage_in_optimizer()
    with pytest.raises(NotImplementedError):          # the captured step keeps refusing parameters outside the U-Net
        z = torch.zeros(1, 4, 16, 16)
        tr.train_step_graphed(z, torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.long), torch.zeros(1, 512), z)


def test_other_aggregation_blocks_are_refused_at_construction():
    with pytest.raises(NotImplementedError):
        _zm(train=True, agg={"name": "mean"}, embedder=torch.nn.Identity())
    with pytest.raises(NotImplementedError):
        _zm(train=True, sampling={"name": "none"})
    assert _zm(train=False, agg={"name": "mean"}, embedder=torch.nn.Identity()).train_style_encoder is False


def test_backward_raises_without_a_kept_forward_and_for_fp8():
    from stedm_amd.style import sViT
    mk = lambda prec: sViT(image_size=16, patch_size=8, num_classes=32, dim=64, depth=1, heads=2, mlp_dim=64, ns=1, precision=prec)
    with pytest.raises(RuntimeError):
        mk("parity").backward(torch.zeros(1, 32))
    with pytest.raises(NotImplementedError):
        mk("fp8").backward(torch.zeros(1, 32))


def test_ldm_module_reads_the_config_key():
    from stedm_amd.ldm_module import LDM_Diffusion
    cfg = {"lr": 1e-3, "cfg_scale": 1.5, "ddim_steps": 4, "eta": 0.0, "data": {"patch_size": 16}, "style_sampling": {"name": "mp", "num_patches": 2},
           "style_agg": dict(SVIT),
           "diffusion": dict(timesteps=1000, loss_type="l1", first_stage_key="image", cond_stage_key="segmentation", image_size=16, channels=4,
                             conditioning_key="hybrid", unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(TINY)})}
    assert LDM_Diffusion(cfg)._model.train_style_encoder is False
    assert LDM_Diffusion(dict(cfg, train_style_encoder=True))._model.train_style_encoder is True
