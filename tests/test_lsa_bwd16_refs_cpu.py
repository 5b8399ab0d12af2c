"""CPU tier: the fp64 emulation of stedm_lsa_bwd16's numerics contract (tests/refs_lsa_bwd16.py) against fp64 autograd - its three roundings
must show (non-zero error) and stay small (sanity caps 1e-2 for f16, 3e-2 for bf16: an order above what randn planes give) - its exact
invariance under a power-of-two scale of dO, and the host switches: sViT(lsa_bwd=...), S_ZSS_DM(style_lsa_bwd=...)."""
import math

import pytest
import torch

from tests import refs_lsa_bwd16 as E
from tests import refs_svit_bwd as R

SEED, SITE = 0x5EED00D5, 9
TEMP = math.log(64 ** -0.5) + 0.05
QSCALE = math.exp(TEMP) * E.LOG2E
CAP = {"f16": 1e-2, "bf16": 3e-2}


def _inputs(T, p, mode, BH=3):
    from oracle import dropmask
    g = torch.Generator().manual_seed(1000 + T)
    q, k, v, dO = (torch.randn(BH, T, 64, generator=g, dtype=torch.float64) for _ in range(4))
    qp, k, v = E.R(q * QSCALE, mode), E.R(k, mode), E.R(v, mode)
    dO = dO.float().double()
    keep = torch.from_numpy(dropmask.keep_attention(BH, T, p, SEED, SITE).copy()) if p > 0 else None
    return qp, k, v, dO, keep


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", [6, 66, 130, 258])
@torch.enable_grad()
def test_emulation_against_fp64_autograd(T, p, mode):
    qp, k, v, dO, keep = _inputs(T, p, mode)
    qa, ka, va = (qp / QSCALE).requires_grad_(True), k.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ta = torch.tensor(TEMP, dtype=torch.float64, requires_grad=True)
    dots = (qa @ ka.transpose(-1, -2)) * ta.exp()
    prob = dots.masked_fill(torch.eye(T, dtype=torch.bool), -torch.finfo(dots.dtype).max).softmax(-1)
    if p > 0:
        prob = prob * (keep.double() / (1.0 - p))
    ((prob @ va) * dO).sum().backward()
    with torch.no_grad():
        got = E.lsa_bwd16_planes(qp, k, v, QSCALE, dO, keep, p, mode)
        exact = R.lsa_bwd(qp / QSCALE, k, v, torch.tensor(TEMP, dtype=torch.float64), dO, keep, p)
    for name, a, e, ref in zip(("dq", "dk", "dv", "dtemp"), got, exact, (qa.grad, ka.grad, va.grad, ta.grad)):
        assert R.rel_err(e, ref) < 1e-10                    # the unrounded formulas are the autograd result
        err = R.rel_err(a, ref)
        print(f"T={T} p={p} {mode} {name} {err:.2e}")
        assert 0.0 < err < CAP[mode], (name, err)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_emulation_is_scale_invariant(mode):
    qp, k, v, dO, keep = _inputs(66, 0.1, mode)
    a = E.lsa_bwd16_planes(qp, k, v, QSCALE, dO, keep, 0.1, mode)
    b = E.lsa_bwd16_planes(qp, k, v, QSCALE, dO * 2.0 ** -30, keep, 0.1, mode)
    for x, y in zip(a, b):
        assert torch.equal(x * 2.0 ** -30, y)
    z = E.lsa_bwd16_planes(qp, k, v, QSCALE, dO * 0.0, keep, 0.1, mode)
    assert all(bool((t == 0).all()) for t in z)
    assert E.do_scale(torch.tensor([3.0])) == 2.0 ** 9 and E.do_scale(torch.tensor([1024.0])) == 1.0 and E.do_scale(torch.zeros(2)) == 1.0


def _svit(**kw):
    from stedm_amd.style import sViT
    return sViT(image_size=16, patch_size=8, num_classes=32, dim=64, depth=1, heads=2, mlp_dim=64, ns=1, **kw)


def test_svit_lsa_bwd_keyword():
    assert _svit().lsa_bwd == "f32"
    assert _svit(lsa_bwd="mfma16", precision="f16").lsa_bwd == "mfma16"
    with pytest.raises(ValueError):
        _svit(lsa_bwd="nope")
    m = _svit()
    m.lsa_bwd = "nope"
    with pytest.raises(ValueError):
        m.backward(torch.zeros(1, 32))


def test_mfma16_refuses_the_parity_mode_without_a_device():
    with pytest.raises(ValueError):
        _svit(lsa_bwd="mfma16", precision="parity").backward(torch.zeros(1, 32))
    with pytest.raises(NotImplementedError):           # the fp8 mode keeps refusing as before
        _svit(lsa_bwd="mfma16", precision="fp8").backward(torch.zeros(1, 32))
    with pytest.raises(RuntimeError):                  # a single-product mode passes the check and then misses its kept forward
        _svit(lsa_bwd="mfma16", precision="bf16").backward(torch.zeros(1, 32))


SVIT = dict(name="svit", patch_size=8, dim=64, depth=1, heads=2, mlp_dim=64, pool="mean", channels=3, dropout=0.0, emb_dropout=0.0, t_dim=256)
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[32], channel_mult=[1, 2],
            num_heads=4)


def _zm(train=None, **kw):
    from stedm_amd.latent_diffusion import S_ZSS_DM
    from stedm_amd.unet import UNetModel
    kwargs = dict(conditioning_key="hybrid", image_size=16, channels=4, cond_stage_key="segmentation", cond_stage_trainable=True,
                  cond_stage_config={"target": "ldm.modules.encoders.modules.SpatialRescaler", "params": {"n_stages": 2, "in_channels": 2, "out_channels": 3}})
    kwargs.update(kw)
    if train is not None:
        kwargs["train_style_encoder"] = train
    return S_ZSS_DM("swin_v2_t", {"name": "mp", "num_patches": 2}, dict(SVIT), {"data": {"patch_size": 16}}, UNetModel(**TINY), **kwargs)


def test_s_zss_dm_passes_the_keyword_on():
    assert _zm(train=True).agg_block.lsa_bwd == "f32"
    assert _zm(train=True, style_lsa_bwd="mfma16").agg_block.lsa_bwd == "mfma16"
    assert _zm(style_lsa_bwd="mfma16").agg_block.lsa_bwd == "f32"          # ignored without train_style_encoder
    with pytest.raises(ValueError):
        _zm(train=True, style_lsa_bwd="nope")
