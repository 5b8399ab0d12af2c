"""GPU tier (-m gpu): sViT.backward with lsa_bwd="mfma16" (the attention backward on the 16-bit matrix pipe, csrc/lsa_bwd16.hip) end to end
against the f34 golden gradients (tests/golden/f34_svit_grads.npz, the cases of test_gpu_svit_backward.py), in f16 and bf16.

Bound, per case and mode, on max-abs error over max-abs golden of every parameter's gradient: 3 x the same figure (the largest over the
parameters) of a CPU run of the restated module - refs_svit_bwd.forward with the mode's `rounder` and its explicit `backward` with the LSA
piece replaced by the contract's emulation (refs_lsa_bwd16.lsa_bwd16) - against the fp32 golden: the rule of the existing bounds with the
new roundings included. The figures are computed in the test; the run on the MI355X machine gave

    case            mode   CPU figure  bound      worst parameter (share of the bound)
    i16_ns2_d2      f16    1.67e-03    5.01e-03   1.18e-03 (0.24)
    i16_ns2_d2      bf16   8.95e-03    2.69e-02   1.32e-02 (0.49)
    i64_ns1_d1_p0   f16    8.37e-04    2.51e-03   1.07e-03 (0.43)
    i64_ns1_d1_p0   bf16   7.09e-03    2.13e-02   1.13e-02 (0.53)

accumulate=True doubles the gradients bit for bit. With ops.lsa_bwd16 patched to raise, a default ("f32") backward in f16 and in parity mode
completes: the default path runs no new code."""
import os

import numpy as np
import pytest
import torch

from tests import refs_lsa_bwd16 as E
from tests import refs_svit_bwd as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f34_svit_grads.npz")
#        tag              image ns B depth heads mlp  pool    dropout
CASES = {"i16_ns2_d2":    (16,  2, 2, 2,    3,   64,  "mean", 0.1),
         "i64_ns1_d1_p0": (64,  1, 1, 1,    2,   128, "cls",  0.0)}

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def build(tag, precision, lsa_bwd="mfma16"):
    from stedm_amd.style import sViT
    from stedm_amd.utils import prng
    img, ns, B, depth, heads, mlp, pool, p = CASES[tag]
    m = sViT(image_size=img, patch_size=8, num_classes=32, dim=64, depth=depth, heads=heads, mlp_dim=mlp, pool=pool, dropout=p, emb_dropout=p,
             ns=ns, precision=precision, lsa_bwd=lsa_bwd)
    prng.fill_module_(m, seed=34)
    for l, (attn, _ff) in enumerate(m.transformer.layers):
        attn.fn.temperature.fill_(float(np.log(64 ** -0.5)) + 0.05 * l)
    return m.train()


def figure(tag, mode, golden):
    """error of the CPU run of the restated module (operand-rounded forward, explicit backward with the emulated LSA piece) against the golden"""
    img, ns, B, depth, heads, mlp, pool, p = CASES[tag]
    P = {k: v.detach().double() for k, v in build(tag, "parity", "f32").named_parameters()}
    cfg = dict(patch=8, heads=heads, pool=pool, p_emb=p, p_drop=p)
    keeps = R.make_keeps(B, (img // 8) ** 2 + 2, 64, mlp, heads, depth, p, p, int(golden["seed"][0]))
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(R, "lsa_bwd", lambda q, k, v, t, d, keep=None, pp=0.0: E.lsa_bwd16(q, k, v, t, d, keep, pp, mode))
        _, tape = R.forward(P, torch.from_numpy(golden[tag + ".img"]).double(), cfg, keeps, rnd=R.rounder(mode))
        G = R.backward(P, tape, torch.from_numpy(golden[tag + ".g"]).double(), cfg, keeps)
    return max(R.rel_err(G[k].reshape(golden[f"{tag}.grad.{k}"].shape), torch.from_numpy(golden[f"{tag}.grad.{k}"])) for k in P
               if "to_time_embedding" not in k)


def run(m, tag, golden, dev):
    m.dropout_seed = int(golden["seed"][0])
    m.keep_for_backward = True
    return m(torch.from_numpy(golden[tag + ".img"]).to(dev))


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("tag", list(CASES))
def test_backward16_against_golden(dev, golden, tag, mode):
    m = build(tag, mode).to(dev)
    run(m, tag, golden, dev)
    m.backward(torch.from_numpy(golden[tag + ".g"]).to(dev))
    torch.cuda.synchronize()
    fig = figure(tag, mode, golden)
    bound = 3.0 * fig
    worst = 0.0
    for name, prm in m.named_parameters():
        if "to_time_embedding" in name:
            assert float(prm.grad.abs().max()) == 0.0
            continue
        e = R.rel_err(prm.grad.cpu(), torch.from_numpy(golden[f"{tag}.grad.{name}"]))
        worst = max(worst, e)
        print(f"    {name:52s} {e:.2e}")
    print(f"sViT.backward mfma16 {tag} {mode}: CPU figure {fig:.2e} bound {bound:.2e} worst {worst:.2e} = {worst / bound:.2f} of the bound")
    assert worst <= bound, f"{worst:.3e} > {bound:.3e}"


@pytest.mark.parametrize("tag", list(CASES))
def test_accumulate_doubles_bit_for_bit(dev, golden, tag):
    m = build(tag, "f16").to(dev)
    run(m, tag, golden, dev)
    g = torch.from_numpy(golden[tag + ".g"]).to(dev)
    m.backward(g)
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.backward(g, accumulate=True)
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, first[n] + first[n]), n
    m.backward(g)
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, first[n]), n


@pytest.mark.parametrize("mode", ["f16", "parity"])
def test_default_path_runs_no_new_code(dev, golden, monkeypatch, mode):
    from stedm_amd import ops

    def boom(*a, **k):
        raise AssertionError("the default path called ops.lsa_bwd16")
    monkeypatch.setattr(ops, "lsa_bwd16", boom)
    monkeypatch.setattr(ops, "lsa_bwd16_ws_bytes", boom)
    tag = "i16_ns2_d2"
    m = build(tag, mode, lsa_bwd="f32").to(dev)
    run(m, tag, golden, dev)
    m.backward(torch.from_numpy(golden[tag + ".g"]).to(dev))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
