"""GPU tier (-m gpu): stedm_amd.style.sViT.backward end to end against the f34 golden gradients (the reference's own set-ViT under torch
autograd, tests/golden/make_golden_svit_grads.py), both cases, every precision mode.

Bound, per precision mode and case, on max-abs error over max-abs golden of every parameter's gradient: 3 x the same figure (the largest over
the parameters) of a CPU torch-autograd run of the restated module (tests/refs_svit_bwd.py) with the operands of its Linears and of its two
attention products rounded to the mode's operand format, against the fp32 golden. The figures were measured on the CPU, without the code
under test (FIGURES below; tests/refs_svit_bwd.py::autograd_grads with `rounder(mode)` reproduces them, and each test prints what that run
gives on the machine it runs on - the low bits of torch's CPU matmuls move it by up to a third between machines, which is why the bound
uses the recorded figures):

    case            f16        bf16       parity (fp16 hi + lo)
    i16_ns2_d2      2.46e-03   1.09e-02   1.59e-06
    i64_ns1_d1_p0   1.12e-03   9.08e-03   8.43e-07

Measured on the MI355X, worst parameter per case (error = share of its bound): i16_ns2_d2 parity 3.87e-06 (0.81), f16 1.51e-03 (0.20),
bf16 1.29e-02 (0.39); i64_ns1_d1_p0 parity 1.90e-06 (0.75), f16 9.74e-04 (0.29), bf16 9.44e-03 (0.35).

accumulate=True doubles the gradients bit for bit; with keep_for_backward = False the forward's output bits are unchanged."""
import os

import numpy as np
import pytest
import torch

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


def build(tag, precision):
    from stedm_amd.style import sViT
    from stedm_amd.utils import prng
    img, ns, B, depth, heads, mlp, pool, p = CASES[tag]
    m = sViT(image_size=img, patch_size=8, num_classes=32, dim=64, depth=depth, heads=heads, mlp_dim=mlp, pool=pool, dropout=p, emb_dropout=p,
             ns=ns, precision=precision)
    prng.fill_module_(m, seed=34)
    for l, (attn, _ff) in enumerate(m.transformer.layers):
        attn.fn.temperature.fill_(float(np.log(64 ** -0.5)) + 0.05 * l)
    return m.train()


FIGURES = {("i16_ns2_d2", "f16"): 2.46e-03, ("i16_ns2_d2", "bf16"): 1.09e-02, ("i16_ns2_d2", "parity"): 1.59e-06,
           ("i64_ns1_d1_p0", "f16"): 1.12e-03, ("i64_ns1_d1_p0", "bf16"): 9.08e-03, ("i64_ns1_d1_p0", "parity"): 8.43e-07}
_FIG = {}


def figure(tag, mode, golden):
    """error of the operand-rounded CPU autograd run against the fp32 golden: the largest parameter's figure"""
    if (tag, mode) not in _FIG:
        img, ns, B, depth, heads, mlp, pool, p = CASES[tag]
        m = build(tag, "parity")
        P = {k: v.detach().clone() for k, v in m.named_parameters()}
        cfg = dict(patch=8, heads=heads, pool=pool, p_emb=p, p_drop=p)
        keeps = R.make_keeps(B, (img // 8) ** 2 + 2, 64, mlp, heads, depth, p, p, int(golden["seed"][0]))
        _, gr = R.autograd_grads(P, torch.from_numpy(golden[tag + ".img"]), torch.from_numpy(golden[tag + ".g"]), cfg, keeps, torch.float32,
                                 rnd=R.rounder(mode))
        _FIG[(tag, mode)] = max(R.rel_err(gr[k], torch.from_numpy(golden[f"{tag}.grad.{k}"])) for k in P if "to_time_embedding" not in k)
    return _FIG[(tag, mode)]


def run(m, tag, golden, dev, keep=True):
    m.dropout_seed = int(golden["seed"][0])
    m.keep_for_backward = keep
    return m(torch.from_numpy(golden[tag + ".img"]).to(dev))


@pytest.mark.parametrize("mode", ["parity", "f16", "bf16"])
@pytest.mark.parametrize("tag", list(CASES))
def test_backward_against_golden(dev, golden, tag, mode):
    m = build(tag, mode).to(dev)
    out = run(m, tag, golden, dev)
    g = torch.from_numpy(golden[tag + ".g"]).to(dev)
    m.backward(g)
    torch.cuda.synchronize()
    fig = FIGURES[(tag, mode)]
    bound = 3.0 * fig
    print(f"sViT.backward {tag} {mode}: forward error {R.rel_err(out.cpu(), torch.from_numpy(golden[tag + '.out'])):.2e}; bound {bound:.2e} "
          f"(CPU operand-rounding figure {fig:.2e} recorded, {figure(tag, mode, golden):.2e} on this machine)")
    worst = 0.0
    for name, prm in m.named_parameters():
        gold = torch.from_numpy(golden[f"{tag}.grad.{name}"])
        assert prm.grad is not None and tuple(prm.grad.shape) == tuple(gold.shape), name
        if "to_time_embedding" in name:
            assert float(prm.grad.abs().max()) == 0.0
            continue
        e = R.rel_err(prm.grad.cpu(), gold)
        worst = max(worst, e)
        print(f"    {name:52s} {e:.2e}")
        assert e <= bound, f"{name}: {e:.3e} > {bound:.3e}"
    print(f"  worst {worst:.2e} = {worst / bound:.2f} of the bound")


@pytest.mark.parametrize("tag", list(CASES))
def test_accumulate_doubles_bit_for_bit(dev, golden, tag):
    m = build(tag, "parity").to(dev)
    run(m, tag, golden, dev)
    g = torch.from_numpy(golden[tag + ".g"]).to(dev)
    m.backward(g)
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.backward(g, accumulate=True)
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, first[n] + first[n]), n
    m.backward(g)                                    # and without it the gradients are rewritten
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, first[n]), n


@pytest.mark.parametrize("mode", ["parity", "f16"])
@pytest.mark.parametrize("tag", list(CASES))
def test_keep_flag_leaves_the_forward_bits(dev, golden, tag, mode):
    m = build(tag, mode).to(dev)
    a = run(m, tag, golden, dev, keep=False).clone()
    assert m._tape is None
    with pytest.raises(RuntimeError):
        m.backward(torch.zeros_like(a))
    b = run(m, tag, golden, dev, keep=True).clone()
    assert m._tape is not None and len(m._tape["xa"]) == len(m._tape["xf"]) == m.depth
    assert torch.equal(a, b)
