"""GPU tier (-m gpu): what the training backward finds of the planes and {mean, rstd} that the training forward kept.

A training forward in bf16 (the backward's operand format) keeps every normalised plane it writes and, in every mode, the group
statistics its normalise passes fold (UNetModel._keep); the backward reads them back (UNetTrainer._kept16 / _kept_mr). When the two
sides disagree on a key nothing fails: the backward recomputes the plane or folds the statistics again, the numbers stay the same and
the step gets slower. This file counts the normalise passes and the statistics folds a backward issues, for the TINY net (B = 2,
16 x 16) in its four flavours - plain, use_scale_shift_norm, resblock_updown, live dropout:

  bf16: the backward recomputes only out[0]'s plane and folds only its statistics (the fused conv_out keeps neither);
  f16:  single product but not the backward's format, so no plane is kept - every site is recomputed by the pass of its own form -
        while the statistics are kept all the same.

The expected counts are what the code did before the plane policy moved into one place, recorded by running this file there."""
import pytest
import torch

from stedm_amd.utils import prng

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
B, HW, SEED = 2, 16, 6
FLAVOURS = {"plain": {}, "film": dict(use_scale_shift_norm=True), "updown": dict(resblock_updown=True), "dropout": dict(dropout=0.1)}
PASSES = ("gn_apply16c", "gn_apply16c_film", "gn_apply16c_drop", "gn_apply16c_resample", "gn_fold")
# calls during UNetTrainer.backward after one training forward, in the order of PASSES
EXPECTED = {
    ("plain", "bf16"): (1, 0, 0, 0, 1),
    ("film", "bf16"): (1, 0, 0, 0, 1),
    ("updown", "bf16"): (1, 0, 0, 0, 1),
    ("dropout", "bf16"): (1, 0, 0, 0, 1),
    ("plain", "f16"): (38, 0, 0, 0, 1),
    ("film", "f16"): (20, 18, 0, 0, 1),
    ("updown", "f16"): (42, 0, 0, 4, 1),
    ("dropout", "f16"): (20, 0, 18, 0, 1),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_backward_finds_what_the_forward_kept(dev, monkeypatch, flavour, precision):
    from stedm_amd import ops
    from stedm_amd.train import UNetTrainer
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, **FLAVOURS[flavour], **TINY)
    m.train(flavour == "dropout")
    prng.fill_module_(m, seed=SEED)
    m = m.to(dev)
    m.dropout_seed = 0xD0D0CAFE
    tr = UNetTrainer(m)
    x = prng.normal(SEED, "unet.tiny.x", (B, 7, HW, HW)).to(dev)
    ctx = prng.normal(SEED, "unet.tiny.ctx", (B, 128)).to(dev)
    target = prng.normal(SEED, "unet.tiny.target", (B, 4, HW, HW)).to(dev)
    t = torch.tensor([951, 21], device=dev)
    pred = tr.forward(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx)
    dpred = torch.empty_like(pred)
    tr.loss(pred, target, t, None, dpred)
    n = dict.fromkeys(PASSES, 0)

    def counted(name):
        real = getattr(ops, name)

        def call(*a, **k):
            n[name] += 1
            return real(*a, **k)
        return call
    for name in PASSES:
        monkeypatch.setattr(ops, name, counted(name))
    tr.backward(dpred)
    torch.cuda.synchronize()
    got = tuple(n[name] for name in PASSES)
    print(f"[kept planes {flavour} {precision}] " + " ".join(f"{name}={v}" for name, v in zip(PASSES, got)))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert got == EXPECTED[(flavour, precision)]
