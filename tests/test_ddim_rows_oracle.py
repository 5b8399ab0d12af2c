"""CPU tier: DDIM with one guidance scale per sample (stedm_ddim_step_rows) and the epoch-end monitoring images built on it.

F26 (tests/golden/make_golden_ddim_rows.py: the reference's own DDIMSampler, one run per distinct scale, row b taken from the run at
scales[b]) is reproduced by the oracle loop of tests/test_ddim_options_oracle.py run the same way; the sampler's handling of a sequence of
scales is checked without a GPU (what reaches which op, the refusals before any device work); the new kernel's variants must not spill;
LDM_Diffusion.sample_test_images / on_train_epoch_end are checked for what they read and which two runs they make, the samplers stubbed.
The GPU tier (tests/test_gpu_ddim_rows.py) checks the kernel, the HIP sampler and the hook end to end."""
import glob
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import ddim as oddim
from tests.golden import make_golden_ddim_rows as f26
from tests.test_ddim_options_oracle import _CPUToy, ddim_opts_sample, rel, toy_eps

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_rows(apply_model, x_T, cond, uncond, scales, S, eta, noises=None):
    """The per-sample result as F26 defines it: the oracle loop once per distinct scale on the whole batch, row b from the run at
    scales[b] -> (final latents, the last iteration's pred_x0)."""
    runs = {}
    for s in sorted(set(float(v) for v in scales)):
        out, pred = ddim_opts_sample(apply_model, oddim.Schedule(), x_T, cond, S, eta=eta, uncond=uncond, scale=s, noises=noises)
        runs[s] = (out, pred[-1])
    return (torch.stack([runs[float(s)][0][b] for b, s in enumerate(scales)]),
            torch.stack([runs[float(s)][1][b] for b, s in enumerate(scales)]))


# ------------------------------------------------------------------------------------------------ F26
def test_f26_oracle_loop_per_scale_matches_the_reference_sampler(golden):
    fx = golden("f26_ddim_rows")
    assert fx["scales"].tolist() == list(f26.SCALES)
    xT, cond, unc = f26.inputs()
    for tag, eta in f26.ETAS.items():
        calls = [0]

        def am(x, t, c):
            calls[0] += 1
            return toy_eps(x, t, c)

        out, pred = oracle_rows(am, xT, cond, unc, f26.SCALES, f26.S, eta, noises=f26.noises())
        assert calls[0] == int(fx[f"{tag}_calls"])           # the scale-1 run is the unguided branch: one call per iteration
        e1, e2 = rel(out, fx[f"{tag}_out"]), rel(pred, fx[f"{tag}_pred_x0"])
        print(f"[F26 {tag}] oracle rows vs reference: out {e1:.2e}, pred_x0 {e2:.2e}")
        assert e1 < 1e-5 and e2 < 1e-5, (tag, e1, e2)
    # the scales matter: rows 1 and 3 (scale 3) differ from a run of the batch at scale 5, row 0 from a guided run
    other, _ = ddim_opts_sample(toy_eps, oddim.Schedule(), xT, cond, f26.S, eta=0.0, uncond=unc, scale=5.0)
    assert rel(other[1], fx["eta0_out"][1]) > 1e-3 and rel(other[0], fx["eta0_out"][0]) > 1e-3
    assert rel(other[2], fx["eta0_out"][2]) < 1e-5


def test_f26_regenerates_from_the_reference(golden):
    if not os.path.isdir(os.path.join(f26.reference_dir(), "ldm")):
        pytest.skip("the reference tree is not present")
    fx = golden("f26_ddim_rows")
    new = f26.generate()
    assert sorted(new) == sorted(fx.files)
    for k in fx.files:
        assert new[k].shape == fx[k].shape and new[k].dtype == fx[k].dtype, k
        assert np.allclose(new[k], fx[k], rtol=0, atol=1e-6), k


# ------------------------------------------------------------------------------------------------ host dispatch (no GPU)
class _Counting(_CPUToy):
    def __init__(self):
        super().__init__()
        self.n_calls = 0

    def apply_model(self, x, t, c):
        self.n_calls += 1
        return toy_eps(x, t, c)


@pytest.fixture
def recorded(monkeypatch):
    from stedm_amd import ops
    calls = []
    for name in ("ddim_step", "ddim_step_ex", "ddim_step_rows", "ddim_quantize_x0", "ddim_mask_blend", "plms_step", "dpm_step"):
        monkeypatch.setattr(ops, name, (lambda nm: lambda *a, **k: calls.append((nm, a, k)))(name))
    return calls


def _args(B=2):
    z = torch.zeros(B, 3, 8, 8)
    return dict(conditioning={"bias": z}, verbose=False, x_T=z.clone())


def test_a_sequence_of_scales_reaches_ddim_step_rows(recorded):
    from stedm_amd.ddim import DDIMSampler
    unc = {"bias": torch.ones(2, 3, 8, 8)}
    for scales in ([1.5, 3.0], (1.0, 3.0), np.asarray([1.5, 3.0]), torch.tensor([1.5, 3.0])):
        recorded.clear()
        toy = _Counting()
        DDIMSampler(toy).sample(5, 2, (3, 8, 8), unconditional_guidance_scale=scales, unconditional_conditioning=unc, **_args())
        assert [c[0] for c in recorded] == ["ddim_step_rows"] * 5
        assert toy.n_calls == 10                              # every row runs the conditional and the unconditional forward
        for _, a, k in recorded:
            sc = a[5]
            assert isinstance(sc, torch.Tensor) and sc.dtype == torch.float32 and tuple(sc.shape) == (2,)
            assert sc.tolist() == [float(v) for v in scales]
            assert a[2] is not None and k["noise"] is None and not k["draw"]
    # eta 1: given noises / torch's draw arrive as `noise`; noise_seed turns the in-kernel draw on
    recorded.clear()
    DDIMSampler(_Counting()).sample(5, 2, (3, 8, 8), eta=1.0, unconditional_guidance_scale=[1.5, 3.0], unconditional_conditioning=unc, **_args())
    assert [c[0] for c in recorded] == ["ddim_step_rows"] * 5 and all(c[2]["noise"] is not None and not c[2]["draw"] for c in recorded)
    recorded.clear()
    DDIMSampler(_Counting()).sample(5, 2, (3, 8, 8), eta=1.0, unconditional_guidance_scale=[1.5, 3.0], unconditional_conditioning=unc,
                                    noise_seed=11, sample_id0=4, **_args())
    k = recorded[0][2]
    assert k["draw"] and k["noise"] is None and k["seed"] == 11 and k["first_id"] == 4 and k["n_iters"] == 5
    # p_sample_ddim on its own takes the sequence too
    recorded.clear()
    smp = DDIMSampler(_Counting())
    smp.make_schedule(5, verbose=False)
    x = torch.zeros(2, 3, 8, 8)
    smp.p_sample_ddim(x, {"bias": x}, torch.full((2,), 1, dtype=torch.long), 0, unconditional_guidance_scale=[2.0, 4.0],
                      unconditional_conditioning=unc)
    assert [c[0] for c in recorded] == ["ddim_step_rows"] and recorded[0][1][5].tolist() == [2.0, 4.0]


def test_a_scalar_scale_keeps_todays_path(recorded):
    from stedm_amd.ddim import DDIMSampler
    unc = {"bias": torch.ones(2, 3, 8, 8)}
    for scale in (1.5, np.float32(1.5), np.asarray(1.5), torch.tensor(1.5)):
        recorded.clear()
        toy = _Counting()
        DDIMSampler(toy).sample(5, 2, (3, 8, 8), unconditional_guidance_scale=scale, unconditional_conditioning=unc, **_args())
        assert [c[0] for c in recorded] == ["ddim_step"] * 5 and toy.n_calls == 10
        assert all(c[2]["cfg_scale"] == 1.5 and isinstance(c[2]["cfg_scale"], float) for c in recorded)


def test_all_ones_or_no_unconditional_conditioning_is_the_unguided_run(recorded):
    from stedm_amd.ddim import DDIMSampler
    unc = {"bias": torch.ones(2, 3, 8, 8)}
    for kw in (dict(unconditional_guidance_scale=[1.0, 1.0], unconditional_conditioning=unc),
               dict(unconditional_guidance_scale=[3.0, 5.0], unconditional_conditioning=None)):
        recorded.clear()
        toy = _Counting()
        DDIMSampler(toy).sample(5, 2, (3, 8, 8), **kw, **_args())
        assert toy.n_calls == 5                               # one forward per step, as the reference's branch ddim.py:170-171
        assert [c[0] for c in recorded] == ["ddim_step"] * 5 and all(c[1][2] is None for c in recorded)       # e_u is None


def test_refusals_with_per_sample_scales_raise_before_any_op(recorded):
    from stedm_amd.ancestral import AncestralSampler
    from stedm_amd.ddim import DDIMSampler
    from stedm_amd.dpm_solver import DPMSolverSampler
    from stedm_amd.plms import PLMSSampler
    unc = {"bias": torch.ones(2, 3, 8, 8)}
    toy = _Counting()
    smp = DDIMSampler(toy)
    g = dict(unconditional_conditioning=unc)
    for bad in ([1.5], [1.5, 3.0, 5.0], torch.tensor([1.5, 2.0, 3.0]), [[1.5, 3.0]]):
        with pytest.raises(ValueError):
            smp.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=bad, **g, **_args())
    for bad in ([1.5, float("nan")], [float("inf"), 2.0]):
        with pytest.raises(ValueError):
            smp.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=bad, **g, **_args())
    with pytest.raises(NotImplementedError):
        smp.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=[1.5, 3.0], quantize_x0=True, **g, **_args())
    with pytest.raises(NotImplementedError):
        smp.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=[1.5, 3.0], eta=1.0, temperature=0.7, **g, **_args())
    with pytest.raises(NotImplementedError):
        smp.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=[1.5, 3.0], eta=0.5, noise_dropout=0.2, **g, **_args())
    for other in (PLMSSampler(toy), DPMSolverSampler(toy, device=torch.device("cpu"))):
        with pytest.raises(NotImplementedError, match="DDIMSampler"):
            other.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=[1.5, 3.0], **g, **_args())
    with pytest.raises(NotImplementedError, match="DDIMSampler"):
        AncestralSampler(toy).sample({"bias": torch.zeros(2, 3, 8, 8)}, batch_size=2, unconditional_guidance_scale=[1.5, 3.0], **g)
    assert recorded == [] and toy.n_calls == 0
    # eta 0: temperature and noise_dropout change nothing (sigma == 0), as for one scale
    smp.sample(5, 2, (3, 8, 8), unconditional_guidance_scale=[1.5, 3.0], eta=0.0, temperature=0.5, noise_dropout=0.3, **g, **_args())
    assert [c[0] for c in recorded] == ["ddim_step_rows"] * 5


# ------------------------------------------------------------------------------------------------ the built kernel
def test_ddim_step_rows_variants_have_no_register_spills():
    """The code-object notes of sampler.o (the way tests/test_abi.py reads them): every instantiation of ddim_step_kernel - for
    stedm_ddim_step_rows (DdimRowsForm) the register forms up to the 24 elements a thread holds at the native 3 x 128 x 128 latent and the
    looped form, each with and without the in-kernel draw; and every form of the scalar entries - keeps `.vgpr_spill_count` and
    `.sgpr_spill_count` 0."""
    from stedm_amd import build
    build.build(verbose=False)
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    obj = os.path.join(ROOT, "stedm_amd", "csrc", "sampler.o")
    if not all(os.path.exists(x) for x in (obj, objdump, readelf)):
        pytest.skip("built objects / llvm tools not present")
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(obj, os.path.join(d, "x.o"))
        subprocess.run([objdump, "--offloading", "x.o"], cwd=d, capture_output=True)
        dev = glob.glob(os.path.join(d, "x.o.*gfx950"))
        assert dev, "no gfx950 code object in sampler.o"
        notes = subprocess.run([readelf, "--notes", dev[0]], capture_output=True, text=True).stdout
    kname, seen = None, set()
    for ln in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", ln)
        if m:
            kname = m.group(1)
        m = re.match(r"\s+\.(vgpr|sgpr)_spill_count:\s+(\d+)", ln)
        if m and kname and "ddim_step_kernel" in kname:
            seen.add(kname)
            assert int(m.group(2)) == 0, f"{kname} spills {m.group(2)} {m.group(1)}s"
    rows = {k for k in seen if "DdimRowsForm" in k}
    assert len(rows) == 12 and len(seen - rows) == 16, sorted(seen)          # R in {0, 2, 4, 8, 16, 24} x DRAW; R in {0, 4, 8, 16} x DRAW x EXT
    assert any("Li24E" in k for k in rows) and any("Li0E" in k for k in rows), sorted(rows)


# ------------------------------------------------------------------------------------------------ sample_test_images plumbing
class _FakeModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.inner = torch.nn.Linear(2, 2)
        self.channels, self.image_size, self.use_graph = 3, 6, False
        self.device = torch.device("cpu")

    def decode_first_stage(self, z):
        return torch.zeros(z.shape[0], 3, 24, 24) + z[:, :1, :1, :1]


def _module(sampling, style_drop_rate, data=None):
    from stedm_amd.ldm_module import LDM_Diffusion, _Cfg
    mod = LDM_Diffusion.__new__(LDM_Diffusion)
    torch.nn.Module.__init__(mod)
    mod._cfg = _Cfg({"style_sampling": sampling, "style_drop_rate": style_drop_rate, "data": data or {}, "location": {"data_dir": "/nowhere"}})
    mod._model = _FakeModel()
    mod._wandb_id = ""
    mod._loss_sum, mod._loss_n = torch.tensor(3.0), 2
    return mod


def _write_folder(root, sampling):
    from PIL import Image
    g = np.random.default_rng(5)
    seg = (g.random((24, 24)) > 0.5).astype(np.uint8) * 200
    Image.fromarray(seg, mode="L").save(os.path.join(root, "test_c.png"))
    os.makedirs(os.path.join(root, sampling["name"]), exist_ok=True)
    files = {}
    names = [f"{i}_img.png" for i in range(4)] if sampling["name"] == "nearby" else \
            [f"{i}_img_{k}.png" for i in range(4) for k in range(sampling.get("num_patches", 0))] if sampling["name"] == "mp" else []
    for n in names:
        a = g.integers(0, 256, (24, 24, 4), dtype=np.uint8)          # RGBA: the alpha channel is dropped
        Image.fromarray(a, mode="RGBA").save(os.path.join(root, sampling["name"], n))
        files[n] = a[:, :, :3].astype(np.float32) / 127.5 - 1
    return seg, files


@pytest.fixture
def stubbed(monkeypatch):
    from stedm_amd import ldm_module
    runs = []

    def predict_latents(model, batch, **kw):
        runs.append(dict(batch={k: v.clone() for k, v in batch.items()}, kw=kw, use_graph=model.use_graph, training=model.training))
        return torch.full((len(batch["image"]), 3, 6, 6), float(len(runs)))

    monkeypatch.setattr(ldm_module, "predict_latents", predict_latents)
    monkeypatch.setattr(ldm_module, "images_for_saving", lambda dec, seg=None: (dec.permute(0, 2, 3, 1).to(torch.uint8), None))
    return runs


@pytest.mark.parametrize("sampling", [{"name": "nearby"}, {"name": "mp", "num_patches": 2}, {"name": "dummy"}], ids=lambda s: s["name"])
def test_sample_test_images_reads_the_folder_and_makes_the_two_runs(tmp_path, stubbed, sampling):
    from stedm_amd import parallel as par
    seg, files = _write_folder(str(tmp_path), sampling)
    mod = _module(sampling, 0.1)
    mod.train()
    mod._model.inner.eval()                                   # a mixed state, to be restored as it was
    out = mod.sample_test_images(str(tmp_path), seed=9)
    assert mod.training and mod._model.training and not mod._model.inner.training and mod._model.use_graph is False
    guided = sampling["name"] != "dummy"
    assert len(stubbed) == (2 if guided else 1)
    assert sorted(out) == (["Sample Images", "Sample Images CFG"] if guided else ["Sample Images"])
    onehot = np.stack([seg == 0, seg > 0], -1).astype(np.float32)
    num = sampling.get("num_patches", 1)
    style = lambda i: np.stack([files[f"{i}_img.png" if sampling["name"] == "nearby" else f"{i}_img_{k}.png"] for k in range(num)]) \
        if guided else np.full((1, 24, 24, 3), -1.0, dtype=np.float32)
    expect = [([0, 1, 2, 3], 1.0, 0)] + ([([0, 0, 1, 1], [3.0, 5.0, 3.0, 5.0], 4)] if guided else [])
    for run, (rows, scale, first) in zip(stubbed, expect):
        assert run["use_graph"] is True and run["training"] is False
        kw = run["kw"]
        assert kw["cfg_scale"] == scale and kw["eta"] == 0.0 and kw["ddim_steps"] == 128 and kw["style_sampling"] == sampling["name"]
        assert torch.equal(kw["x_T"], par.per_sample_normal(9, list(range(first, first + 4)), (3, 6, 6), stream=0))
        b = run["batch"]
        assert tuple(b["image"].shape) == (4, 24, 24, 3) and not b["image"].any()
        assert np.array_equal(b["segmentation"].numpy(), np.broadcast_to(onehot, (4, 24, 24, 2)))
        assert tuple(b["style_imgs"].shape) == (4, num, 24, 24, 3)
        for r, i in enumerate(rows):
            assert np.array_equal(b["style_imgs"][r].numpy(), style(i)), (r, i)
    for k, (title, imgs) in enumerate(sorted(out.items())):
        assert len(imgs) == 4 and all(im.dtype == np.uint8 and im.shape == (24, 24, 3) for im in imgs)
        assert all(int(im[0, 0, 0]) == k + 1 for im in imgs)          # each batch decoded once, from its own run's latents


def test_no_guided_run_without_style_dropout_and_the_epoch_end_hook(tmp_path, stubbed):
    sampling = {"name": "nearby"}
    _write_folder(str(tmp_path), sampling)
    mod = _module(sampling, 0.0)
    out = mod.sample_test_images(str(tmp_path), ddim_steps=7)
    assert len(stubbed) == 1 and sorted(out) == ["Sample Images"] and stubbed[0]["kw"]["ddim_steps"] == 7
    # the hook: default folder from the config, logger calls with the reference's titles and captions, the loss accumulator reset
    stubbed.clear()
    mod = _module(sampling, 0.2, data={"test_folder": "t"})
    mod._cfg["location"]["data_dir"] = str(tmp_path.parent)
    os.rename(str(tmp_path), os.path.join(str(tmp_path.parent), "t"))
    logged = []
    mod.logger = type("L", (), {"version": "run7", "log_image": lambda self, title, images, caption: logged.append((title, len(images), caption))})()
    mod.on_train_epoch_end()
    assert len(stubbed) == 2 and sorted(mod.last_test_images) == ["Sample Images", "Sample Images CFG"]
    caps = ["Test 0", "Test 1", "Test 2", "Test 3"]
    assert logged == [("Sample Images CFG", 4, caps), ("Sample Images", 4, caps)]
    assert mod._wandb_id == "run7" and mod._loss_sum is None and mod._loss_n == 0
    # no test_folder in the config: the loss is still taken, nothing is sampled
    stubbed.clear()
    mod = _module(sampling, 0.2)
    mod.on_train_epoch_end()
    assert stubbed == [] and mod.last_test_images == {} and mod._loss_n == 0
