"""GPU tier (-m gpu): DDIM with one guidance scale per sample - the kernel (stedm_ddim_step_rows) row by row against the oracle's
cfg_combine / ddim_update, its properties (scale-1 rows never read e_u, a row depends on itself alone, the in-kernel draw, graph replay
reading the scales), the HIP sampler eager and graphed against the oracle loop and F26, sharded prediction with per-sample scales, and
LDM_Diffusion's epoch-end images end to end. The per-sample result is defined as in tests/test_ddim_rows_oracle.py: a run of the whole
batch at scales[b], row b taken."""
import os

import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests.test_ddim_options_oracle import rel
from tests.test_gpu_kernels import rel_err

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CYCLE = [1.0, 3.0, 5.0, 1.5, 7.5]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _operands(shape, seed=7):
    """test_ddim_step's operands"""
    x = prng.normal(seed, "dd.x", shape)
    ec = prng.normal(seed, "dd.ec", shape)
    eu = prng.normal(seed, "dd.eu", shape) * 0.8 + 0.1 * ec
    nz = prng.normal(seed, "dd.nz", shape)
    return x, ec, eu, nz


def _table(dev, eta, n=20):
    from oracle import ddim as od
    ds = od.DDIMSchedule(od.Schedule(), n, eta)
    return ds, torch.tensor([ds.scalars(i) for i in range(n)], dtype=torch.float32, device=dev)


def _rows(dev, x, ec, eu, table, scales, idx=10, **kw):
    from stedm_amd import ops
    xp, x0 = torch.empty(x.shape, device=dev), torch.empty(x.shape, device=dev)
    step = torch.tensor([idx], dtype=torch.int32, device=dev)
    sc = scales if isinstance(scales, torch.Tensor) else torch.tensor(scales, dtype=torch.float32, device=dev)
    ops.ddim_step_rows(x.to(dev), ec.to(dev), None if eu is None else eu.to(dev), table, xp, sc, pred_x0=x0, step_idx=step, **kw)
    return xp, x0


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("shape", [(3, 4, 32, 32), (2, 3, 40, 40), (2, 3, 128, 128), (5, 4, 8, 8), (2, 4, 12, 24)])
def test_ddim_step_rows_vs_oracle_row_by_row(dev, shape, eta):
    """(3,4,32,32): 8 elements per thread, two chunks; (2,3,40,40): C H = 120 and W = 40, neither a multiple of 16; (2,3,128,128): the native
    latent, 24 elements per thread, 8 workgroups per sample; (5,4,8,8): W below the chunk, every scale of the cycle; (2,4,12,24): H != W."""
    from oracle import ddim as od
    x, ec, eu, nz = _operands(shape)
    scales = [CYCLE[b % 5] for b in range(shape[0])]
    ds, table = _table(dev, eta)
    noise = nz if eta else None
    xp, x0 = _rows(dev, x, ec, eu, table, scales, noise=None if noise is None else noise.to(dev))
    for b, s in enumerate(scales):
        r = slice(b, b + 1)
        e = ec[r] if s == 1.0 else od.cfg_combine(ec[r], eu[r], s)
        xp_ref, x0_ref = od.ddim_update(x[r], e, *ds.scalars(10), noise=None if noise is None else noise[r])
        e1, e2 = rel_err(xp[r], xp_ref), rel_err(x0[r], x0_ref)
        print(f"[ddim_step_rows {shape} eta {eta} row {b} scale {s}] x_prev {e1:.2e} pred_x0 {e2:.2e}")
        assert e1 < 2e-5 and e2 < 2e-5, (b, s)


def test_scale_one_rows_ignore_e_u(dev):
    shape = (4, 3, 40, 40)
    x, ec, eu, nz = _operands(shape)
    scales = [1.0, 3.0, 1.0, 5.0]
    _, table = _table(dev, 1.0)
    ref = _rows(dev, x, ec, eu, table, scales, noise=nz.to(dev))
    bad = eu.clone()
    bad[0] = float("nan")
    bad[2] = float("nan")
    got = _rows(dev, x, ec, bad, table, scales, noise=nz.to(dev))
    for a, b in zip(got, ref):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    # and they are the unguided update: the same entry without e_u
    plain = _rows(dev, x, ec, None, table, scales, noise=nz.to(dev))
    assert torch.equal(plain[0][0], ref[0][0]) and torch.equal(plain[0][2], ref[0][2]) and not torch.equal(plain[0][1], ref[0][1])


@pytest.mark.parametrize("chw", [(3, 128, 128), (3, 40, 40)])
def test_a_row_depends_only_on_itself(dev, chw):
    shape = (4,) + chw
    x, ec, eu, nz = _operands(shape)
    scales = [3.0, 1.0, 5.0, 1.5]
    _, table = _table(dev, 1.0)
    full = _rows(dev, x, ec, eu, table, scales, noise=nz.to(dev))
    one = _rows(dev, x[2:3], ec[2:3], eu[2:3], table, scales[2:3], noise=nz[2:3].to(dev))
    assert torch.equal(full[0][2:3], one[0]) and torch.equal(full[1][2:3], one[1])


def test_in_kernel_draw_equals_the_philox_rows(dev):
    from stedm_amd import ops
    shape = (3, 3, 40, 40)
    x, ec, eu, _ = _operands(shape)
    scales = [3.0, 1.0, 5.0]
    _, table = _table(dev, 1.0)
    n_iters, idx, seed = 20, 10, 1234
    nz = ops.philox_normal(3, shape[1:], seed, 1 + n_iters - 1 - idx, dev, first_id=5)
    given = _rows(dev, x, ec, eu, table, scales, idx=idx, noise=nz)
    drawn = _rows(dev, x, ec, eu, table, scales, idx=idx, draw=True, n_iters=n_iters, seed=seed, first_id=5)
    assert torch.equal(given[0], drawn[0]) and torch.equal(given[1], drawn[1])
    none = _rows(dev, x, ec, eu, table, scales, idx=idx)
    assert not torch.equal(none[0], drawn[0])


def test_graph_replay_reads_the_scales(dev):
    from stedm_amd import ops
    shape = (4, 4, 32, 32)
    x, ec, eu, _ = _operands(shape)
    _, table = _table(dev, 0.0)
    xd, ecd, eud = x.to(dev), ec.to(dev), eu.to(dev)
    sc = torch.tensor([3.0, 1.0, 5.0, 1.5], dtype=torch.float32, device=dev)
    step = torch.tensor([10], dtype=torch.int32, device=dev)
    xp, x0 = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
    ops.ddim_step_rows(xd, ecd, eud, table, xp, sc, pred_x0=x0, step_idx=step)
    first = xp.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = ops.Graph()
        with g:
            ops.ddim_step_rows(xd, ecd, eud, table, xp, sc, pred_x0=x0, step_idx=step)
        new = torch.tensor([1.0, 7.5, 2.0, 1.0], dtype=torch.float32, device=dev)
        sc.copy_(new)                      # in place: the captured launch holds the pointer, not the values
        xp.zero_()
        g.launch()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    want, want0 = _rows(dev, x, ec, eu, table, new)
    assert torch.equal(xp, want) and torch.equal(x0, want0) and not torch.equal(xp, first)


# ------------------------------------------------------------------------------------------------ the sampler, TINY U-Net
def _tiny(dev, use_graph, precision="parity"):
    from tests.test_gpu_sampler import make
    return make(dev, use_graph, precision)


def _conds(dev, cc, ctx, ctx_u):
    return ({"c_concat": [cc.to(dev)], "c_crossattn": [ctx.to(dev)]}, {"c_concat": [cc.to(dev)], "c_crossattn": [ctx_u.to(dev)]})


@pytest.fixture(scope="module")
def oracle_runs():
    """the oracle loop on the TINY inputs, once per scale the sampler tests use (1.0: the unguided loop)"""
    from tests.test_gpu_sampler import inputs, oracle_sample
    xT, cc, ctx, ctx_u = inputs()
    return {s: oracle_sample(xT, cc, ctx, ctx_u if s != 1.0 else None, 5, 0.0, s) for s in (1.0, 1.5, 3.0)}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("scales", [[1.5, 3.0], [1.0, 3.0]])
def test_ddim_rows_loop_vs_oracle(dev, oracle_runs, scales, use_graph):
    from tests.test_gpu_sampler import inputs
    xT, cc, ctx, ctx_u = inputs()
    ld = _tiny(dev, use_graph)
    cond, unc = _conds(dev, cc, ctx, ctx_u)
    s, inter = ld.sample_log(cond, 2, True, 5, eta=0.0, x_T=xT.to(dev), unconditional_conditioning=unc,
                             unconditional_guidance_scale=scales, log_every_t=1000)
    ref = torch.stack([oracle_runs[sc][b] for b, sc in enumerate(scales)])
    err = rel(s.cpu(), ref)
    print(f"[ddim rows x5 scales {scales}, graph={use_graph}] max|diff|/std vs the oracle loop per scale: {err:.3e}")
    assert err < 1e-3
    assert len(inter["x_inter"]) == 3


def test_ddim_rows_graph_equals_eager_bits(dev):
    from tests.test_gpu_sampler import inputs
    xT, cc, ctx, ctx_u = inputs()
    outs = []
    for g in (False, True):
        ld = _tiny(dev, g, "f16")
        cond, unc = _conds(dev, cc, ctx, ctx_u)
        s, _ = ld.sample_log(cond, 2, True, 5, eta=0.0, x_T=xT.to(dev), unconditional_conditioning=unc,
                             unconditional_guidance_scale=[1.5, 3.0])
        outs.append(s.clone())
    assert torch.equal(outs[0], outs[1])


def test_set_scales_on_a_captured_step_graph(dev):
    from stedm_amd.ddim import DDIMSampler, StepGraph
    from tests.test_gpu_sampler import inputs
    xT, cc, ctx, ctx_u = inputs()
    ld = _tiny(dev, True, "f16")
    cond, unc = _conds(dev, cc, ctx, ctx_u)
    smp = DDIMSampler(ld, use_graph=True)
    smp.make_schedule(5, ddim_eta=0.0, verbose=False)
    n = smp.ddim_timesteps.shape[0]

    def run(sg, img):
        img.copy_(xT.to(dev))
        sg.reset(n - 1)
        first = sg.graph is None
        if first:
            sg.step_eager()                # packs weights and allocates every buffer before capture
        with sg.stream_ctx():
            if first:
                sg.capture()
            for _ in range(n - 1 if first else n):
                sg.replay()
        sg.join()
        torch.cuda.synchronize()
        return img.clone()

    img = torch.empty_like(xT, device=dev)
    sg = StepGraph(smp, img, cond, unc, [1.5, 3.0])
    a = run(sg, img)
    sg.set_scales([5.0, 1.0])
    b = run(sg, img)                      # every step replayed from the graph captured with the first scales
    img2 = torch.empty_like(xT, device=dev)
    fresh = run(StepGraph(smp, img2, cond, unc, [5.0, 1.0]), img2)
    assert torch.equal(b, fresh) and not torch.equal(a, b)
    with pytest.raises(ValueError):
        sg.set_scales([1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        StepGraph(smp, img2, cond, unc, 1.5).set_scales([1.0, 2.0])


# ------------------------------------------------------------------------------------------------ F26 on the HIP sampler
@pytest.mark.parametrize("tag", ["eta0", "eta1"])
def test_f26_on_the_hip_sampler(dev, golden, tag):
    from stedm_amd.ddim import DDIMSampler
    from tests.golden import make_golden_ddim_rows as f26
    from tests.test_gpu_masked_sampler import GpuToy
    fx = golden("f26_ddim_rows")
    xT, cond, unc = f26.inputs()
    d = lambda c: {"bias": c["bias"].to(dev)}
    toy = GpuToy(dev)
    s, inter = DDIMSampler(toy).sample(f26.S, 4, (3, 8, 8), d(cond), verbose=False, eta=f26.ETAS[tag], x_T=xT.to(dev),
                                       unconditional_guidance_scale=list(f26.SCALES), unconditional_conditioning=d(unc),
                                       noises=f26.noises() if f26.ETAS[tag] else None, log_every_t=1)
    assert toy.calls == 2 * f26.ITERS                      # every row through both forwards: the scale-1 row pays its unconditional share
    e1, e2 = rel(s.cpu(), fx[f"{tag}_out"]), rel(inter["pred_x0"][-1].cpu(), fx[f"{tag}_pred_x0"])
    print(f"[F26 {tag} on the HIP sampler] max|diff|/std out {e1:.3e} pred_x0 {e2:.3e}")
    assert e1 < 1e-4 and e2 < 1e-4


# ------------------------------------------------------------------------------------------------ sharded prediction
def test_sharded_with_per_sample_scales_equals_the_explicit_path(dev):
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import predict_latents, predict_latents_sharded
    from tests.test_gpu_sharded import GLOBAL_B, SEED, STEPS, _batch, _model
    model = _model(dev)
    scales = [1.5, 3.0, 1.0, 5.0, 2.0, 7.5, 1.0, 3.0]
    assert len(scales) == GLOBAL_B
    rank, world = 1, 2
    lo, hi = par.shard_range(GLOBAL_B, rank, world)
    batch = _batch(list(range(lo, hi)), dev)
    got = predict_latents_sharded(model, batch, GLOBAL_B, STEPS, eta=0.0, cfg_scale=scales, seed=SEED, rank=rank, world=world, gather=False)
    x_T = par.per_sample_normal_device(SEED, lo, hi - lo, (4, 32, 32), 0, dev)
    ref = predict_latents(model, batch, STEPS, eta=0.0, cfg_scale=scales[lo:hi], x_T=x_T)
    assert torch.equal(got, ref)
    shard = predict_latents_sharded(model, batch, GLOBAL_B, STEPS, eta=0.0, cfg_scale=scales[lo:hi], seed=SEED, rank=rank, world=world,
                                    gather=False)
    assert torch.equal(shard, ref)
    with pytest.raises(ValueError):
        predict_latents_sharded(model, batch, GLOBAL_B, STEPS, cfg_scale=scales[:3], seed=SEED, rank=rank, world=world, gather=False)


# ------------------------------------------------------------------------------------------------ epoch end, end to end
def _write_test_folder(root, num):
    from PIL import Image
    g = np.random.default_rng(11)
    Image.fromarray(((g.random((64, 64)) > 0.5) * 255).astype(np.uint8), mode="L").save(os.path.join(root, "test_c.png"))
    os.makedirs(os.path.join(root, "mp"))
    for i in range(4):
        for k in range(num):
            Image.fromarray(g.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(os.path.join(root, "mp", f"{i}_img_{k}.png"))


def test_epoch_end_images_end_to_end(dev, tmp_path):
    from PIL import Image
    from stedm_amd import parallel as par
    from stedm_amd.latent_diffusion import images_for_saving, predict_latents
    from stedm_amd.ldm_module import LDM_Diffusion
    from tests.test_gpu_train import _PoolStage, _module_cfg
    cfg = _module_cfg()
    cfg["style_agg"] = dict(cfg["style_agg"], depth=2)
    cfg["style_drop_rate"] = 0.1
    cfg["data"] = dict(cfg["data"], test_folder="test")
    cfg["location"] = {"data_dir": str(tmp_path)}
    folder = os.path.join(str(tmp_path), "test")
    os.makedirs(folder)
    _write_test_folder(folder, 2)
    mod = LDM_Diffusion(cfg)
    mod._model.first_stage_model = _PoolStage()
    prng.fill_module_(mod._model.model.diffusion_model, seed=6)
    prng.fill_module_(mod._model.cond_stage_model, seed=9)
    prng.fill_module_(mod._model.agg_block, seed=51)
    mod = mod.to(dev)
    mod.train()
    out = mod.sample_test_images(ddim_steps=4, seed=21)
    assert mod.training and mod._model.training
    assert sorted(out) == ["Sample Images", "Sample Images CFG"]
    for imgs in out.values():
        assert len(imgs) == 4 and all(im.dtype == np.uint8 and im.shape == (64, 64, 3) for im in imgs)
    assert not np.array_equal(out["Sample Images CFG"][0], out["Sample Images CFG"][1])          # same style, scales 3 and 5
    assert not np.array_equal(out["Sample Images"][0], out["Sample Images"][1])

    # guided image 0 from a direct predict_latents call on the same rows, scales and per-sample x_T
    m = mod._model.eval()
    seg = (np.array(Image.open(os.path.join(folder, "test_c.png")).convert("L")) > 0).astype(np.int64)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(seg), 2).float()[None].expand(4, -1, -1, -1).contiguous()
    sty = [torch.stack([torch.from_numpy(np.array(Image.open(os.path.join(folder, "mp", f"{i}_img_{k}.png")))).float() / 127.5 - 1
                        for k in range(2)]) for i in (0, 0, 1, 1)]
    batch = {"image": torch.zeros(4, 64, 64, 3, device=dev), "segmentation": onehot.to(dev), "style_imgs": torch.stack(sty).to(dev)}
    graph = m.use_graph
    m.use_graph = True
    lat = predict_latents(m, batch, ddim_steps=4, eta=0.0, cfg_scale=[3.0, 5.0, 3.0, 5.0], style_sampling="mp",
                          x_T=par.per_sample_normal_device(21, 4, 4, (4, 16, 16), 0, dev))
    m.use_graph = graph
    img, _ = images_for_saving(m.decode_first_stage(lat))
    assert np.array_equal(img.cpu().numpy()[0], out["Sample Images CFG"][0])

    # the hook without a logger (and without Lightning): images kept, loss accumulator reset
    mod._loss_sum, mod._loss_n = torch.tensor(2.0, device=dev), 4
    mod.sample_test_images = lambda *a, **k: out
    mod.on_train_epoch_end()
    assert mod.last_test_images is out and mod._loss_sum is None and mod._loss_n == 0
