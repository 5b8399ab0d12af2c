"""GPU tier: gradient-norm clipping and scheduled learning rates of the fused training step. The norm kernel alone against a float64
reference (tests/refs_clip.py), the optimizer kernels with the device coefficient against torch.nn.utils.clip_grad_norm_ + the oracle's AdamW /
EMA, the trainer under accumulation, graph capture and two ranks, and the LatentDiffusion surface."""
import math

import numpy as np
import pytest
import torch

from stedm_amd.utils import prng
from tests import refs_clip

pytestmark = pytest.mark.gpu

TINY = refs_clip.TINY
CAP = dict(image_size=16, in_channels=7, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=[32, 16, 8], channel_mult=[1, 4, 8],
           num_heads=4)          # the capture config of tests/test_gpu_train.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build(cfg, seed, dev, precision="parity"):
    from stedm_amd.unet import UNetModel
    m = UNetModel(precision=precision, **cfg).eval()
    prng.fill_module_(m, seed=seed)
    return m.to(dev)


def _inputs(tag, cfg, B, hw, seed, dev):
    x = prng.normal(seed, f"unet.{tag}.x", (B, cfg["in_channels"], hw, hw)).to(dev)
    ctx = prng.normal(seed, f"unet.{tag}.ctx", (B, cfg["model_channels"] * 4)).to(dev)
    target = prng.normal(seed, f"unet.{tag}.target", (B, cfg["out_channels"], hw, hw)).to(dev)
    return x, ctx, target


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


# ---------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("n", [1, 3, 255, 256, 4097, 2 ** 20 + 5])
def test_grad_norm_kernel_vs_float64(dev, n):
    """stedm_grad_norm from a 16-byte aligned start and from one float past it, grad_scale 1 and 0.25: the norm within 2^-22 (2 fp32 ulp) of the
    float64 reference (the sum is exact to double rounding; the one fp32 rounding is the result's), equal bits from two calls, the coefficient
    exactly 1.0f under max_norm and fp32(max_norm / (norm + 1e-6)) of the kernel's own fp32 norm above it."""
    from stedm_amd import ops
    host = prng.normal(11, f"gnorm.{n}", (n,)) * 0.37
    buf = torch.zeros((n + 8,), dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    for off in (0, 1):
        g = buf[off:off + n]
        g.copy_(host)
        assert g.data_ptr() % 16 == 4 * off
        for gs in (1.0, 0.25):
            ref = refs_clip.total_norm64([host], gs)
            for max_norm in (0.0, 4.0 * ref, 0.5 * ref):
                out = ops.grad_norm(g, gs, max_norm).clone()
                again = ops.grad_norm(g, gs, max_norm)
                assert _bits(out) == _bits(again)
                norm, coef, flag = (np.float32(v) for v in out.cpu().numpy())
                rel = abs(float(norm) - ref) / ref
                assert rel <= refs_clip.REL_NORM, (n, off, gs, rel)
                assert flag == 0.0
                if max_norm <= 0 or float(norm) < max_norm:
                    assert coef == np.float32(1.0)
                else:
                    assert coef == np.float32(max_norm) / (norm + np.float32(1e-6)) and coef < 1.0
                assert coef == refs_clip.clip_coef32(norm, max_norm)
        buf.zero_()


def test_grad_norm_kernel_non_finite(dev):
    """one inf element: inf norm, coefficient 0, flag 1; one NaN: NaN norm and coefficient (as clip_grad_norm_ with error_if_nonfinite=False);
    with max_norm <= 0 the coefficient stays 1"""
    from stedm_amd import ops
    host = prng.normal(12, "gnorm.nf", (4097,))
    g = host.to(dev)
    g[4096] = float("inf")
    norm, coef, flag = ops.grad_norm(g, 1.0, 2.0).cpu().tolist()
    assert math.isinf(norm) and norm > 0 and coef == 0.0 and flag == 1.0
    g[4096] = 0.5
    g[77] = float("nan")
    norm, coef, flag = ops.grad_norm(g, 1.0, 2.0).cpu().tolist()
    assert math.isnan(norm) and math.isnan(coef) and flag == 1.0
    norm, coef, flag = ops.grad_norm(g, 1.0, 0.0).cpu().tolist()
    assert math.isnan(norm) and coef == 1.0 and flag == 1.0
    # a finite fp64 sum whose scaled root overflows fp32: the norm is inf and the coefficient 0 as above, and the flag says so too
    big = torch.full((3,), 1e30, dtype=torch.float32, device=dev)
    norm, coef, flag = ops.grad_norm(big, 1e10, 2.0).cpu().tolist()
    assert math.isinf(norm) and coef == 0.0 and flag == 1.0
    norm, coef, flag = ops.grad_norm(big, 1.0, 2.0).cpu().tolist()
    assert abs(norm - math.sqrt(3.0) * 1e30) <= 1e24 and flag == 0.0 and 0.0 < coef < 1e-29


# ---------------------------------------------------------------------------------------------------- the trainer's arena
def test_arena_padding_does_not_enter_the_norm(dev):
    """the kernel walks the whole arena, alignment padding included: with every p.grad filled, the norm is that of the parameters' gradients
    alone (two extra parameters of 5 and 3 elements force padding), and max_grad_norm = 0 reports it without clipping"""
    from stedm_amd.train import UNetTrainer
    m = build(TINY, 6, dev)
    extra = [torch.nn.Parameter(torch.zeros(5, device=dev)), torch.nn.Parameter(torch.zeros(3, device=dev))]
    tr = UNetTrainer(m, lr=1e-3, extra_params=extra, max_grad_norm=0)
    m._prepare()
    tr._alloc_grads()
    params = list(tr._arena_params)
    host = [prng.normal(4, f"pad.g{i}", tuple(p.shape)) for i, p in enumerate(params)]
    for p, g in zip(params, host):
        p.grad.copy_(g)
    assert tr.grad_arena.numel() > sum(p.numel() for p in params), "no padding in this arena: the test checks nothing"
    before = [p.detach().clone() for p in params]
    tr._grads_ready = True
    tr.optimizer_step()
    ref = refs_clip.total_norm64(host)
    assert tr.last_grad_norm.dim() == 0 and abs(float(tr.last_grad_norm) - ref) / ref <= refs_clip.REL_NORM
    assert float(tr._gnorm[1][1]) == 1.0 and any(not torch.equal(a, p.detach()) for a, p in zip(before, params))


@pytest.mark.parametrize("fuse_packs", [True, False])
def test_a_coefficient_of_one_is_the_unclipped_step_bitwise(dev, fuse_packs):
    """max_grad_norm far above the norm (the *_clip entry points with a device coefficient of exactly 1.0f) against no clipping (the plain entry
    points): parameters, moments, EMA shadows and weight packs bit for bit after each of three steps. overlap_optimizer is pinned off on both
    sides (clipping never takes that route), so the two runs differ in the entry points alone."""
    from stedm_amd.train import UNetTrainer
    runs = []
    for mx in (1e9, None):
        m = build(TINY, 6, dev, "bf16")
        tr = UNetTrainer(m, lr=1e-3, weight_decay=0.01, max_grad_norm=mx)
        tr.fuse_packs = fuse_packs
        tr.overlap_optimizer = False
        snaps = []
        for step in range(3):
            x, ctx, target = _inputs(f"one{step}", TINY, 2, 16, 6 + step, dev)
            t = torch.tensor([951 - step, 21 + step], device=dev)
            tr.train_step(x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
            m._prepare()
            packs = [it[8].clone() for pl in (m._plan, tr._dplan) for it in pl.items]
            snaps.append([p.detach().clone() for p in m.parameters()] + [e.clone() for e in tr.ema_parameters()] +
                         [v.clone() for v in tr._opt["m"]] + [v.clone() for v in tr._opt["v"]] + packs)
        if mx is not None:
            assert float(tr._gnorm[1][1]) == 1.0 and 0 < float(tr.last_grad_norm) < mx
        else:
            assert tr.last_grad_norm is None
        runs.append(snaps)
    for step, (sa, sb) in enumerate(zip(*runs)):
        assert len(sa) == len(sb)
        for i, (a, b) in enumerate(zip(sa, sb)):
            assert torch.equal(a, b), (step, i)


def test_clipped_adamw_steps_vs_torch_clip_and_oracle(dev):
    """Three optimizer steps on gradients prng.normal * {0.01, 1.0, 0.1} with a max_norm that clips steps 2 and 3 and not step 1, against
    clip_grad_norm_ on CPU copies + the oracle's AdamW / EMA (tests/refs_clip.py), at the tolerances test_adamw_ema_step_vs_oracle holds the
    unclipped kernel to (rtol 2e-6, atol 2e-7): the clip is one more fp32 multiply per element and AdamW's m / sqrt(v) is homogeneous of degree 0
    in a common gradient scale. The fp32 reference itself stays inside these tolerances of a float64 one
    (tests/test_clip_lr_cpu.py::test_fp32_clipped_adamw_reference_stays_within_the_kernel_tolerances_of_float64: worst 0.15 of the bound)."""
    from stedm_amd.train import UNetTrainer
    m = build(TINY, 6, dev)
    params = list(m.parameters())
    shapes = [tuple(p.shape) for p in params]
    mx = refs_clip.clip_steps_max_norm(shapes)
    tr = UNetTrainer(m, lr=1e-3, weight_decay=0.01, ema_decay=0.9999, max_grad_norm=mx)
    m._prepare()
    tr._alloc_grads()
    ref_p, ref_e, ref_norms = refs_clip.tiny_unet_clip_reference("float32")
    coefs = []
    for step in (1, 2, 3):
        grads = refs_clip.clip_step_grads(shapes, step)
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        tr._grads_ready = True
        tr.optimizer_step()
        ref = refs_clip.total_norm64(grads)
        assert abs(float(tr.last_grad_norm) - ref) / ref <= refs_clip.REL_NORM
        assert abs(float(tr.last_grad_norm) - ref_norms[step - 1]) <= 1e-5 * ref
        coefs.append(float(tr._gnorm[1][1]))
    assert coefs[0] == 1.0 and coefs[1] < 0.1 and coefs[1] < coefs[2] < 1.0, coefs
    for i, p in enumerate(params):
        assert torch.allclose(p.detach().cpu(), ref_p[i], rtol=2e-6, atol=2e-7), i
    ema = {id(p): e for p, e in zip(tr._opt["params"], tr.ema_parameters())}
    for i, p in enumerate(params):
        assert torch.allclose(ema[id(p)].cpu(), ref_e[i], rtol=2e-6, atol=2e-7), i
    ref_m, ref_v = refs_clip.tiny_unet_clip_moments("float32")          # the moments, at the same tolerances
    mom = {id(p): mv for p, mv in zip(tr._opt["params"], zip(tr._opt["m"], tr._opt["v"]))}
    for i, p in enumerate(params):
        assert torch.allclose(mom[id(p)][0].cpu(), ref_m[i], rtol=2e-6, atol=2e-7), i
        assert torch.allclose(mom[id(p)][1].cpu(), ref_v[i], rtol=2e-6, atol=2e-7), i


def test_norm_under_gradient_accumulation_is_that_of_the_mean_gradient(dev):
    """accumulate_grad_batches = 2: the norm runs after the window has been folded back into the arena, so last_grad_norm is the norm of the mean of
    the two micro-batch gradients. Reference: float64 over the two arenas captured after each backward. Bound: the kernel's 2^-22 plus 2^-24 for
    the one fp32 rounding per element of the running mean (0.5 a + 0.5 b: the halvings are exact, the sum rounds once)."""
    from stedm_amd.train import UNetTrainer
    m = build(TINY, 6, dev)
    tr = UNetTrainer(m, lr=1e-3, weight_decay=0.0, accumulate_grad_batches=2, max_grad_norm=0.05)
    x, ctx, target = _inputs("tiny", TINY, 2, 16, 6, dev)
    t = torch.tensor([951, 21], device=dev)
    arenas = []
    for i in range(2):
        sl = slice(i, i + 1)
        tr.train_step(x[sl, :4].contiguous(), x[sl, 4:].contiguous(), t[sl], ctx[sl].contiguous(), target[sl].contiguous(),
                      after_backward=lambda dx, dctx: arenas.append(tr.grad_arena.double().cpu()))
        assert (tr.last_grad_norm is None) == (i == 0)           # the first micro-batch does not step the optimizer
    assert tr.step_count == 1 and len(arenas) == 2 and not torch.equal(arenas[0], arenas[1])
    ref = float(((arenas[0] + arenas[1]) / 2).norm())
    rel = abs(float(tr.last_grad_norm) - ref) / ref
    print(f"accumulated norm {float(tr.last_grad_norm):.6e}, float64 reference {ref:.6e}, rel {rel:.2e}")
    assert rel <= 2.0 ** -22 + 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- captured step
CAP_MAX_NORM = 1.2           # inside the range of the thirteen steps' norms (about 2.1 falling to 0.5; printed by the test): the early steps clip


def _cap_run(dev, graphed, lam, count_windows=False):
    from stedm_amd.train import UNetTrainer
    m = build(CAP, 6, dev, "bf16")
    tr = UNetTrainer(m, lr=2e-4, weight_decay=0.01, max_grad_norm=CAP_MAX_NORM, lr_lambda=lam)
    tr.opt_bucket_mb = 1
    tr.GRAPH_WINDOW = 3
    windows = [0]
    orig = tr._graph_window

    def counted(g):
        windows[0] += 1
        return orig(g)

    tr._graph_window = counted
    losses, norms, lrs, replays = [], [], [], 0
    for step in range(13):
        x, ctx, target = _inputs(f"cap{step}", CAP, 2, 16, 6 + step, dev)
        t = torch.tensor([951 - 7 * step, 21 + step], device=dev) if step < 9 else torch.tensor([5 + step, 700], device=dev)
        if step == 5:
            tr.lr = 1e-4
        a = (x[:, :4].contiguous(), x[:, 4:].contiguous(), t, ctx, target)
        lrs.append(tr.current_lr())
        if graphed and step != 6:
            losses.append(float(tr.train_step_graphed(*a)))
            replays += int(getattr(tr, "_graph", None) is not None)
        else:
            losses.append(float(tr.train_step(*a)))      # step 6 of the graphed run: eager, behind the graph's back
        norms.append(float(tr.last_grad_norm))
    torch.cuda.synchronize()
    assert tr.step_count == 13
    if count_windows:
        return windows[0], replays
    m._prepare()
    packs = [it[8].clone() for pl in (m._plan, tr._dplan) for it in pl.items]
    state = ([p.detach().clone() for p in m.parameters()], [e.clone() for e in tr.ema_parameters()],
             [v.clone() for v in tr._opt["m"]] + [v.clone() for v in tr._opt["v"]], packs)
    return losses, norms, lrs, state, windows[0], replays


def test_captured_clipped_scheduled_step_equals_the_eager_step_bitwise(dev):
    """The protocol of test_captured_train_step_equals_the_eager_step_bitwise (bf16, GRAPH_WINDOW = 3: three eager steps, replays, a base-rate change
    at step 5, an eager step behind the graph's back at step 6, re-capture) with max_grad_norm set so that some steps clip and a
    LambdaLinearScheduler with a 4-step warm-up: the norm launches and the coefficient pointer are part of the capture, the learning rate of every
    replayed step comes from the device schedule's rows. Losses, last_grad_norm, parameters, EMA shadows, moments and packs bit for bit; the
    schedule is re-filled as often as under a constant rate (never because the schedule moved)."""
    from stedm_amd.lr_scheduler import LambdaLinearScheduler
    mk = lambda: LambdaLinearScheduler(warm_up_steps=[4], f_min=[0.2], f_max=[1.0], f_start=[0.05], cycle_lengths=[40]).schedule
    la, na, ra, sa, wa, reps = _cap_run(dev, True, mk())
    lb, nb, rb, sb, wb, _ = _cap_run(dev, False, mk())
    print("losses", ["%.5f" % v for v in la])
    print("norms", ["%.4f" % v for v in na], "max_grad_norm", CAP_MAX_NORM)
    print("lr", ["%.3e" % v for v in ra], "schedule refills", wa, "replays", reps)
    assert reps == 6          # steps 3-5 and 10-12
    replayed = na[3:6] + na[10:]
    assert any(v > CAP_MAX_NORM for v in replayed) and any(v < CAP_MAX_NORM for v in replayed), "replayed steps must both clip and not clip"
    f = mk()
    assert ra == rb == [(2e-4 if s < 5 else 1e-4) * f(s) for s in range(13)] and len(set(ra)) == 13
    assert la == lb, (la, lb)
    assert na == nb, (na, nb)
    for name, xa, xb in zip(("parameter", "ema", "moment", "pack"), sa, sb):
        assert len(xa) == len(xb)
        for i, (a, b) in enumerate(zip(xa, xb)):
            assert torch.equal(a, b), f"{name} {i}"
    wc, repc = _cap_run(dev, True, None, count_windows=True)
    assert wb == 0 and repc == reps and wa == wc < reps, (wa, wc, reps)


def test_captured_step_runs_a_finite_schedule_to_its_last_step(dev):
    """A LambdaLinearScheduler of ONE 8-step cycle under the default GRAPH_WINDOW (4096 rows, far past the cycle's end): the window ends at the
    schedule's last step, the graphed run takes all nine steps the schedule defines (n = 0 .. 8) with the eager run's bits, and the tenth call
    raises the scheduler's own error on both routes."""
    from stedm_amd.lr_scheduler import LambdaLinearScheduler
    from stedm_amd.train import UNetTrainer
    runs = []
    for graphed in (True, False):
        m = build(TINY, 6, dev, "bf16")
        lam = LambdaLinearScheduler(warm_up_steps=[3], f_min=[0.1], f_max=[1.0], f_start=[0.01], cycle_lengths=[8]).schedule
        tr = UNetTrainer(m, lr=2e-4, weight_decay=0.01, lr_lambda=lam)
        assert tr.GRAPH_WINDOW == 4096
        step = tr.train_step_graphed if graphed else tr.train_step
        losses = []
        for s in range(10):
            x, ctx, target = _inputs(f"fin{s}", TINY, 2, 16, 6 + s, dev)
            a = (x[:, :4].contiguous(), x[:, 4:].contiguous(), torch.tensor([951 - s, 21 + s], device=dev), ctx, target)
            if s < 9:
                losses.append(float(step(*a)))
            else:
                with pytest.raises(ValueError, match="past the last cycle"):
                    step(*a)
        if graphed:
            assert tr._graph is not None and tr._graph["valid"] == 7 and tr._graph["base"] == 3          # rows of steps 3 .. 9
        runs.append((losses, [p.detach().clone() for p in m.parameters()], [e.clone() for e in tr.ema_parameters()]))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)


def test_changing_max_grad_norm_drops_the_captured_step(dev):
    """max_norm is a baked argument of the captured norm launch: another value, or clipping switched off, is a stale key like any other"""
    from stedm_amd.train import UNetTrainer
    m = build(TINY, 6, dev, "bf16")
    tr = UNetTrainer(m, lr=2e-4, max_grad_norm=1.0)
    x, ctx, target = _inputs("tiny", TINY, 2, 16, 6, dev)
    a = (x[:, :4].contiguous(), x[:, 4:].contiguous(), torch.tensor([951, 21], device=dev), ctx, target)
    for _ in range(tr.GRAPH_WARMUP + 1):
        tr.train_step_graphed(*a)
    assert tr._graph is not None and math.isfinite(float(tr.last_grad_norm))
    tr.max_grad_norm = 0.5
    tr.train_step_graphed(*a)
    assert tr._graph is None
    for _ in range(tr.GRAPH_WARMUP):
        tr.train_step_graphed(*a)
    assert tr._graph is not None
    tr.max_grad_norm = None
    tr.train_step_graphed(*a)
    assert tr._graph is None and tr.step_count == 2 * tr.GRAPH_WARMUP + 3


# ---------------------------------------------------------------------------------------------------- two ranks
def _clip_ddp_worker(rank, world, port, q, max_norm):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from stedm_amd.train import UNetTrainer
    dev = torch.device("cuda:0")
    m = build(TINY, 6, dev)
    tr = UNetTrainer(m, lr=1e-3, weight_decay=0.0, max_grad_norm=max_norm)
    x, ctx, target = _inputs("tiny", TINY, world, 16, 6, dev)
    t = torch.tensor([951, 21], device=dev)
    sl = slice(rank, rank + 1)
    tr.train_step(x[sl, :4].contiguous(), x[sl, 4:].contiguous(), t[sl], ctx[sl].contiguous(), target[sl].contiguous())
    out = {"__rank__": np.array([rank]), "__norm_bits__": np.array(_bits(tr.last_grad_norm.reshape(1))), "__coef__": np.array([float(tr._gnorm[1][1])]),
           "__fires__": np.array([tr.overlap_fires])}
    if rank == 0:
        out.update({n: p.detach().cpu().numpy() for n, p in m.named_parameters()})       # numpy: no shared-memory handles across the exit
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_clipped_step_equals_gradient_accumulation(dev):
    """Two ranks, one sample each (the pattern of test_two_rank_data_parallel_step_equals_gradient_accumulation): each rank takes the norm of the
    same all-reduced arena with the 1/world scale, so both report the same bits and no collective is added; the parameters after one clipped
    step equal those of one rank accumulating the two samples with the same max_grad_norm (that test's criterion: max |dw| < 2e-5 at lr 1e-3)."""
    import os
    import torch.multiprocessing as mp
    from stedm_amd.train import UNetTrainer
    x, ctx, target = _inputs("tiny", TINY, 2, 16, 6, dev)
    t = torch.tensor([951, 21], device=dev)

    def accumulate(max_norm):
        m = build(TINY, 6, dev)
        tr = UNetTrainer(m, lr=1e-3, weight_decay=0.0, accumulate_grad_batches=2, max_grad_norm=max_norm)
        for i in range(2):
            sl = slice(i, i + 1)
            tr.train_step(x[sl, :4].contiguous(), x[sl, 4:].contiguous(), t[sl], ctx[sl].contiguous(), target[sl].contiguous())
        return m, tr

    _, tr0 = accumulate(0)                                 # report only: the norm of the mean gradient
    max_norm = float(np.float32(0.5 * float(tr0.last_grad_norm)))
    m, tr = accumulate(max_norm)
    assert float(tr._gnorm[1][1]) < 0.6
    ref = {n: p.detach().cpu() for n, p in m.named_parameters()}
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctxm.Process(target=_clip_ddp_worker, args=(r, 2, port, q, max_norm)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    got.sort(key=lambda d: int(d["__rank__"][0]))
    assert got[0]["__norm_bits__"].tolist() == got[1]["__norm_bits__"].tolist()
    assert float(got[0]["__coef__"][0]) == float(got[1]["__coef__"][0]) < 0.6
    assert int(got[0]["__fires__"][0]) > 0, "the overlapped all-reduce (the default) did not run"
    norm = np.array(got[0]["__norm_bits__"], dtype=np.int32).view(np.float32)[0]
    assert abs(float(norm) - float(tr.last_grad_norm)) <= 1e-5 * float(norm)
    worst = max(float(np.abs(got[0][n] - ref[n].numpy()).max()) for n in ref)
    print(f"two-rank clipped step vs gradient accumulation: max |dw| = {worst:.2e} (lr 1e-3), norm {float(norm):.5f}, max_norm {max_norm:.5f}")
    assert worst < 2e-5


# ---------------------------------------------------------------------------------------------------- surface
def test_latent_diffusion_surface_with_clipping_and_a_scheduler(dev):
    """LatentDiffusion(scheduler_config=...).configure_trainer(gradient_clip_val=...): two training_step_hip calls; current_lr() follows the
    schedule, last_grad_norm is a finite 0-d device tensor, and optimizer_state_dict() round-trips the base rate through initial_lr"""
    from stedm_amd.latent_diffusion import LatentDiffusion
    from stedm_amd.lr_scheduler import LambdaLinearScheduler
    sc = {"target": "ldm.lr_scheduler.LambdaLinearScheduler",
          "params": {"warm_up_steps": [4], "f_min": [0.1], "f_max": [1.0], "f_start": [1e-6], "cycle_lengths": [1000]}}
    f = LambdaLinearScheduler(**sc["params"]).schedule

    def make():
        ld = LatentDiffusion(build(TINY, 6, dev), linear_start=0.0015, linear_end=0.0205, loss_type="l1", image_size=16, channels=4,
                             conditioning_key="hybrid", scheduler_config=sc).to(dev)
        return ld, ld.configure_trainer(lr=2e-4, gradient_clip_val=0.05)

    ld, tr = make()
    ld.train()
    assert ld.use_scheduler and ld.last_grad_norm is None and ld.current_lr() == 2e-4 * f(0)
    p0 = [p.detach().clone() for p in ld.model.diffusion_model.parameters()]
    for step in range(2):
        x0 = prng.normal(21 + step, "ld.x0", (2, 4, 16, 16)).to(dev)
        noise = prng.normal(21 + step, "ld.noise", (2, 4, 16, 16)).to(dev)
        cond = {"c_concat": [prng.uniform(21 + step, "ld.cc", (2, 3, 16, 16)).to(dev)], "c_crossattn": [prng.normal(21 + step, "ld.ctx", (2, 128)).to(dev)]}
        loss = ld.training_step_hip(x0, cond, torch.tensor([951, 21], device=dev), noise)
        assert math.isfinite(float(loss))
        n = ld.last_grad_norm
        assert n.is_cuda and n.dim() == 0 and math.isfinite(float(n)) and float(n) > 0
        assert tr.step_count == step + 1 and ld.current_lr() == 2e-4 * f(step + 1) and tr.lr == 2e-4
    assert any(not torch.equal(a, p.detach()) for a, p in zip(p0, ld.model.diffusion_model.parameters()))
    sd = tr.optimizer_state_dict()
    g = sd["param_groups"][0]
    assert g["initial_lr"] == 2e-4 and g["lr"] == 2e-4 * f(2)
    ld2, tr2 = make()
    tr2.lr = 1.0
    tr2.load_optimizer_state_dict(sd)
    g2 = tr2.optimizer_state_dict()["param_groups"][0]
    assert tr2.lr == 2e-4 and tr2.step_count == 2 and tr2.current_lr() == ld2.current_lr() == 2e-4 * f(2) and g2["lr"] == g["lr"] and g2["initial_lr"] == 2e-4
    for a, b in zip(tr._opt["m"] + tr._opt["v"], tr2._opt["m"] + tr2._opt["v"]):
        assert torch.equal(a, b)
