#!/usr/bin/env python3
"""Ancestral DDPM sampling against DDIM on the graphed loop (NS32 32x32 latents, unguided: one U-Net pass per iteration), in one process:
  * per iteration: the DDPM step graph (stedm_amd/ancestral.py: t from the counter, U-Net, stedm_ddpm_step, counter - 1) replayed
    --iters times from t = 999, plain and masked (left half kept, both draws in the kernel), against DDIM-S's StepGraph replayed for its S
    iterations (unguided, eta 0); the loops alternate run for run, medians of --rounds;
  * the DDPM-1000 wall time through the public call (LatentDiffusion.sample, use_graph: one eager step, one capture, 999 replays);
  * stedm_ddpm_step alone at the headline shape [B, 4, 32, 32] and at [16, 3, 128, 128], plain and masked: a hipGraph of 200 launches
    replayed, microseconds per launch and GB/s of the bytes it must move (x + eps [+ x0 + mask] read, x written);
  * the graphed progressive_denoising iteration (the same step graph on stedm_ddpm_step_ex: a temperature table indexed by t, noise_dropout
    0.2, the predicted x0 written out), without and with quantize_denoised against a synthetic 8192 x 4 codebook, in the same alternation;
  * stedm_ddpm_step_ex alone beside stedm_ddpm_step at the same shapes: with the temperature table, dropout 0.2 and x0_out (x + eps read,
    x + x0 written), and with the codebook on top (two launches: x + eps read and x0 written by the quantiser, x + x0 read and x written
    by the update); and a torch device copy of the plain step's byte count in the same graphed form, the rate to hold them against.
    python tools/bench_ddpm.py [--batches 64,8] [--rounds 6] [--iters 50] [--precision f16] [--no-wall]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


class _DDIMLoop:
    def __init__(self, ld, img, cond, steps):
        from stedm_amd.ddim import DDIMSampler, StepGraph
        smp = DDIMSampler(ld, use_graph=True)
        smp.make_schedule(steps, ddim_eta=0.0, verbose=False)
        self.n = int(smp.ddim_timesteps.shape[0])
        self.img = img
        self.g = StepGraph(smp, img, cond, None, 1.0)
        self.g.reset(self.n - 1)
        self.g.step_eager()
        with self.g.stream_ctx():
            self.g.capture()
        self.g.join()

    def run(self):
        self.g.reset(self.n - 1)
        for _ in range(self.n):
            self.g.replay()


class _DDPMLoop:
    def __init__(self, ld, img, cond, iters, masking=None, opts=None):
        from stedm_amd.ancestral import AncestralStepGraph, step_table
        self.n = iters
        self.img = img
        self.g = AncestralStepGraph(ld, img, cond, step_table(ld), True, 1234, 0, masking, opts=opts)
        self.g.step_idx.fill_(ld.num_timesteps - 1)
        self.g.step()
        with self.g.stream_ctx():
            self.g.capture()
        self.g.join()
        self.t0 = ld.num_timesteps - 1

    def run(self):
        self.g.step_idx.fill_(self.t0)
        for _ in range(self.n):
            self.g.replay()


def time_run(lp, xT):
    with lp.g.stream_ctx():
        lp.img.copy_(xT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    lp.g.join()
    return dt


def _ex_opts(dev, quant):
    """progressive_denoising's options for the timed legs: a temperature ramp over the schedule, dropout 0.2, a synthetic codebook"""
    from stedm_amd.ancestral import _ExOpts
    g = torch.Generator(device=dev).manual_seed(9)
    cb = torch.randn((8192, 4), device=dev, generator=g) * 0.8 if quant else None
    return _ExOpts(torch.linspace(0.5, 1.0, 1000, device=dev), 0.2, cb)


def kernel_us(dev, shape, masked, launches=200, reps=5, ex=None):
    """stedm_ddpm_step alone (ex: stedm_ddpm_step_ex with "opts" = temperature table + dropout 0.2 + x0_out, or "quant" = the same with an
    8192-entry codebook): microseconds per launch (a graph of `launches` launches, median of `reps` replays) and the bytes moved."""
    from oracle import ddim as od
    from stedm_amd import ops
    from stedm_amd.schedule import PosteriorSchedule, ddpm_step_table
    ps = PosteriorSchedule.make(1000, 0.0015, 0.0205)
    tab = torch.from_numpy(ddpm_step_table(ps.sqrt_recip_alphas_cumprod, ps.sqrt_recipm1_alphas_cumprod, ps.posterior_mean_coef1,
                                           ps.posterior_mean_coef2, ps.posterior_log_variance_clipped)).to(dev)
    s = od.Schedule()
    sa, s1 = s.sqrt_alphas_cumprod.to(dev), s.sqrt_one_minus_alphas_cumprod.to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(shape, device=dev, generator=g)
    e = torch.randn(shape, device=dev, generator=g)
    x0 = torch.randn(shape, device=dev, generator=g)
    mask = (torch.rand((shape[0], 1) + tuple(shape[2:]), device=dev, generator=g) > 0.5).float()
    step = torch.tensor([500], dtype=torch.int32, device=dev)
    kw = dict(mask=mask, x0=x0, mask_seed=7, sqrt_ac=sa, sqrt_1mac=s1) if masked else {}
    one = lambda: ops.ddpm_step(x, e, tab, step, True, seed=3, **kw)
    if ex == "copy":                 # a device copy moving what the plain step moves (half read, half written), in the same graphed form
        src, dst = torch.empty(3 * x.numel() // 2, device=dev), torch.empty(3 * x.numel() // 2, device=dev)
        src.normal_()
        one = lambda: dst.copy_(src)
    elif ex is not None:
        o = _ex_opts(dev, ex == "quant")
        cb = None if o.codebook is None else (o.codebook if shape[1] == 4 else o.codebook[:, :shape[1]].contiguous())
        x0o = torch.empty_like(x)
        one = lambda: ops.ddpm_step_ex(x, e, tab, step_idx=step, temperature=o.temperature, noise_dropout=o.noise_dropout, codebook=cb,
                                       seed=3, x_out=x, x0_out=x0o, **kw)
    one()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gr = ops.Graph()
        with gr:
            for _ in range(launches):
                one()
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.launch()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / launches)
    torch.cuda.current_stream().wait_stream(side)
    us = sorted(ts[1:])[len(ts[1:]) // 2]
    n = x.numel()
    nbytes = 4 * (3 * n + (n + mask.numel() if masked else 0) + {None: 0, "copy": 0, "opts": n, "quant": 3 * n}[ex])
    assert bool(torch.isfinite(x).all())
    return {"shape": list(shape), "masked": masked, "entry": "device copy" if ex == "copy" else "stedm_ddpm_step" + ("" if ex is None else "_ex:" + ex), "us": round(us, 2), "GB_per_s": round(nbytes / (us * 1e-6) / 1e9, 1), "bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--no-wall", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddpm: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision)
    res = {"precision": ld.model.diffusion_model.precision.label,
           "workload": f"NS32 32x32 unguided, hipGraph replay: DDPM step x{args.iters} (plain, masked) vs DDIM-{args.iters}", "batches": {},
           "kernel": []}
    for B in (int(b) for b in args.batches.split(",")):
        xT, cond, _ = bench.synth_inputs(dev, B, 0)
        mask = torch.zeros(B, 1, 32, 32, device=dev)
        mask[..., :16] = 1.0
        x0 = torch.randn(B, 4, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        masking = {"mask": mask, "x0": x0, "mask_seed": 99, "mask_noises": None}
        ls = {"ddpm": _DDPMLoop(ld, xT.clone(), cond, args.iters), "ddim": _DDIMLoop(ld, xT.clone(), cond, args.iters),
              "ddpm_masked": _DDPMLoop(ld, xT.clone(), cond, args.iters, masking),
              "progressive": _DDPMLoop(ld, xT.clone(), cond, args.iters, opts=_ex_opts(dev, False)),
              "progressive_quant": _DDPMLoop(ld, xT.clone(), cond, args.iters, opts=_ex_opts(dev, True))}
        order = list(ls)
        for name in order:
            time_run(ls[name], xT)
        ts = {k: [] for k in ls}
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                ts[name].append(time_run(ls[name], xT))
        rec = {}
        for k, v in ts.items():
            med = sorted(v)[len(v) // 2] * 1e3
            n = ls[k].n
            rec[k] = {"iterations": n, "ms_per_loop_median": round(med, 3), "ms_min": round(min(v) * 1e3, 3), "ms_max": round(max(v) * 1e3, 3),
                      "ms_per_iteration": round(med / n, 4)}
        rec["iter_ratio_ddpm_over_ddim"] = round(rec["ddpm"]["ms_per_iteration"] / rec["ddim"]["ms_per_iteration"], 4)
        rec["iter_ratio_masked_over_plain"] = round(rec["ddpm_masked"]["ms_per_iteration"] / rec["ddpm"]["ms_per_iteration"], 4)
        rec["iter_ratio_progressive_over_plain"] = round(rec["progressive"]["ms_per_iteration"] / rec["ddpm"]["ms_per_iteration"], 4)
        assert all(bool(torch.isfinite(lp.img).all()) for lp in ls.values()), "non-finite latents"
        del ls
        if not args.no_wall:
            run = lambda: ld.sample(cond, B, x_T=xT, noise_seed=11)
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            rec["ddpm1000_wall_s"] = round(time.perf_counter() - t0, 3)
            assert bool(torch.isfinite(out).all())
        res["batches"][str(B)] = rec
        print(f"[bench_ddpm] B={B}: DDPM {rec['ddpm']['ms_per_iteration']:.3f} ms/iter, masked {rec['ddpm_masked']['ms_per_iteration']:.3f} "
              f"(x{rec['iter_ratio_masked_over_plain']:.4f}), DDIM-{args.iters} {rec['ddim']['ms_per_iteration']:.3f} ms/iter, "
              f"DDPM / DDIM x{rec['iter_ratio_ddpm_over_ddim']:.4f}, progressive {rec['progressive']['ms_per_iteration']:.3f} "
              f"(x{rec['iter_ratio_progressive_over_plain']:.4f}), quantised {rec['progressive_quant']['ms_per_iteration']:.3f} ms/iter"
              + ("" if args.no_wall else f", DDPM-1000 wall {rec['ddpm1000_wall_s']:.2f} s"), flush=True)
    B0 = int(args.batches.split(",")[0])
    for shape in ((B0, 4, 32, 32), (16, 3, 128, 128)):
        for masked in (False, True):
            k = kernel_us(dev, shape, masked)
            res["kernel"].append(k)
            print(f"[bench_ddpm] stedm_ddpm_step {shape} masked={masked}: {k['us']:.2f} us, {k['GB_per_s']:.0f} GB/s", flush=True)
        for ex in ("opts", "quant", "copy"):
            k = kernel_us(dev, shape, False, ex=ex)
            res["kernel"].append(k)
            print(f"[bench_ddpm] {k['entry']} {shape}: {k['us']:.2f} us, {k['GB_per_s']:.0f} GB/s", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
