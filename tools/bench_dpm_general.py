#!/usr/bin/env python3
"""The general DPM-Solver on the graphed sampling loop (NS32 32x32 latents, CFG 1.5, 20 model evaluations (NFE), one captured NFE replayed
per row), variants alternating round for round in one process:
  * 2m:        DPM-Solver++(2M) as shipped (the default keywords: dpm_tables, stedm_dpm_step, DPMStepGraph);
  * 2m_plan:   the same keywords through the plan path (dpm_plan, stedm_dpm_update, DPMPlanGraph): the rows of 2m, bit for bit;
  * 3m:        order=3 (multistep, stedm_dpm_update);
  * ss3:       method="singlestep", order=3;
  * 2m_thr:    order=2 with thresholding (stedm_dpm_update split around stedm_dpm_threshold);
  * ss2_noise: method="singlestep", order=2, predict_x0=False.
Per batch: whole-loop ms and ms per NFE (median of the rounds, with min / max). Then the two kernels alone (CUDA-event timing of
back-to-back launches, median of rounds): stedm_dpm_update (a multistep third-order row, CFG) and stedm_dpm_threshold at the bench shape
(B x 4 x 32 x 32) and at 4 x 128 x 128 for B = 1 / 16 / 64.
    python tools/bench_dpm_general.py [--batches 64,8] [--rounds 6] [--steps 20] [--precision f16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

VARIANTS = {"2m": {}, "2m_plan": {}, "3m": dict(order=3), "ss3": dict(method="singlestep", order=3), "2m_thr": dict(thresholding=True),
            "ss2_noise": dict(method="singlestep", order=2, predict_x0=False)}


def build(ld, dev, B, steps, name):
    """-> (graph object, img, reset fn, NFE count) for one variant, captured and warm"""
    from stedm_amd.dpm_solver import DPMPlanGraph, DPMSolverSampler, DPMStepGraph, dpm_plan
    xT, cond, unc = bench.synth_inputs(dev, B, 0)
    smp = DPMSolverSampler(ld, device=dev, use_graph=True)
    img = xT.clone()
    if name == "2m":
        smp.make_schedule(steps)
        g = DPMStepGraph(smp, img, cond, unc, 1.5)
        g.reset(0)
        g.step_eager()
        R = steps

        def reset():
            g.reset(0)
            img.copy_(xT)
    else:
        plan = dpm_plan(smp.alphas_cumprod, steps, **VARIANTS[name])
        smp.plan, smp._rows, smp._t_table = plan, plan.rows.to(dev), plan.t_input.to(dev)
        g = DPMPlanGraph(smp, img, cond, unc, 1.5)
        g.nfe()
        R = int(plan.rows.shape[0])

        def reset():
            g.reset(0)
            img.copy_(xT)
            if g.base is not img:
                g.base.copy_(xT)
    with g.stream_ctx():
        g.capture()
    g.join()
    return g, reset, R


def time_loop(g, reset, R):
    with g.stream_ctx():
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(R):
            g.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    g.join()
    return dt


def kernel_us(fn, reps=200, rounds=5):
    """median over rounds of the mean per-launch time of `reps` back-to-back launches (after a warm-up round), in microseconds"""
    for _ in range(20):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return round(statistics.median(out), 2)


def kernels(dev):
    from oracle import ddim as od
    from stedm_amd import ops
    from stedm_amd.dpm_solver import dpm_plan
    plan = dpm_plan(od.Schedule().alphas_cumprod, 20, order=3)
    rows = plan.rows.to(dev)
    step = torch.tensor([5], dtype=torch.int32, device=dev)           # a multistep third-order row
    res = {}
    for B, C, H in ((64, 4, 32), (8, 4, 32), (1, 4, 128), (16, 4, 128), (64, 4, 128)):
        shp = (B, C, H, H)
        x, base = torch.randn(shp, device=dev), torch.randn(shp, device=dev)
        ec, eu = torch.randn(shp, device=dev), torch.randn(shp, device=dev)
        slots = torch.randn((3,) + shp, device=dev)
        xs = torch.randn(shp, device=dev)
        upd = kernel_us(lambda: ops.dpm_update(x, base, ec, eu, slots, rows, step_idx=step, cfg_scale=1.5))
        thr = kernel_us(lambda: ops.dpm_threshold(xs, 1.0), reps=50)
        res[f"{B}x{C}x{H}x{H}"] = {"dpm_update_us": upd, "dpm_threshold_us": thr, "elements_per_sample": C * H * H}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None, help="also write the result JSON to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpm_general: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision)
    res = {"precision": ld.model.diffusion_model.precision.label,
           "workload": f"NS32 32x32 + CFG 1.5, hipGraph replay, {args.steps} NFE per loop", "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        built = {n: build(ld, dev, B, args.steps, n) for n in VARIANTS}
        for n, (g, reset, R) in built.items():
            time_loop(g, reset, R)                       # warm-up loop
        times = {n: [] for n in VARIANTS}
        for _ in range(args.rounds):
            for n, (g, reset, R) in built.items():
                times[n].append(time_loop(g, reset, R))
        row = {}
        for n, (g, reset, R) in built.items():
            med = statistics.median(times[n]) * 1e3
            row[n] = {"nfe": R, "loop_ms": round(med, 2), "ms_per_nfe": round(med / R, 3), "loop_ms_min": round(min(times[n]) * 1e3, 2),
                      "loop_ms_max": round(max(times[n]) * 1e3, 2)}
        base = row["2m"]["ms_per_nfe"]
        for n in row:
            row[n]["vs_2m_per_nfe"] = round(row[n]["ms_per_nfe"] / base, 4)
        res["batches"][str(B)] = row
        print(json.dumps({str(B): row}), flush=True)
        del built
        torch.cuda.empty_cache()
    res["kernels"] = kernels(dev)
    print(json.dumps({"kernels": res["kernels"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
