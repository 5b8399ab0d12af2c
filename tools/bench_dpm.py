#!/usr/bin/env python3
"""DPM-Solver++(2M) against DDIM on the graphed sampling loop: the whole loop of each, replayed from its captured step (NS32 32x32 latents,
CFG 1.5, one U-Net CFG pass per evaluation), in one process, the two alternating run for run:
  * DPM-Solver-S (default 20 steps = 20 evaluations; stedm_amd/dpm_solver.py, DPMStepGraph),
  * DDIM-128 (the predict config's ddim_steps; the uniform stride makes it 143 iterations; stedm_amd/ddim.py, StepGraph).
Per batch: ms per loop and ms per evaluation of each (median of the rounds, with min / max), and the loop ratio DDIM / DPM.
    python tools/bench_dpm.py [--batches 64,8] [--rounds 6] [--dpm-steps 20] [--ddim-steps 128] [--precision f16]
The update kernel alone: run this under `rocprofv3 --kernel-trace --stats` (a run of its own) and read dpm_step_kernel's row."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def loops(ld, B, dev, dpm_steps, ddim_steps):
    """the two captured steps over the same model and inputs -> {name: (graph, img, reset index, iterations)}, x_T"""
    from stedm_amd.ddim import DDIMSampler, StepGraph
    from stedm_amd.dpm_solver import DPMSolverSampler, DPMStepGraph
    xT, cond, unc = bench.synth_inputs(dev, B, 0)
    out = {}
    smp = DDIMSampler(ld, use_graph=True)
    smp.make_schedule(ddim_steps, ddim_eta=0.0, verbose=False)
    n = smp.ddim_timesteps.shape[0]
    img = xT.clone()
    sg = StepGraph(smp, img, cond, unc, 1.5)
    sg.reset(n - 1)
    sg.step_eager()
    with sg.stream_ctx():
        sg.capture()
    sg.join()
    out["ddim"] = (sg, img, n - 1, n)
    dpm = DPMSolverSampler(ld, device=dev, use_graph=True)
    dpm.make_schedule(dpm_steps)
    img = xT.clone()
    dg = DPMStepGraph(dpm, img, cond, unc, 1.5)
    dg.reset(0)
    dg.step_eager()
    with dg.stream_ctx():
        dg.capture()
    dg.join()
    out["dpm"] = (dg, img, 0, int(dpm_steps))
    return out, xT


def time_run(g, img, index, n, xT):
    """one whole sampling loop from x_T by graph replay -> seconds"""
    with g.stream_ctx():
        g.reset(index)
        img.copy_(xT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            g.replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    g.join()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--ddim-steps", type=int, default=128)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpm: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision)
    res = {"precision": ld.model.diffusion_model.precision.label,
           "workload": f"NS32 32x32 + CFG 1.5, hipGraph replay: DPM-Solver++(2M)-{args.dpm_steps} vs DDIM-{args.ddim_steps} loop", "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        ls, xT = loops(ld, B, dev, args.dpm_steps, args.ddim_steps)
        for name in ls:                                       # warm-up run of each
            time_run(*ls[name], xT)
        ts = {k: [] for k in ls}
        for r in range(args.rounds):
            for name in (("dpm", "ddim") if r % 2 == 0 else ("ddim", "dpm")):
                ts[name].append(time_run(*ls[name], xT))
        rec = {}
        for k, v in ts.items():
            med = sorted(v)[len(v) // 2] * 1e3
            n = ls[k][3]
            rec[k] = {"evaluations": n, "ms_per_loop_median": round(med, 3), "ms_min": round(min(v) * 1e3, 3), "ms_max": round(max(v) * 1e3, 3),
                      "ms_per_evaluation": round(med / n, 4)}
        rec["loop_ratio_ddim_over_dpm"] = round(rec["ddim"]["ms_per_loop_median"] / rec["dpm"]["ms_per_loop_median"], 3)
        res["batches"][str(B)] = rec
        print(f"[bench_dpm] B={B}: DPM-{args.dpm_steps} {rec['dpm']['ms_per_loop_median']:.2f} ms ({rec['dpm']['ms_per_evaluation']:.3f} ms/eval), "
              f"DDIM-{args.ddim_steps} ({rec['ddim']['evaluations']} it) {rec['ddim']['ms_per_loop_median']:.2f} ms "
              f"({rec['ddim']['ms_per_evaluation']:.3f} ms/eval), ratio {rec['loop_ratio_ddim_over_dpm']:.2f}", flush=True)
        assert all(bool(torch.isfinite(img).all()) for _, img, _, _ in ls.values()), "non-finite latents"
        del ls
    print(json.dumps(res))


if __name__ == "__main__":
    main()
