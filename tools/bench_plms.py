#!/usr/bin/env python3
"""PLMS against DDIM on the graphed sampling loop (NS32 32x32 latents, CFG 1.5, one U-Net CFG pass per evaluation), in one process, the
loops alternating run for run:
  * PLMS-S (default 50 steps = 50 iterations, 51 evaluations; stedm_amd/plms.py: iteration 0 eager, PLMSStepGraph replayed for the rest),
  * PLMS-S masked (mask / x0, left half kept, the blend's noise drawn in the kernel),
  * DDIM-S (the same S; stedm_amd/ddim.py, StepGraph replayed for every iteration).
Per batch: ms per loop and ms per evaluation of each (median of the rounds, with min / max), the loop ratio PLMS / DDIM and masked / plain.
    python tools/bench_plms.py [--batches 64,8] [--rounds 6] [--steps 50] [--precision f16]
The update kernel alone: run this under `rocprofv3 --kernel-trace --stats` (a run of its own) and read plms_step_kernel's row."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


class _DDIMLoop:
    def __init__(self, ld, img, cond, unc, steps):
        from stedm_amd.ddim import DDIMSampler, StepGraph
        smp = DDIMSampler(ld, use_graph=True)
        smp.make_schedule(steps, ddim_eta=0.0, verbose=False)
        self.n = self.evaluations = int(smp.ddim_timesteps.shape[0])
        self.img = img
        self.g = StepGraph(smp, img, cond, unc, 1.5)
        self.g.reset(self.n - 1)
        self.g.step_eager()
        with self.g.stream_ctx():
            self.g.capture()
        self.g.join()

    def run(self):
        g = self.g
        g.reset(self.n - 1)
        for _ in range(self.n):
            g.replay()


class _PLMSLoop:
    def __init__(self, ld, img, cond, unc, steps, blend=None):
        from stedm_amd.plms import PLMSSampler, PLMSStepGraph
        smp = PLMSSampler(ld, use_graph=True)
        smp.make_schedule(steps, ddim_eta=0.0, verbose=False)
        self.n = int(smp.ddim_timesteps.shape[0])
        self.evaluations = self.n + 1
        self.img = img
        self.g = PLMSStepGraph(smp, img, cond, unc, 1.5, blend=blend)
        self.g.reset(self.n - 1)
        self.g.first_step()
        with self.g.stream_ctx():
            self.g.capture()
        self.g.join()

    def run(self):
        g = self.g
        g.reset(self.n - 1)
        g.first_step()
        for _ in range(1, self.n):
            g.replay()


def time_run(lp, xT):
    """one whole sampling loop from x_T -> seconds"""
    with lp.g.stream_ctx():
        lp.img.copy_(xT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    lp.g.join()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plms: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision)
    S = args.steps
    res = {"precision": ld.model.diffusion_model.precision.label,
           "workload": f"NS32 32x32 + CFG 1.5, hipGraph replay: PLMS-{S} (plain, masked) vs DDIM-{S} loop", "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        xT, cond, unc = bench.synth_inputs(dev, B, 0)
        mask = torch.zeros(B, 1, 32, 32, device=dev)
        mask[..., :16] = 1.0
        x0 = torch.randn(B, 4, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        ls = {"plms": _PLMSLoop(ld, xT.clone(), cond, unc, S), "ddim": _DDIMLoop(ld, xT.clone(), cond, unc, S),
              "plms_masked": _PLMSLoop(ld, xT.clone(), cond, unc, S, blend=(mask, x0, 1234, 0))}
        order = list(ls)
        for name in order:                                    # warm-up run of each
            time_run(ls[name], xT)
        ts = {k: [] for k in ls}
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                ts[name].append(time_run(ls[name], xT))
        rec = {}
        for k, v in ts.items():
            med = sorted(v)[len(v) // 2] * 1e3
            n = ls[k].evaluations
            rec[k] = {"evaluations": n, "ms_per_loop_median": round(med, 3), "ms_min": round(min(v) * 1e3, 3), "ms_max": round(max(v) * 1e3, 3),
                      "ms_per_evaluation": round(med / n, 4)}
        rec["loop_ratio_plms_over_ddim"] = round(rec["plms"]["ms_per_loop_median"] / rec["ddim"]["ms_per_loop_median"], 4)
        rec["eval_ratio_plms_over_ddim"] = round(rec["plms"]["ms_per_evaluation"] / rec["ddim"]["ms_per_evaluation"], 4)
        rec["loop_ratio_masked_over_plain"] = round(rec["plms_masked"]["ms_per_loop_median"] / rec["plms"]["ms_per_loop_median"], 4)
        res["batches"][str(B)] = rec
        print(f"[bench_plms] B={B}: PLMS-{S} {rec['plms']['ms_per_loop_median']:.2f} ms ({rec['plms']['ms_per_evaluation']:.3f} ms/eval), "
              f"masked {rec['plms_masked']['ms_per_loop_median']:.2f} ms (x{rec['loop_ratio_masked_over_plain']:.4f}), "
              f"DDIM-{S} {rec['ddim']['ms_per_loop_median']:.2f} ms ({rec['ddim']['ms_per_evaluation']:.3f} ms/eval), "
              f"PLMS / DDIM loop x{rec['loop_ratio_plms_over_ddim']:.4f}, per eval x{rec['eval_ratio_plms_over_ddim']:.4f}", flush=True)
        assert all(bool(torch.isfinite(lp.img).all()) for lp in ls.values()), "non-finite latents"
        del ls
    print(json.dumps(res))


if __name__ == "__main__":
    main()
