#!/usr/bin/env python3
"""Stochastic DDIM (eta > 0) on the graphed loop against today's eager loop (NS32 32x32 latents, CFG 1.5, DDIM-S), in one process, the
variants alternated run for run, medians of --rounds:
  * graph_eta1        StepGraph replayed S times, eta 1, the step noise drawn in stedm_ddim_step_ex from (noise_seed, sample id);
  * eager_eta1_list   the eager loop fed a pre-drawn list of S noise tensors (what predict_latents_sharded ran before; drawing the list is
                      not timed);
  * graph_eta0        StepGraph, eta 0 (stedm_ddim_step);
  * graph_eta1_quant  graph_eta1 with quantize_x0 against a synthetic 8192 x 4 codebook (stedm_ddim_quantize_x0 after the update).
--kernels: only run the two new kernels (and stedm_ddim_step) at [B, 4, 32, 32] a few hundred times, for a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_ddim_eta.py --kernels` run.
    python tools/bench_ddim_eta.py [--batches 64,8,1] [--rounds 10] [--steps 50] [--precision f16]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


class _FirstStage(torch.nn.Module):
    def __init__(self, dev, n_e=8192, e_dim=4):
        super().__init__()
        self.quantize = torch.nn.Module()
        self.quantize.embedding = torch.nn.Embedding(n_e, e_dim).to(dev)


class _GraphLoop:
    def __init__(self, ld, img, cond, unc, steps, eta, noise_seed=None, quantize=False):
        from stedm_amd.ddim import DDIMSampler, StepGraph
        smp = DDIMSampler(ld, use_graph=True)
        smp.make_schedule(steps, ddim_eta=eta, verbose=False)
        self.n = int(smp.ddim_timesteps.shape[0])
        opts = smp._step_opts(1.0, 0.0, smp._codebook(img.shape[1]) if quantize else None, noise_seed, True, 0)
        self.img = img
        self.g = StepGraph(smp, img, cond, unc, 1.5, opts=opts)
        self.g.reset(self.n - 1)
        self.g.step_eager()
        with self.g.stream_ctx():
            self.g.capture()
        self.g.join()

    def run(self):
        self.g.reset(self.n - 1)
        with self.g.stream_ctx():
            for _ in range(self.n):
                self.g.replay()
        self.g.join()


class _EagerLoop:
    def __init__(self, ld, img, cond, unc, steps, noises):
        from stedm_amd.ddim import DDIMSampler
        self.smp = DDIMSampler(ld, use_graph=False)
        self.smp.make_schedule(steps, ddim_eta=1.0, verbose=False)
        self.n = int(self.smp.ddim_timesteps.shape[0])
        self.img, self.cond, self.unc, self.noises = img, cond, unc, noises

    def run(self):
        out, _ = self.smp.ddim_sampling(self.cond, tuple(self.img.shape), x_T=self.img, unconditional_guidance_scale=1.5,
                                        unconditional_conditioning=self.unc, noises=self.noises, log_every_t=10 ** 9)
        self.img.copy_(out)


def time_run(lp, xT):
    lp.img.copy_(xT)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lp.run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernels(dev, B, reps=200):
    """The update kernels and the quantize kernel alone (timed by rocprofv3 in its own run)."""
    from stedm_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    shape = (B, 4, 32, 32)
    x, e_c, e_u = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
    cb = torch.randn(8192, 4, device=dev, generator=g) * 0.5
    coefs = torch.rand(50, 4, device=dev, generator=g) * 0.5 + 0.25
    step = torch.tensor([20], dtype=torch.int32, device=dev)
    xp, px, nz = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    for _ in range(reps):
        ops.ddim_step(x, e_c, e_u, coefs, xp, pred_x0=px, step_idx=step, cfg_scale=1.5)
        ops.ddim_step_ex(x, e_c, e_u, coefs, xp, pred_x0=px, draw=True, step_idx=step, n_iters=50, cfg_scale=1.5, seed=3)
        ops.ddim_step_ex(x, e_c, e_u, coefs, xp, pred_x0=px, draw=True, step_idx=step, n_iters=50, cfg_scale=1.5, seed=3, temperature=0.9,
                         noise_dropout=0.1, eps_out=e_u, noise_out=nz)
        ops.ddim_quantize_x0(px, e_u, coefs, cb, xp, noise=nz, step_idx=step)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8,1")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ddim_eta: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    if args.kernels:
        kernels(dev, int(args.batches.split(",")[0]))
        return
    ld = bench.build_model(dev, args.precision)
    ld.first_stage_model = _FirstStage(dev)
    res = {"precision": ld.model.diffusion_model.precision.label, "workload": f"NS32 32x32, CFG 1.5, DDIM-{args.steps}", "batches": {}}
    from stedm_amd import ops
    for B in (int(b) for b in args.batches.split(",")):
        xT, cond, unc = bench.synth_inputs(dev, B, 0)
        lp = {"graph_eta1": _GraphLoop(ld, xT.clone(), cond, unc, args.steps, 1.0, noise_seed=5),
              "graph_eta0": _GraphLoop(ld, xT.clone(), cond, unc, args.steps, 0.0),
              "graph_eta1_quant": _GraphLoop(ld, xT.clone(), cond, unc, args.steps, 1.0, noise_seed=5, quantize=True)}
        n = lp["graph_eta1"].n
        noises = [ops.philox_normal(B, (4, 32, 32), 5, 1 + i, dev) for i in range(n)]
        lp["eager_eta1_list"] = _EagerLoop(ld, xT.clone(), cond, unc, args.steps, noises)
        order = list(lp)
        for k in order:
            time_run(lp[k], xT)
        ts = {k: [] for k in lp}
        for r in range(args.rounds):
            for k in (order if r % 2 == 0 else order[::-1]):
                ts[k].append(time_run(lp[k], xT))
        rec = {}
        for k, v in ts.items():
            med = sorted(v)[len(v) // 2] * 1e3
            rec[k] = {"iterations": n, "ms_per_loop_median": round(med, 3), "ms_min": round(min(v) * 1e3, 3), "ms_max": round(max(v) * 1e3, 3),
                      "ms_per_step": round(med / n, 4)}
        g1, g0 = rec["graph_eta1"]["ms_per_step"], rec["graph_eta0"]["ms_per_step"]
        rec["step_ratio_graph_eta1_over_eta0"] = round(g1 / g0, 4)
        rec["step_ratio_eager_list_over_graph_eta1"] = round(rec["eager_eta1_list"]["ms_per_step"] / g1, 4)
        rec["quant_extra_ms_per_step"] = round(rec["graph_eta1_quant"]["ms_per_step"] - g1, 4)
        assert all(bool(torch.isfinite(x.img).all()) for x in lp.values()), "non-finite latents"
        del lp, noises
        res["batches"][str(B)] = rec
        print(f"[bench_ddim_eta] B={B}: graph eta1 {g1:.3f} ms/step, graph eta0 {g0:.3f} (eta1/eta0 x{rec['step_ratio_graph_eta1_over_eta0']:.4f}), "
              f"eager eta1 list {rec['eager_eta1_list']['ms_per_step']:.3f} (x{rec['step_ratio_eager_list_over_graph_eta1']:.3f} of graph), "
              f"quantize_x0 +{rec['quant_extra_ms_per_step']:.4f} ms/step", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
