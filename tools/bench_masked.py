#!/usr/bin/env python3
"""Masked DDIM sampling on the graphed step: the hipGraph-replayed denoising step (NS32, DDIM-50 + CFG 1.5) with and without a mask
(the extra node: stedm_ddim_mask_blend, q_sample of x0 blended into the latents with noise drawn in the kernel), timed in one process,
the two alternating run for run. Per batch: ms per step of each (median of the rounds, with min / max), and the ratio masked / unmasked.
    python tools/bench_masked.py [--batches 64,1] [--rounds 8] [--precision f16]
The blend kernel alone: run this under `rocprofv3 --kernel-trace --stats` (a run of its own) and read ddim_mask_blend_kernel's row."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def graphs(ld, B, dev):
    """two captured steps over the same model and inputs: unmasked, and masked (left half kept from a per-sample x0)"""
    from stedm_amd import parallel as par
    from stedm_amd.ddim import DDIMSampler, StepGraph
    xT, cond, unc = bench.synth_inputs(dev, B, 0)
    x0 = par.per_sample_normal(5, range(B), (4, 32, 32)).to(dev)
    mask = torch.zeros(B, 1, 32, 32, device=dev)
    mask[..., :16] = 1.0
    smp = DDIMSampler(ld, use_graph=True)
    smp.make_schedule(50, ddim_eta=0.0, verbose=False)
    n = smp.ddim_timesteps.shape[0]
    out = {}
    for name, blend in (("plain", None), ("masked", (mask, x0, 1234, 0))):
        img = xT.clone()
        sg = StepGraph(smp, img, cond, unc, 1.5, blend=blend)
        sg.reset(n - 1)
        sg.step_eager()
        with sg.stream_ctx():
            sg.capture()
        sg.join()
        out[name] = (sg, img)
    return out, xT, n


def time_run(sg, img, xT, n):
    """one DDIM-50 run from x_T by graph replay -> seconds per step"""
    with sg.stream_ctx():
        sg.reset(n - 1)
        img.copy_(xT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            sg.replay()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
    sg.join()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_masked: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision)
    res = {"precision": ld.model.diffusion_model.precision.label, "workload": "NS32 32x32 DDIM-50 + CFG 1.5 step, hipGraph replay", "batches": {}}
    for B in (int(b) for b in args.batches.split(",")):
        gs, xT, n = graphs(ld, B, dev)
        for name in gs:                                       # warm-up run of each
            time_run(*gs[name], xT, n)
        ts = {k: [] for k in gs}
        for r in range(args.rounds):
            for name in (("plain", "masked") if r % 2 == 0 else ("masked", "plain")):
                ts[name].append(time_run(*gs[name], xT, n))
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in ts.items()}
        rec = {k: {"ms_per_step_median": round(med[k], 4), "ms_min": round(min(ts[k]) * 1e3, 4), "ms_max": round(max(ts[k]) * 1e3, 4)} for k in ts}
        rec["ratio_masked_over_plain"] = round(med["masked"] / med["plain"], 4)
        res["batches"][str(B)] = rec
        print(f"[bench_masked] B={B}: plain {med['plain']:.4f} ms/step, masked {med['masked']:.4f} ms/step, ratio {rec['ratio_masked_over_plain']:.4f}",
              flush=True)
        finite = all(bool(torch.isfinite(img).all()) for _, img in gs.values())
        assert finite, "non-finite latents"
        del gs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
