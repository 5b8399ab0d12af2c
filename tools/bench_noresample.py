#!/usr/bin/env python
"""The headline-shaped denoising step (bench.py's own inputs and timed loop: DDIM-50 step with CFG 1.5 under hipGraph replay, the NS32 net)
at batch 64 and 8 for the same net with conv_resample True and False, alternating in one process, --runs each; plus stedm_avgpool2x2 and
stedm_replicate2x2 alone (with their statistics, as the walk calls them) on the shapes of that step, against a torch device-to-device copy
moving the same number of bytes (half read, half written) timed in the same run as the yardstick. Information only: no claim is made for
the new mode.

    python tools/bench_noresample.py [--steps 100] [--warmup 5] [--runs 3] [--batches 64,8 | --batches "" for the kernels alone] [--precision f16] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build(dev, precision, conv_resample):
    import bench
    from stedm_amd.latent_diffusion import LatentDiffusion
    from stedm_amd.unet import UNetModel
    from stedm_amd.utils import prng
    unet = UNetModel(precision=precision, conv_resample=conv_resample, **bench.NS32).eval()
    prng.fill_module_(unet, seed=0)
    return LatentDiffusion(unet, linear_start=0.0015, linear_end=0.0205, image_size=32, channels=4, conditioning_key="hybrid", loss_type="l1",
                           use_graph=True).to(dev)


def time_kernel(fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def kernels(dev, B, runs):
    """the two kernels on the step's shapes (the pool at encoder batch B, the nearest x2 at decoder batch 2 B), warm caches, back to back
    launches; bytes = input read once + output written once (the statistics are not counted)"""
    from stedm_amd import ops
    out = {}
    for kind, Bk, H, C in (("avgpool2x2", B, 32, 128), ("avgpool2x2", B, 16, 512), ("replicate2x2", 2 * B, 8, 1024), ("replicate2x2", 2 * B, 16, 512)):
        x = torch.randn((Bk, H, H, C), device=dev)
        Ho = H // 2 if kind == "avgpool2x2" else 2 * H
        y = torch.empty((Bk, Ho, Ho, C), device=dev)
        cs = torch.empty((Bk, ops.gn_chan_nslab(Ho * Ho), C, 2), device=dev)
        nbytes = (x.numel() + y.numel()) * 4
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        fn = (lambda: ops.avgpool2x2(x, y, cs)) if kind == "avgpool2x2" else (lambda: ops.replicate2x2(x, y, 1.0, False, cs))
        rk = [round(nbytes / time_kernel(fn) / 1e9, 1) for _ in range(runs)]
        rc = [round(nbytes / time_kernel(lambda: dst.copy_(src)) / 1e9, 1) for _ in range(runs)]
        frac = round(statistics.median(rk) / statistics.median(rc), 3)
        out[f"{kind} {Bk}x{H}x{H}x{C}"] = dict(kernel_gbs=rk, copy_gbs=rc, mbytes=round(nbytes / 1e6, 1), fraction_of_copy=frac)
        print(f"{kind} {Bk}x{H}x{H}x{C} ({nbytes / 1e6:.0f} MB): kernel {rk} GB/s  device copy {rc} GB/s  kernel / copy {frac:.2f}", flush=True)
        del x, y, cs, src, dst
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", default="64,8")
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--json")
    args = ap.parse_args()
    import bench
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    res = {}
    for B in [int(v) for v in args.batches.split(",") if v]:
        ms = {"conv_resample=True": [], "conv_resample=False": []}
        for _ in range(args.runs):
            for name in ms:
                ld = build(dev, args.precision, name.endswith("True"))
                xT, cond, unc = bench.synth_inputs(dev, B, 0, 1)
                dt, _ = bench.run_steps(ld, xT, cond, unc, args.warmup, args.steps, 1)
                try:
                    ld.model.diffusion_model.check_f16_range("tools/bench_noresample.py")
                except Exception as e:      # (timing only: an fp16 overflow of the synthetic weights is reported, not fatal)
                    print(f"note ({name}): {e}")
                ms[name].append(round(1e3 * dt / args.steps, 4))
                del ld
                torch.cuda.empty_cache()
        res[f"B{B}"] = {n: dict(runs=v, median=statistics.median(v), spread=round(max(v) - min(v), 4)) for n, v in ms.items()}
        for n, r in res[f"B{B}"].items():
            print(f"step B={B} {n:20s} ms per step {r['runs']}  median {r['median']:.4f}  spread {r['spread']:.4f}", flush=True)
    kern = kernels(dev, 64, args.runs)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(steps=args.steps, warmup=args.warmup, precision=args.precision, step_ms=res, kernels=kern), f, indent=1)


if __name__ == "__main__":
    main()
