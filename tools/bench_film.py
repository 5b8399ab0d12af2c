#!/usr/bin/env python
"""The headline-shaped denoising step (bench.py's own inputs and timed loop: batch 64, DDIM-50 step with CFG 1.5 under hipGraph replay,
the NS32 net) for the same net with and without use_scale_shift_norm (AdaGN / FiLM ResBlocks), alternating in one process, --runs each;
plus stedm_gn_apply16c_film alone against stedm_gn_apply16c on the widest out_layers shapes of that step, in GB/s of the bytes each
moves (4 B read + 2 B written per element). Information only: no claim is made for the new mode.

    python tools/bench_film.py [--steps 100] [--warmup 5] [--runs 3] [--batch 64] [--precision f16] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def build(dev, precision, film):
    import bench
    from stedm_amd.latent_diffusion import LatentDiffusion
    from stedm_amd.unet import UNetModel
    from stedm_amd.utils import prng
    unet = UNetModel(precision=precision, use_scale_shift_norm=film, **bench.NS32).eval()
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


def apply_kernel(dev, precision, B, runs):
    """the FiLM apply pass and the plain one on out_layers[0] shapes of the step (decoder batch 2 B), warm caches, back to back launches"""
    from stedm_amd import ops
    from stedm_amd.ops import Precision
    prec = Precision.parse(precision)
    out = {}
    for (H, C) in ((32, 128), (16, 512), (8, 1024)):
        Bd = 2 * B
        x = torch.randn((Bd, H, H, C), device=dev)
        cs = torch.empty((Bd, ops.gn_chan_nslab(H * H), C, 2), device=dev)
        ops.gn_chan_stats(x, cs)
        hi = torch.empty((Bd, H, H, C), dtype=torch.int16, device=dev)
        gm, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        film = torch.randn((Bd, 2 * C), device=dev) * 0.5
        gb = x.numel() * 6 / 1e9
        f_film = lambda: ops.gn_apply16c_film(x, cs, hi, None, prec, gm, bt, film, 0, 2 * C, 1e-5, 32, 1)
        f_plain = lambda: ops.gn_apply16c(x, cs, None, None, hi, None, prec, gm, bt, 1e-5, 32, 1)
        rf = [round(gb / time_kernel(f_film), 1) for _ in range(runs)]
        rp = [round(gb / time_kernel(f_plain), 1) for _ in range(runs)]
        out[f"{Bd}x{H}x{H}x{C}"] = dict(film_gbs=rf, plain_gbs=rp, mbytes=round(gb * 1e3, 1))
        print(f"apply {Bd}x{H}x{H}x{C} ({gb * 1e3:.0f} MB): film {rf} GB/s  plain {rp} GB/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--json")
    args = ap.parse_args()
    import bench
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ms = {"plain": [], "film": []}
    for _ in range(args.runs):
        for name in ("plain", "film"):
            ld = build(dev, args.precision, name == "film")
            xT, cond, unc = bench.synth_inputs(dev, args.batch, 0, 1)
            dt, _ = bench.run_steps(ld, xT, cond, unc, args.warmup, args.steps, 1)
            try:
                ld.model.diffusion_model.check_f16_range("tools/bench_film.py")
            except Exception as e:      # (timing only: an fp16 overflow of the synthetic weights is reported, not fatal)
                print(f"note ({name}): {e}")
            ms[name].append(round(1e3 * dt / args.steps, 4))
            del ld
            torch.cuda.empty_cache()
    res = {n: dict(runs=v, median=statistics.median(v), spread=round(max(v) - min(v), 4)) for n, v in ms.items()}
    for n, r in res.items():
        print(f"step {n:6s} ms per step {r['runs']}  median {r['median']:.4f}  spread {r['spread']:.4f}")
    kern = apply_kernel(dev, args.precision, args.batch, args.runs)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(steps=args.steps, warmup=args.warmup, batch=args.batch, precision=args.precision, step_ms=res, apply=kern), f, indent=1)


if __name__ == "__main__":
    main()
