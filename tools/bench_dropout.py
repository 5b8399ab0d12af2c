#!/usr/bin/env python
"""The training step (forward + L1 + backward + AdamW / EMA, the NS32 net, bf16, UNetTrainer.train_step) at batch 8 and 64 with
`dropout` 0 against 0.1, both models in train(), alternating in one process, --runs rounds of --steps steps each; plus the GroupNorm
apply pass and the GroupNorm backward alone on the three decoder shapes of DESIGN.md section 4.3, with and without DROP, in TB/s of the
bytes each moves (apply: 4 B read + 2 B written per element; backward: x, dA read, dx and its 16-bit plane written: 14 B per element).
Information only: no claim is made for the dropout mode.

    python tools/bench_dropout.py [--steps 10] [--warmup 3] [--runs 3] [--batches 8,64] [--precision bf16] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

NS32 = dict(image_size=32, in_channels=7, model_channels=128, out_channels=4, num_res_blocks=2, attention_resolutions=[32, 16, 8],
            channel_mult=[1, 4, 8], num_heads=8)
DROP = (0.1, 0x1234ABCD5678, 0x55000000 + 5, 7, None)


def trainer(dev, precision, dropout):
    from stedm_amd.train import UNetTrainer
    from stedm_amd.unet import UNetModel
    from stedm_amd.utils import prng
    m = UNetModel(precision=precision, dropout=dropout, **NS32).train()
    prng.fill_module_(m, seed=0)
    m.dropout_seed = 1
    return UNetTrainer(m.to(dev), lr=1e-5)


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


def steps(dev, precision, B, nsteps, warmup, runs):
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(B, 4, 32, 32, generator=g).to(dev); cc = torch.randn(B, 3, 32, 32, generator=g).to(dev)
    ctx = torch.randn(B, 512, generator=g).to(dev); tgt = torch.randn(B, 4, 32, 32, generator=g).to(dev)
    t = torch.randint(0, 1000, (B,), generator=g).to(dev)
    sides = {"dropout 0": trainer(dev, precision, 0.0), "dropout 0.1": trainer(dev, precision, 0.1)}
    for tr in sides.values():
        for _ in range(warmup):
            tr.train_step(x, cc, t, ctx, tgt)
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(runs):
        for k, tr in sides.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(nsteps):
                tr.train_step(x, cc, t, ctx, tgt)
            torch.cuda.synchronize(); ms[k].append(round((time.perf_counter() - t0) / nsteps * 1e3, 3))
    res = {k: dict(runs=v, median=statistics.median(v), spread=round(max(v) - min(v), 3)) for k, v in ms.items()}
    for k, r in res.items():
        print(f"train step B={B} {precision} {k:12s} ms per step {r['runs']}  median {r['median']:.3f}  spread {r['spread']:.3f}")
    del sides
    torch.cuda.empty_cache()
    return res


def passes(dev, precision, B, runs):
    """the apply pass and the backward on out_layers[0] shapes of the step, warm caches, back to back launches"""
    from stedm_amd import ops
    from stedm_amd.ops import Precision
    prec = Precision.parse(precision)
    out = {}
    for (H, C) in ((32, 128), (16, 512), (8, 1024)):
        G = 32
        x = torch.randn((B, H, H, C), device=dev)
        dA = torch.randn((B, H, H, C), device=dev)
        cs = torch.empty((B, ops.gn_chan_nslab(H * H), C, 2), device=dev)
        ops.gn_chan_stats(x, cs)
        mr = torch.empty((B, G, 2), device=dev)
        ops.gn_fold(cs, None, G, H * H, 1e-5, mr)
        hi = torch.empty((B, H, H, C), dtype=torch.int16, device=dev)
        dx = torch.empty_like(x)
        gm, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty((ops.gn_bwd_ws_floats(B, H * H, C, G),), device=dev)
        fa, fb = x.numel() * 6 / 1e12, x.numel() * 14 / 1e12
        f = dict(
            apply_plain=lambda: ops.gn_apply16c(x, cs, None, None, hi, None, prec, gm, bt, 1e-5, G, 1),
            apply_drop=lambda: ops.gn_apply16c_drop(x, cs, hi, None, prec, gm, bt, DROP, 1e-5, G, 1),
            bwd_plain=lambda: ops.gn_bwd(x, None, mr, gm, bt, G, 1, dA, None, ws, dx, False, None, False, (hi, None), prec, dg, db, False),
            bwd_drop=lambda: ops.gn_bwd_drop(x, mr, gm, bt, G, 1, dA, None, ws, dx, False, (hi, None), prec, dg, db, False, DROP))
        r = {k: [round((fa if k.startswith("apply") else fb) / time_kernel(fn), 2) for _ in range(runs)] for k, fn in f.items()}
        out[f"{B}x{H}x{H}x{C}"] = r
        print(f"{B}x{H}x{H}x{C} TB/s: " + "  ".join(f"{k} {v}" for k, v in r.items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--json")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    res = {}
    for B in [int(v) for v in args.batches.split(",")]:
        res[f"B{B}"] = steps(dev, args.precision, B, args.steps, args.warmup, args.runs)
    kern = passes(dev, args.precision, 64, args.runs)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(steps=args.steps, warmup=args.warmup, precision=args.precision, step_ms=res, passes=kern), f, indent=1)


if __name__ == "__main__":
    main()
