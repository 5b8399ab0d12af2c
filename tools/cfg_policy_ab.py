#!/usr/bin/env python
"""Headline A/B of the CFG routing policies of UNetModel without touching bench.py: the benchmark's own model, inputs and timed loop
(bench.build_model / synth_inputs / run_steps) with the policy attributes set from here, the configurations alternating, --runs each.

    python tools/cfg_policy_ab.py [--steps 200] [--warmup 5] [--runs 3] [--configs default,front_off,partials_on] [--json FILE]

Configurations: default (every attribute None: the rules), front_off (cfg_shared_front False), partials_on (cfg_skip_partials True),
front_on (cfg_shared_front True), skip_all (cfg_shared_skip True: every admissible site).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CONFIGS = {"default": {}, "front_off": dict(cfg_shared_front=False), "partials_on": dict(cfg_skip_partials=True),
           "front_on": dict(cfg_shared_front=True), "skip_all": dict(cfg_shared_skip=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--configs", default="default,front_off,partials_on")
    ap.add_argument("--json")
    args = ap.parse_args()
    import bench
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    names = args.configs.split(",")
    ms = {n: [] for n in names}
    for _ in range(args.runs):
        for n in names:
            ld = bench.build_model(dev, args.precision)
            for k, v in CONFIGS[n].items():
                setattr(ld.model.diffusion_model, k, v)
            xT, cond, unc = bench.synth_inputs(dev, args.batch, 0, 1)
            dt, _ = bench.run_steps(ld, xT, cond, unc, args.warmup, args.steps, 1)
            ms[n].append(round(1e3 * dt / args.steps, 4))
            del ld
            torch.cuda.empty_cache()
    res = {n: dict(runs=v, median=statistics.median(v), spread=round(max(v) - min(v), 4)) for n, v in ms.items()}
    for n, r in res.items():
        print(f"{n:14s} ms per step {r['runs']}  median {r['median']:.4f}  spread {r['spread']:.4f}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(steps=args.steps, warmup=args.warmup, batch=args.batch, precision=args.precision, configs=res), f, indent=1)


if __name__ == "__main__":
    main()
