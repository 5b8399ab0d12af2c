#!/usr/bin/env python3
"""The epoch-end monitoring images (LDM_Diffusion.sample_test_images) and the kernel under them, in one process, the variants alternated
run for run, medians of --rounds:

  loops    the reference-native U-Net (bench.REF128: 128 x 128 x 3 latents), DDIM-128 (143 iterations), eta 0, graphed loops:
    * batched   the two runs of sample_test_images: B = 4 unguided, then B = 4 guided with per-sample scales [3, 5, 3, 5]
                (stedm_ddim_step_rows) against one shared unconditional conditioning;
    * literal   the reference's eight batch-1 sample_log calls (ldm_diffusion.py:183-201): four unguided, four guided at 3, 5, 3, 5
                (stedm_ddim_step), each graphed as well.
    The VQ decode is the same work in both forms and is not timed.
  kernels  stedm_ddim_step_rows (uniform scale 1.5 in the device array) against stedm_ddim_step (cfg_scale 1.5) on the same operands at
           [4,3,128,128], [16,3,128,128] and [64,4,32,32]: --launches launches between two device events, and the largest difference of the
           two results.

    python tools/bench_epoch_samples.py [--rounds 3] [--steps 128] [--precision f16] [--launches 200] [--no-loops] [--no-kernels]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

SCALES = [3.0, 5.0, 3.0, 5.0]
KERNEL_SHAPES = [(4, 3, 128, 128), (16, 3, 128, 128), (64, 4, 32, 32)]


def median(v):
    return sorted(v)[len(v) // 2]


def kernels(dev, launches, rounds):
    from stedm_amd import ops
    out = {}
    g = torch.Generator(device="cpu").manual_seed(5)
    coefs = (torch.rand(50, 4, generator=g) * 0.5 + 0.25).to(dev)
    step = torch.tensor([20], dtype=torch.int32, device=dev)
    for shape in KERNEL_SHAPES:
        x, e_c = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
        e_u = (torch.randn(shape, generator=g) * 0.8).to(dev) + 0.1 * e_c
        sc = torch.full((shape[0],), 1.5, dtype=torch.float32, device=dev)
        xp, px = torch.empty_like(x), torch.empty_like(x)
        run = {"ddim_step": lambda: ops.ddim_step(x, e_c, e_u, coefs, xp, pred_x0=px, step_idx=step, cfg_scale=1.5),
               "ddim_step_rows": lambda: ops.ddim_step_rows(x, e_c, e_u, coefs, xp, sc, pred_x0=px, step_idx=step)}
        res = {}
        for k, f in run.items():
            for _ in range(20):
                f()
            res[k] = xp.clone()
        ts = {k: [] for k in run}
        order = list(run)
        for r in range(rounds):
            for k in (order if r % 2 == 0 else order[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(launches):
                    run[k]()
                b.record()
                b.synchronize()
                ts[k].append(a.elapsed_time(b) * 1e3 / launches)
        mb = 6 * x.numel() * 4 / 1e6                       # x, e_c, e_u read once; x_prev, pred_x0 written; (the scalar kernel re-reads)
        rec = {k: {"us_per_launch_median": round(median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)} for k, v in ts.items()}
        rec["rows_over_scalar"] = round(rec["ddim_step_rows"]["us_per_launch_median"] / rec["ddim_step"]["us_per_launch_median"], 3)
        rec["max_abs_diff"] = float((res["ddim_step"] - res["ddim_step_rows"]).abs().max())
        rec["operand_MB"] = round(mb, 2)
        out["x".join(str(d) for d in shape)] = rec
        print(f"[bench_epoch_samples] kernels {shape}: ddim_step {rec['ddim_step']['us_per_launch_median']} us, "
              f"ddim_step_rows {rec['ddim_step_rows']['us_per_launch_median']} us (x{rec['rows_over_scalar']}), max|diff| {rec['max_abs_diff']:.2e}",
              flush=True)
    return out


def loops(dev, precision, steps, rounds):
    from stedm_amd.latent_diffusion import LatentDiffusion
    from stedm_amd.unet import UNetModel
    from stedm_amd.utils import prng
    unet = UNetModel(precision=precision, **bench.REF128).eval()
    prng.fill_module_(unet, seed=0)
    ld = LatentDiffusion(unet, linear_start=0.0015, linear_end=0.0205, image_size=128, channels=3, conditioning_key="hybrid", loss_type="l1",
                         use_graph=True).to(dev)
    g = torch.Generator(device="cpu").manual_seed(13)
    xT = torch.randn(8, 3, 128, 128, generator=g).to(dev)
    lay = (torch.randn(1, 3, 128, 128, generator=g) > 0).float().to(dev)           # one test condition image for every row
    ctx = torch.randn(4, 512, generator=g).to(dev)                                   # four test styles
    ctx_u = torch.randn(1, 512, generator=g).to(dev)
    cond = lambda rows: {"c_concat": [lay.expand(len(rows), -1, -1, -1).contiguous()], "c_crossattn": [ctx[rows].contiguous()]}
    unc = lambda n: {"c_concat": [lay.expand(n, -1, -1, -1).contiguous()], "c_crossattn": [ctx_u.expand(n, -1).contiguous()]}
    kw = dict(eta=0.0, log_every_t=10 ** 9)

    def batched():
        a, _ = ld.sample_log(cond([0, 1, 2, 3]), 4, True, steps, x_T=xT[:4], **kw)
        b, _ = ld.sample_log(cond([0, 0, 1, 1]), 4, True, steps, x_T=xT[4:], unconditional_conditioning=unc(4),
                             unconditional_guidance_scale=SCALES, **kw)
        return torch.cat([a, b])

    def literal():
        outs = [ld.sample_log(cond([i]), 1, True, steps, x_T=xT[i:i + 1], **kw)[0] for i in range(4)]
        for j, (i, s) in enumerate(zip([0, 0, 1, 1], SCALES)):
            outs.append(ld.sample_log(cond([i]), 1, True, steps, x_T=xT[4 + j:5 + j], unconditional_conditioning=unc(1),
                                      unconditional_guidance_scale=s, **kw)[0])
        return torch.cat(outs)

    forms = {"batched": batched, "literal": literal}
    finals, ts = {}, {k: [] for k in forms}
    for k, f in forms.items():                    # warm-up: packs weights, loads code objects
        finals[k] = f()
    torch.cuda.synchronize()
    order = list(forms)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            forms[k]()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    assert all(bool(torch.isfinite(v).all()) for v in finals.values()), "non-finite latents"
    a, b = finals["batched"].double(), finals["literal"].double()
    rec = {k: {"s_median": round(median(v), 3), "s_min": round(min(v), 3), "s_max": round(max(v), 3)} for k, v in ts.items()}
    rec["literal_over_batched"] = round(rec["literal"]["s_median"] / rec["batched"]["s_median"], 3)
    rec["latents_rel_l2_batched_vs_literal"] = float((a - b).norm() / b.norm())
    rec["workload"] = f"REF128 128x128x3 latents, DDIM-{steps}, eta 0, {unet.precision.label}, graphed loops, eight images"
    print(f"[bench_epoch_samples] loops: batched {rec['batched']['s_median']} s, literal eight calls {rec['literal']['s_median']} s "
          f"(x{rec['literal_over_batched']}), latents rel-L2 {rec['latents_rel_l2_batched_vs_literal']:.2e}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch_samples: no GPU (timings are taken on the device only)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    res = {}
    if not args.no_kernels:
        res["kernels"] = kernels(dev, args.launches, max(args.rounds, 5))
    if not args.no_loops:
        res["loops"] = loops(dev, args.precision, args.steps, args.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
