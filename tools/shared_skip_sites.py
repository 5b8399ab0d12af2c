#!/usr/bin/env python
"""Per-site measurement behind UNetModel._shared_skip_rule: the in_layers convolution of each decoder ResBlock under forward_cfg as ONE launch
over [h | skip] at batch 2B against the shared-skip pair (shared launch over the skip-only channels at batch B + 2B launch over the rest,
UNetModel._in_conv), at the bench shape (NS32, B = 64, 32 x 32 latents) and on the 64 x 64 latents of bench.py's ns64_step.

One eager forward_cfg per mode (cfg_shared_skip False / True) records every site's call with the buffers it ran on; each site is then
captured as REPS back-to-back repetitions in a hipGraph and the graph is timed with HIP events (GPU-bound: no launch gaps), median of
--iters launches. --pack-f also packs the 32x32x16 fragment order at the sites whose filter the model packs in the 16x16x32 order only:
their skip-only window is narrower than the 256 channels from which the dispatcher takes that kind, so the pair is not admitted on the
model's own packs; with it those sites are measured all the same.

    python tools/shared_skip_sites.py [--batch 64] [--precision f16] [--sizes 32,64] [--pack-f] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

REPS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--pack-f", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    import bench
    from stedm_amd import ops
    from stedm_amd.unet import ResBlock, UNetModel
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision, use_graph=False)
    m = ld.model.diffusion_model
    B = args.batch
    rows = []
    side = torch.cuda.Stream()
    for size in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator(device="cpu").manual_seed(11)
        x = torch.randn(B, 4, size, size, generator=g).to(dev)
        cc = (torch.randn(B, 3, size, size, generator=g) > 0).float().to(dev)
        ctx, ctx_u = torch.randn(B, 512, generator=g).to(dev), torch.randn(1, 512, generator=g).repeat(B, 1).to(dev)
        t = torch.full((B,), 951, dtype=torch.long, device=dev)
        m.forward_cfg(x, cc, t, ctx, ctx_u, uniform_t=True)          # packs, buffers
        if args.pack_f:
            for blk in m.output_blocks:
                rb = list(blk)[0]
                pk = m._packed[id(rb.in_layers[2])]
                if isinstance(rb, ResBlock) and pk.frag is None:
                    pk.frag = ops.pack_conv_weight_frag(rb.in_layers[2].weight.detach().float(), m.precision)
            m._consts = {k: v for k, v in m._consts.items() if not (isinstance(k, tuple) and k and k[0] == "sskip")}
        orig = UNetModel._in_conv
        per_mode = {}
        for on in (False, True):
            calls = []

            def rec(self, tag, rb, pk, a16, c1, x2_bmod, h, kw, _calls=calls):
                if x2_bmod > 0:
                    plan = self._shared_skip(rb, pk, a16, c1, x2_bmod, h, kw)
                    _calls.append((tag, rb, pk, a16, c1, x2_bmod, h, dict(kw), None if plan is None else plan[0]))
                return orig(self, tag, rb, pk, a16, c1, x2_bmod, h, kw)

            UNetModel._in_conv = rec
            m.cfg_shared_skip = on
            try:
                m.forward_cfg(x, cc, t, ctx, ctx_u, uniform_t=True)
            finally:
                UNetModel._in_conv = orig
            torch.cuda.synchronize()
            res = {}
            for (tag, rb, pk, a16, c1, bm, h, kw, seam) in calls:
                with torch.cuda.stream(side):                      # (a capture needs a stream of its own, not the default one)
                    orig(m, tag, rb, pk, a16, c1, bm, h, kw)       # warm (attributes, first-use costs) outside the capture
                    torch.cuda.synchronize()
                    gr = ops.Graph()
                    with gr:
                        for _ in range(REPS):
                            orig(m, tag, rb, pk, a16, c1, bm, h, kw)
                    ts = []
                    for _ in range(args.iters):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); gr.launch(); e1.record()
                        torch.cuda.synchronize()
                        ts.append(1e3 * e0.elapsed_time(e1) / REPS)
                res[tag] = dict(us=statistics.median(ts), seam=seam, C=a16[0].shape[-1], c1=c1, H=h.shape[1], cout=h.shape[-1], Bd=h.shape[0])
            per_mode[on] = res
        m.cfg_shared_skip = None
        for tag, off in per_mode[False].items():
            on = per_mode[True][tag]
            rows.append(dict(latent=size, site=tag, Bd=off["Bd"], H=off["H"], C=off["C"], c1=off["c1"], cout=off["cout"], seam=on["seam"],
                             one_launch_us=round(off["us"], 1), pair_us=round(on["us"], 1) if on["seam"] else None,
                             gain_us=round(off["us"] - on["us"], 1) if on["seam"] else None))
    print("| latent | site | 2B x H^2 | C = h + skip | cout | seam | one launch us | pair us | gain us |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['latent']} | {r['site']} | {r['Bd']} x {r['H']}^2 | {r['c1']} + {r['C'] - r['c1']} | {r['cout']} | {r['seam'] or 'not admitted'} | "
              f"{r['one_launch_us']} | {r['pair_us'] if r['pair_us'] is not None else '-'} | {r['gain_us'] if r['gain_us'] is not None else '-'} |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(batch=B, precision=args.precision, pack_f=args.pack_f, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
