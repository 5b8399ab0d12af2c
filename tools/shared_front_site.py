#!/usr/bin/env python
"""Per-site measurement behind UNetModel._shared_front_rule: the CFG seam of forward_cfg - middle_block[0], the hand-over and the style block
(middle_block[1]) - in its present form (middle_block[0] at batch B, two broadcast copies to 2B, the style block wholly at 2B) against the
shared front (in_layers' GroupNorm riding on middle_block[0]'s tail convolution at batch B, in_layers' convolution once per CFG pair as
partials, the finish pass at 2B, the tail convolution with the shared residual: UNetModel._res_front).

One eager forward_cfg records what the seam runs on; each form is then captured as REPS back-to-back repetitions in a hipGraph and the
graph is timed with HIP events, median of --iters launches. Points: --points batch:latent pairs.

    python tools/shared_front_site.py [--points 64:32,64:64,48:32,32:32] [--precision f16] [--json FILE]
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
    ap.add_argument("--points", default="64:32,64:64,48:32,32:32")
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--json")
    args = ap.parse_args()
    import bench
    from stedm_amd import ops
    from stedm_amd.unet import UNetModel
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    ld = bench.build_model(dev, args.precision, use_graph=False)
    m = ld.model.diffusion_model
    mid = list(m.middle_block)
    side = torch.cuda.Stream()
    rows = []
    for point in args.points.split(","):
        B, size = [int(v) for v in point.split(":")]
        g = torch.Generator(device="cpu").manual_seed(11)
        x = torch.randn(B, 4, size, size, generator=g).to(dev)
        cc = (torch.randn(B, 3, size, size, generator=g) > 0).float().to(dev)
        ctx, ctx_u = torch.randn(B, 512, generator=g).to(dev), torch.randn(1, 512, generator=g).repeat(B, 1).to(dev)
        t = torch.full((B,), 951, dtype=torch.long, device=dev)
        rec = {}
        orig = UNetModel._run_block

        def spy(self, tag, blk, h, skip, emb_all, emb_bstride, style_all, *a, _rec=rec, **kw):
            if tag == "mid.a":
                _rec.update(h=h, emb_e=emb_all, stride=emb_bstride, cs=dict(self._cs), pre=dict(self._pre16))
            if tag == "mid.b":
                _rec.update(emb_d=emb_all, style=style_all)
            return orig(self, tag, blk, h, skip, emb_all, emb_bstride, style_all, *a, **kw)

        UNetModel._run_block = spy
        m.cfg_shared_front = False
        try:
            m.forward_cfg(x, cc, t, ctx, ctx_u, uniform_t=True)
        finally:
            UNetModel._run_block = orig
        torch.cuda.synchronize()
        nn_ = m._first_norm(mid[2])
        m.cfg_shared_front = True
        admitted = m._shared_front("mid.b.1", mid[1].block, tuple(rec["h"].shape), nn_)

        def region(front):
            m._cs, m._pre16 = dict(rec["cs"]), dict(rec["pre"])
            h = m._run_block("mid.a", mid[:1], rec["h"], None, rec["emb_e"], rec["stride"], None, next_layer=mid[1] if front else None)
            if front:
                return m._res_front("mid.b.1", mid[1].block, h, rec["style"], nn_)
            return m._run_block("mid.b", mid[1:2], m._replicate(h, 2), None, rec["emb_d"], rec["stride"], rec["style"], li0=1, next_layer=mid[2])

        us = {}
        for front in ((False, True) if admitted else (False,)):
            with torch.cuda.stream(side):
                region(front)
                torch.cuda.synchronize()
                gr = ops.Graph()
                with gr:
                    for _ in range(REPS):
                        region(front)
                ts = []
                for _ in range(args.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); gr.launch(); e1.record()
                    torch.cuda.synchronize()
                    ts.append(1e3 * e0.elapsed_time(e1) / REPS)
            us[front] = statistics.median(ts)
        m.cfg_shared_front = None
        key = [k for k in m._consts if isinstance(k, tuple) and k and k[0] == "sfront" and k[-1] is True and k[2] == 2 * B]
        rows.append(dict(batch=B, latent=size, shape=list(rec["h"].shape), partials=m._consts[key[-1]] if key else 0, rule=bool(
            UNetModel._shared_front_rule(2 * B, rec["h"].shape[1], rec["h"].shape[2], rec["h"].shape[3])),
            present_us=round(us[False], 1), front_us=round(us[True], 1) if True in us else None,
            gain_us=round(us[False] - us[True], 1) if True in us else None))
    print("| batch B | latent | shared tensor | partials | rule | present form us | shared front us | gain us |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['batch']} | {r['latent']}^2 | {' x '.join(str(v) for v in r['shape'])} | {r['partials'] or 'not admitted'} | {r['rule']} | {r['present_us']} | "
              f"{r['front_us'] if r['front_us'] is not None else '-'} | {r['gain_us'] if r['gain_us'] is not None else '-'} |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(precision=args.precision, reps=REPS, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
