#!/usr/bin/env python3
"""The two forms of the LSA backward side by side, in one process, alternating, after warm-up: medians with min - max (device events).

  kernels alone : ops.lsa_bwd (fp32 matrix pipe) against ops.lsa_bwd16 (16-bit matrix pipe) at the reference shape (B = 8, 12 heads,
                  T = 4098), p = 0 and p = 0.1, f16 and bf16
  backward      : sViT.backward with lsa_bwd="f32" against "mfma16" at the shape of DESIGN 5.5.1 (B = 8, ns = 10, 512^2 style images,
                  depth 6, 12 heads, dim 256, dropout 0.1, f16)

For every pair it prints whether "mfma16" is faster by more than three times the larger of the two min - max spreads.
  python tools/bench_lsa_bwd.py [reps] [B]"""
import json, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stedm_amd import ops
from stedm_amd.style import sViT
from stedm_amd.utils import prng


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def pair(name, f32, m16, reps):
    for fn in (f32, m16, f32, m16):      # warm-up: code objects, workspaces
        fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):                # alternating
        a.append(timed(f32)); b.append(timed(m16))
    ma, mb = statistics.median(a), statistics.median(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    ok = ma - mb > 3.0 * spread
    print(f"| {name} | {ma:.2f} ({min(a):.2f} - {max(a):.2f}) | {mb:.2f} ({min(b):.2f} - {max(b):.2f}) | {ma / mb:.2f} | {'yes' if ok else 'NO'} |", flush=True)
    return dict(name=name, f32_ms=ma, f32_min=min(a), f32_max=max(a), mfma16_ms=mb, mfma16_min=min(b), mfma16_max=max(b), margin_ok=ok)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    heads, T = 12, 4098
    Tp = (T + 127) // 128 * 128
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    res = []
    print("| (ms, median of %d, min - max) | f32 | mfma16 | ratio | faster by > 3 x spread |\n|---|---|---|---|---|" % reps)
    qscale = math.exp(math.log(64 ** -0.5)) * 1.4426950408889634
    qkv = prng.normal(36, "bench.qkv", (B, T, 3 * heads * 64)).to(dev)
    dO = prng.normal(36, "bench.dO", (B * T, heads * 64)).to(dev)
    dqkv = torch.empty((B * T, 3 * heads * 64), device=dev)
    dtemp = torch.zeros((1,), device=dev)
    for mode in ("f16", "bf16"):
        prec = ops.Precision.parse(mode)
        mk = lambda shp: (torch.zeros(shp, dtype=torch.int16, device=dev), None)
        q, k, vt = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
        ops.qkv_pack(qkv, qscale, q, k, vt, B, T, Tp, heads, prec)
        for p in (0.0, 0.1):
            ws32 = torch.empty((ops.lsa_bwd_ws_floats(B, T, Tp, heads),), device=dev)
            ws16 = torch.empty((ops.lsa_bwd16_ws_bytes(B, T, Tp, heads, p),), dtype=torch.uint8, device=dev)
            f32 = lambda: ops.lsa_bwd(q, k, vt, dO, dqkv, dtemp, qscale, B, T, Tp, heads, prec, p=p, seed=7, site=1, ws=ws32)
            m16 = lambda: ops.lsa_bwd16(q, k, vt, dO, dqkv, dtemp, qscale, B, T, Tp, heads, prec, p=p, seed=7, site=1, ws=ws16)
            res.append(pair(f"LSA backward alone, {mode}, p = {p}", f32, m16, reps))
            del ws32, ws16
    del qkv, dO, dqkv
    torch.cuda.empty_cache()
    m = sViT(image_size=512, patch_size=8, num_classes=512, dim=256, depth=6, heads=heads, mlp_dim=256, pool="mean", channels=3, dim_head=64,
             dropout=0.1, emb_dropout=0.1, ns=10, t_dim=256, precision="f16").train()
    prng.fill_module_(m, seed=7)
    m = m.to(dev)
    m.keep_for_backward = True
    m.dropout_seed = 11
    x = torch.rand(B, 10, 512, 512, 3, device=dev) * 2 - 1
    m(x)
    g = prng.normal(36, "bench.g", (B, 512)).to(dev)

    def bwd(form):
        def run():
            m.lsa_bwd = form
            m.backward(g)
        return run
    res.append(pair("`sViT.backward` (6 layers), f16, dropout 0.1", bwd("f32"), bwd("mfma16"), reps))
    print(json.dumps(dict(bench="lsa_bwd", B=B, T=T, heads=heads, reps=reps, rows=res)))
    return 0 if all(r["margin_ok"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
