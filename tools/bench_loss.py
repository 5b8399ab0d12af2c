"""Loss kernels at the training benchmark's shape (tools/bench_train.py: batch 64, 32x32x4 latents -> pred [64, 4, 32, 32], n = 4096 per sample):
stedm_l1_loss (the plain objective) beside stedm_diffusion_loss (l1 and l2, with d_pred, with and without d_logvar). Stream time per call
(two launches each) from device events around runs of --calls back-to-back calls, the candidates alternating within every round; median and
spread over --rounds. Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_loss.py --rounds 2`."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stedm_amd import ops  # noqa: E402
from stedm_amd.schedule import lvlb_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--latent", type=int, default=32)
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--rounds", type=int, default=11)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_loss needs a GPU (no CPU fallback)")
dev = torch.device("cuda:0")
B, L, T = a.batch, a.latent, 1000
g = torch.Generator(device="cpu").manual_seed(1)
pred = torch.randn(B, 4, L, L, generator=g).to(dev)
tgt = torch.randn(B, 4, L, L, generator=g).to(dev)
t = torch.randint(0, T, (B,), generator=g).to(dev)
logvar = (0.3 * torch.randn(T, generator=g)).to(dev)
lvlb = torch.from_numpy(lvlb_weights(T, 0.0015, 0.0205)).to(dev)
dpred, dlv = torch.empty_like(pred), torch.empty(T, device=dev)
ws1, loss1 = torch.empty(1024, dtype=torch.float64, device=dev), torch.empty(1, device=dev)
n = pred.numel() // B
ws, out = torch.empty(ops.diffusion_loss_ws_doubles(B, n), dtype=torch.float64, device=dev), torch.empty(4, device=dev)
cands = {
    "stedm_l1_loss": lambda: ops.l1_loss(pred, tgt, dpred, ws1, loss1),
    "stedm_diffusion_loss l1": lambda: ops.diffusion_loss(pred, tgt, t, logvar, lvlb, 0, 1.0, 0.0, 1.0, dpred, None, ws, out),
    "stedm_diffusion_loss l2 + elbo": lambda: ops.diffusion_loss(pred, tgt, t, logvar, lvlb, 1, 1.0, 0.5, 1.0, dpred, None, ws, out),
    "stedm_diffusion_loss l2 + elbo + d_logvar": lambda: ops.diffusion_loss(pred, tgt, t, logvar, lvlb, 1, 1.0, 0.5, 1.0, dpred, dlv, ws, out),
}
for f in cands.values():
    for _ in range(20):
        f()
torch.cuda.synchronize()
times = {k: [] for k in cands}
for _ in range(a.rounds):
    for k, f in cands.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            f()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
moved = 12 * pred.numel()           # bytes: pred and target read, d_pred written
print(f"B={B} n={n} ({moved / 1e6:.2f} MB per call); stream time per call (2 launches), median [min .. max] over {a.rounds} rounds of {a.calls} calls")
for k, v in times.items():
    print(f"  {k:44s} {statistics.median(v):7.2f} us  [{min(v):.2f} .. {max(v):.2f}]")
