#!/usr/bin/env python3
"""The patch-distributed first stage (LatentDiffusion.decode_first_stage(split=...)) on the shipped VQ-f4 architecture, two workloads:
  1. latent 256^2 -> image 1024^2 at B = 4, ks 128 / stride 64 / vqf 4 (9 crops of the 128^2 latent shape), tile_batch at its default
     (4 crops per call); with --untiled also the one-call decode of the same latents (1024-pixel rows: a shape no test covers, hence opt-in);
  2. latent 128^2 -> image 512^2 at B = 64, ks 64 / stride 32 / vqf 4 (9 crops), tile_batch at its default (1 crop per call), against the
     one-call decode where it fits (the convolution refuses planes past 2^31 elements: reported, not an error).
For each workload: stedm_fold_blend alone (fp32 output, and the uint8-only form) with its traffic rate (tile stack read once + output
written once; the weight tables are not counted), and a torch device-to-device copy moving the same number of bytes (half read, half
written) timed in the same run as the yardstick. Warm-up, then medians over the repetitions (events around each repetition).
    python tools/bench_tiled.py [bf16|f16|parity] [--reps N] [--untiled] [--only 1|2]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from stedm_amd import ops  # noqa: E402
from stedm_amd._lib import StedmHipError  # noqa: E402
from stedm_amd.latent_diffusion import LatentDiffusion  # noqa: E402
from stedm_amd.tiling import TilePlan  # noqa: E402
from stedm_amd.utils import prng  # noqa: E402
from stedm_amd.vq import VQModelInterface  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("precision", nargs="?", default="bf16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--untiled", action="store_true")
ap.add_argument("--only", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.set_grad_enabled(False)


class _Net(torch.nn.Module):
    def forward_parts(self, x, xc, t, cc, out=None, uniform_t=False):
        return x


def median_ms(fn, warm=2, reps=args.reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


m = VQModelInterface(embed_dim=3, n_embed=8192, lossconfig={"target": "torch.nn.Identity"}, precision=args.precision,
                     ddconfig=dict(double_z=False, z_channels=3, resolution=512, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4], num_res_blocks=2,
                                   attn_resolutions=[], dropout=0.0)).eval()
prng.fill_module_(m, seed=53)
m = m.to(dev)
ld = LatentDiffusion(_Net(), linear_start=0.0015, linear_end=0.0205, image_size=128, channels=3, conditioning_key="hybrid", loss_type="l1").to(dev)
ld.first_stage_model = m
W = dict(vqf=4, patch_distributed_vq=True, clip_min_weight=0.01, clip_max_weight=0.5, tie_braker=False)
WORK = [(1, 4, 256, dict(ks=(128, 128), stride=(64, 64), **W), args.untiled), (2, 64, 128, dict(ks=(64, 64), stride=(32, 32), **W), True)]

for num, B, side, split, untiled in WORK:
    if args.only and args.only != num:
        continue
    z = torch.randn(B, 3, side, side, device=dev)
    plan = TilePlan.from_split(split, side, side, False)
    nb = plan.default_tile_batch(B)
    tag = f"[{num}] latent {side}^2 -> image {side * 4}^2, B = {B}, ks {split['ks'][0]} / stride {split['stride'][0]} ({plan.L} crops, tile_batch {nb})"
    reps = max(3, args.reps // 2)
    t_tiled = median_ms(lambda: ld.decode_first_stage(z, split=split), warm=1, reps=reps)
    t_u8 = median_ms(lambda: ld.decode_first_stage(z, split=split, out_u8=True), warm=1, reps=reps)
    print(f"{tag}: tiled decode {args.precision} {t_tiled:.1f} ms, with out_u8 {t_u8:.1f} ms ({B / t_tiled * 1e3:.1f} images/s)", flush=True)
    if untiled:
        try:
            t_one = median_ms(lambda: ld.decode_first_stage(z), warm=1, reps=reps)
            print(f"{tag}: one-call decode {t_one:.1f} ms: tiled / one-call = {t_tiled / t_one:.2f}", flush=True)
        except (StedmHipError, torch.cuda.OutOfMemoryError) as e:
            print(f"{tag}: one-call decode does not fit: {str(e)[:160]}", flush=True)
    # the blend alone
    th, tw = plan.tile
    stack = torch.randn(plan.L, B, 3, th, tw, device=dev)
    w_tile, w_tie = plan.weights(dev)
    geo = (plan.out_stride, (plan.Ly, plan.Lx))
    t_f32 = median_ms(lambda: ops.fold_blend(stack, w_tile, w_tie, *geo))
    t_b8 = median_ms(lambda: ops.fold_blend(stack, w_tile, w_tie, *geo, want_f32=False, want_u8=True))
    t_unf = median_ms(lambda: ops.unfold_tiles(z, plan.ks, plan.stride))
    out_el = B * 3 * plan.out_size[0] * plan.out_size[1]
    by_f32, by_u8 = stack.numel() * 4 + out_el * 4, stack.numel() * 4 + out_el
    src = torch.empty(by_f32 // 8, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    t_copy = median_ms(lambda: dst.copy_(src))
    r_f32, r_u8, r_copy = by_f32 / t_f32 / 1e9, by_u8 / t_b8 / 1e9, src.numel() * 8 / t_copy / 1e9
    print(f"{tag}: fold_blend fp32 {t_f32:.3f} ms = {r_f32:.2f} TB/s over {by_f32 / 1e6:.0f} MB; uint8 only {t_b8:.3f} ms = {r_u8:.2f} TB/s over "
          f"{by_u8 / 1e6:.0f} MB; device copy of {by_f32 / 1e6:.0f} MB of traffic {t_copy:.3f} ms = {r_copy:.2f} TB/s; fold_blend / copy rate "
          f"{r_f32 / r_copy:.2f}; unfold_tiles {t_unf:.3f} ms", flush=True)
    del stack, src, dst, z
    m._bufs.clear()
    torch.cuda.empty_cache()
