"""Patch-distributed first stage (ddpm.py:567-654, 709-766, 829-866: `split_input_params`): the first stage runs over overlapping crops
of its input and the crop outputs are stitched with border-distance weights.

    out[b, c, Y, X] = ( sum over crops l covering (Y, X):  o[l, b, c, Y - ly*sy, X - lx*sx] * w_tile[y, x] * w_tie[l] )
                      / ( sum over the same crops:  w_tile[y, x] * w_tie[l] )

`TilePlan` holds the host side of it (crop grid, output tile size and strides, the two weight tables, in the reference's operation order)
and refuses the settings on which the reference divides by zero or crashes. `unfold_tiles_cpu` / `fold_blend_cpu` run a plan in plain
torch for tensors that do not live on the GPU; GPU tensors go through ops.unfold_tiles / ops.fold_blend (csrc/tile.hip). Crops are
numbered l = ly*Lx + lx, nn.Unfold's order, and stacked crop-major ([L, B, C, kh, kw]) so that a run of crops is one contiguous first-stage
batch. Any number of covering crops per axis (ceil(k/s)) is allowed.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

# the activation budget of one first-stage call of the tiled path, in latent pixels summed over the call's batch. The shipped VQ-f4 decoder
# addresses its planes with 32-bit element offsets, and its widest plane (the last Upsample's output: 16 image pixels per latent pixel x 256
# channels) reaches 2^31 elements at 32 latents of 128 x 128: a B = 64 decode of 128 x 128 latents is refused by the convolution. Half of
# that limit: 16 latents of 128 x 128, which is also the 64 latents of 64 x 64 the stage is benchmarked at.
CALL_LATENT_PIXELS = 16 * 128 * 128


def _pair(v, what) -> Tuple[int, int]:
    if isinstance(v, (int,)) and not isinstance(v, bool):
        v = (v, v)
    v = tuple(int(a) for a in v)
    if len(v) != 2 or v[0] < 1 or v[1] < 1:
        raise ValueError(f"{what} must be one or two positive integers, got {v}")
    return v


def delta_border(h: int, w: int) -> torch.Tensor:
    """ddpm.py:574-586: distance to the nearest border normalised to [0, 0.5], fp32 [h, w]: the integer grid divided by the integer corner
    (fp32 quotient), then `1 - arr` for the far sides."""
    ys = (torch.arange(0, h).view(h, 1) / torch.tensor(h - 1)).expand(h, w)
    xs = (torch.arange(0, w).view(1, w) / torch.tensor(w - 1)).expand(h, w)
    near = torch.minimum(ys, xs)
    far = torch.minimum(1 - ys, 1 - xs)
    return torch.minimum(near, far).contiguous()


class TilePlan:
    """The crop grid and blend weights of one tiled first-stage call over an input of h x w.

    ks, stride: crop size and step in input pixels (latent pixels for decode, image pixels for encode), an int or a pair. uf / df: the
    first stage's up- (decode) or down-sampling (encode) factor; the output tile is ks*uf or ks//df and the output strides scale alike.
    A ks or stride larger than the input is reduced to the input (ddpm.py:724-730, 837-843)."""

    def __init__(self, h: int, w: int, ks, stride, uf: int = 1, df: int = 1, clip_min_weight: float = 0.01, clip_max_weight: float = 0.5,
                 tie_braker: bool = False, clip_min_tie_weight: float = 0.01, clip_max_tie_weight: float = 0.5):
        h, w, uf, df = int(h), int(w), int(uf), int(df)
        ks, stride = _pair(ks, "ks"), _pair(stride, "stride")
        if h < 1 or w < 1 or uf < 1 or df < 1:
            raise ValueError(f"TilePlan: input {h} x {w}, uf {uf}, df {df} must be positive")
        if ks[0] > h or ks[1] > w:
            ks = (min(ks[0], h), min(ks[1], w))
        if stride[0] > h or stride[1] > w:
            stride = (min(stride[0], h), min(stride[1], w))
        if uf > 1 and df > 1:
            raise NotImplementedError("TilePlan: uf > 1 together with df > 1 (get_fold_unfold, ddpm.py:651-652, raises as well)")
        if (uf != 1 or df != 1) and ks[0] != ks[1]:
            raise ValueError(f"TilePlan: ks {ks} must be square when uf or df is not 1: the reference folds with kernel_size[0] on both sides "
                             "(ddpm.py:629, 642), so a non-square crop is stitched at the wrong size")
        if df > 1 and (ks[0] % df or ks[1] % df or stride[0] % df or stride[1] % df):
            raise ValueError(f"TilePlan: ks {ks} and stride {stride} must be divisible by df = {df}: the output tile and stride are ks // df and "
                             "stride // df, and a remainder shifts every crop after the first")
        for n, k, s, ax in ((h, ks[0], stride[0], "height"), (w, ks[1], stride[1], "width")):
            if s > k and n > k:
                raise ValueError(f"TilePlan: {ax} stride {s} exceeds ks {k}: the {s - k} rows between two crops lie under no crop, so the "
                                 "fold of the weights is 0 there and the normalisation divides 0 by 0")
            if (n - k) % s != 0:
                raise ValueError(f"TilePlan: {ax} {n} with ks {k}, stride {s}: the trailing {(n - k) % s} rows are covered by no crop, so the "
                                 "fold of the weights is 0 there and the normalisation divides 0 by 0")
        self.h, self.w, self.ks, self.stride, self.uf, self.df = h, w, ks, stride, uf, df
        self.Ly, self.Lx = (h - ks[0]) // stride[0] + 1, (w - ks[1]) // stride[1] + 1
        self.L = self.Ly * self.Lx
        if df > 1:
            self.tile, self.out_stride = (ks[0] // df, ks[1] // df), (stride[0] // df, stride[1] // df)
        else:
            self.tile, self.out_stride = (ks[0] * uf, ks[1] * uf), (stride[0] * uf, stride[1] * uf)
        th, tw = self.tile
        if th == 1 or tw == 1:
            raise ValueError(f"TilePlan: output tile {th} x {tw}: delta_border (ddpm.py:581-582) divides by h - 1 = 0 for a side of 1")
        self.tie_braker = bool(tie_braker)
        if self.tie_braker and (self.Ly == 1 or self.Lx == 1):
            raise ValueError(f"TilePlan: tie_braker over a {self.Ly} x {self.Lx} crop grid: delta_border (ddpm.py:581-582) divides by h - 1 = 0 "
                             "for a side of 1")
        self.out_size = ((self.Ly - 1) * self.out_stride[0] + th, (self.Lx - 1) * self.out_stride[1] + tw)
        self.w_tile = torch.clip(delta_border(th, tw), clip_min_weight, clip_max_weight).contiguous()
        if self.tie_braker:
            self.w_tie = torch.clip(delta_border(self.Ly, self.Lx), clip_min_tie_weight, clip_max_tie_weight).reshape(self.L).contiguous()
        else:
            self.w_tie = torch.ones(self.L, dtype=torch.float32)
        self._dev = {}

    @classmethod
    def from_split(cls, split: dict, h: int, w: int, encode: bool) -> "TilePlan":
        """from a `split_input_params` dict (the reference's keys); vqf is uf for decode and df for encode"""
        f = int(split["vqf"])
        kw = {k: split[k] for k in ("clip_min_weight", "clip_max_weight", "tie_braker", "clip_min_tie_weight", "clip_max_tie_weight") if k in split}
        return cls(h, w, split["ks"], split["stride"], uf=1 if encode else f, df=f if encode else 1, **kw)

    def weights(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(w_tile, w_tie) on `device` (copied once per device)"""
        device = torch.device(device)
        if device.type == "cpu":
            return self.w_tile, self.w_tie
        if device not in self._dev:
            self._dev[device] = (self.w_tile.to(device), self.w_tie.to(device))
        return self._dev[device]

    def default_tile_batch(self, batch: int) -> int:
        """crops per first-stage call such that one call stays within CALL_LATENT_PIXELS (at least one crop)"""
        kh, kw = self.ks
        lat = (kh // self.df) * (kw // self.df) if self.df > 1 else kh * kw
        return max(1, min(self.L, CALL_LATENT_PIXELS // max(1, int(batch) * lat)))

    def __repr__(self):
        return (f"TilePlan({self.h}x{self.w}, ks={self.ks}, stride={self.stride}, uf={self.uf}, df={self.df}, crops {self.Ly}x{self.Lx}, "
                f"tile {self.tile}, out {self.out_size}, tie_braker={self.tie_braker})")


def _crop_range(plan: TilePlan, l0: int, nl: Optional[int]) -> Tuple[int, int]:
    nl = plan.L - l0 if nl is None else int(nl)
    if l0 < 0 or nl < 1 or l0 + nl > plan.L:
        raise ValueError(f"crops {l0} .. {l0 + nl - 1} are outside the plan's 0 .. {plan.L - 1}")
    return int(l0), nl


def unfold_tiles_cpu(x: torch.Tensor, plan: TilePlan, l0: int = 0, nl: Optional[int] = None) -> torch.Tensor:
    """crops l0 .. l0+nl-1 of x [B, C, h, w] -> [nl, B, C, kh, kw] (copies)"""
    if x.dim() != 4 or tuple(x.shape[2:]) != (plan.h, plan.w):
        raise ValueError(f"unfold_tiles: x {tuple(x.shape)} does not match the plan's input {plan.h} x {plan.w}")
    l0, nl = _crop_range(plan, l0, nl)
    (kh, kw), (sy, sx) = plan.ks, plan.stride
    out = []
    for l in range(l0, l0 + nl):
        y0, x0 = (l // plan.Lx) * sy, (l % plan.Lx) * sx
        out.append(x[:, :, y0:y0 + kh, x0:x0 + kw])
    return torch.stack(out, 0).contiguous()


def fold_blend_cpu(tiles: torch.Tensor, plan: TilePlan) -> torch.Tensor:
    """tiles [L, B, C, th, tw] -> [B, C, Ho, Wo] per the module docstring, in the tiles' dtype; every pixel sums its crops in ascending l.
    The weight of a crop pixel is the fp32 product w_tile * w_tie[l], as in the reference (get_weighting) and in the kernel."""
    th, tw = plan.tile
    if tiles.dim() != 5 or tiles.shape[0] != plan.L or tuple(tiles.shape[3:]) != (th, tw):
        raise ValueError(f"fold_blend: tiles {tuple(tiles.shape)} do not match the plan's [{plan.L}, B, C, {th}, {tw}]")
    (sy, sx), (Ho, Wo) = plan.out_stride, plan.out_size
    w_tile, w_tie = plan.weights(tiles.device)
    num = torch.zeros(tuple(tiles.shape[1:3]) + (Ho, Wo), dtype=tiles.dtype, device=tiles.device)
    den = torch.zeros((Ho, Wo), dtype=tiles.dtype, device=tiles.device)
    for l in range(plan.L):
        y0, x0 = (l // plan.Lx) * sy, (l % plan.Lx) * sx
        wl = (w_tile * w_tie[l]).to(tiles.dtype)
        num[:, :, y0:y0 + th, x0:x0 + tw] += tiles[l] * wl
        den[y0:y0 + th, x0:x0 + tw] += wl
    return num / den


def image_to_uint8_cpu(x: torch.Tensor) -> torch.Tensor:
    """((clip(x, -1, 1).permute(0, 2, 3, 1) + 1) * 127.5) truncated to uint8 (modules/ldm_diffusion.py:93-95) for CPU tensors"""
    return ((x.float().clamp(-1, 1).permute(0, 2, 3, 1) + 1) * 127.5).to(torch.uint8).contiguous()
