"""Thin torch-tensor front end over the C ABI (include/stedm_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every function below
forwards raw device pointers to libstedm_hip.so and raises on error. No function in this
module computes anything with torch ops."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import BF16, CONV_DOWN, CONV_S1, CONV_S2D, CONV_UP, CONV_UP_SUBPIXEL, F16, STREAM_POSTERIOR, ConvArgs, check, lib


@dataclass(frozen=True)
class Precision:
    """MFMA operand format of the contraction kernels.
    parity: fp16 operands, 3 split products (hi*hi + hi*lo + lo*hi), fp32 accumulate — the mode
            checked against the oracle at 1e-3 (SURVEY.md §7 precision budget).
    fast:   single product (fp16 or bf16 operands), fp32 accumulate / activations / GN / softmax."""
    mm_dtype: int = F16
    npass: int = 3
    attn_fp8: bool = False      # style encoder's attention on e4m3 MFMA operands (BASELINE config 5); everything else as mm_dtype / npass say

    @staticmethod
    def parse(name: str) -> "Precision":
        table = {"parity": Precision(F16, 3), "parity_bf16": Precision(BF16, 3),
                 "fast": Precision(F16, 1), "f16": Precision(F16, 1), "bf16": Precision(BF16, 1),
                 "fp8": Precision(BF16, 1, True), "bf16+fp8attn": Precision(BF16, 1, True)}
        if name not in table:
            raise ValueError(f"unknown precision {name!r}; choose from {sorted(table)}")
        return table[name]

    @property
    def label(self) -> str:
        return ("f16" if self.mm_dtype == F16 else "bf16") + ("x3" if self.npass == 3 else "") + ("+fp8attn" if self.attn_fp8 else "")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype=torch.float32, name="tensor"):
    if not t.is_cuda:
        raise _lib.StedmHipError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def device_cus() -> int:
    return lib().stedm_device_cus()


# ------------------------------------------------------------------------------------------- fp16 operand range guard
# The reference is fp32 (train_diff.py:48). The `f16` / `parity` modes round the residual stream to fp16 operand planes: a value beyond 65 504
# becomes inf there. The kernels that do the rounding flag it (include/stedm_hip.h, stedm_f16_guard_set); the host checks at its own
# synchronisation points and RAISES — a silently wrong sample is the one outcome this must exclude.
_F16_GUARD: dict = {}          # device index -> the 4 flag words (kept for the life of the process: captured graphs hold the address)
F16_GUARD_SITES = {1: "un-normalised operand planes of a 1x1 skip_connection (stedm_gn_apply16c)", 2: "GroupNorm output planes",
                   4: "16-bit side output of a convolution (Upsample operand / qkv planes)", 8: "space-to-depth planes (Downsample operand)",
                   16: "plain fp32 -> fp16 conversion (stedm_gn_apply16 / stedm_gn_chan_stats16)", 32: "fp32-source convolution loader"}


def f16_guard_enable() -> torch.Tensor:
    """Allocate (once per device) and register the guard's flag words for the current device. Not inside a graph capture."""
    dev = torch.cuda.current_device()
    w = _F16_GUARD.get(dev)
    if w is None:
        w = torch.zeros((4,), dtype=torch.int32, device=torch.device("cuda", dev))
        check(lib().stedm_f16_guard_set(w.data_ptr()), "stedm_f16_guard_set")
        _F16_GUARD[dev] = w
    return w


def f16_guard_check(where: str = "") -> None:
    """Read (synchronising) and clear the flag of the current device; raise StedmHipError when an fp16 operand overflowed since the last
    check. A no-op when no fp16-mode model ever enabled the guard on this device."""
    coop_check(where)
    w = _F16_GUARD.get(torch.cuda.current_device()) if torch.cuda.is_available() else None
    if w is None:
        return
    bits = int(w[0].item())
    if bits:
        w.zero_()
        sites = "; ".join(v for k, v in F16_GUARD_SITES.items() if bits & k)
        raise _lib.StedmHipError(
            f"fp16 operand overflow{' in ' + where if where else ''}: a value beyond the fp16 range (|x| > 65504) or a NaN was rounded into "
            f"an MFMA operand plane [{sites}]. The reference computes in fp32; run this checkpoint with precision='bf16', or 'parity_bf16' for the 1e-3 tolerance (fp32 exponent "
            f"range) — the 'f16' and 'parity' modes cannot represent its activations.")


# ------------------------------------------------------------------------------------------- in-launch GroupNorm hand-off (stedm_conv_args.gn_coop)
_COOP: dict = {}               # device index -> [int32[4] per model]: word 0 = the epoch of the model's current forward, word 1 = the give-up flag of the bounded spins


def coop_words_new() -> torch.Tensor:
    """Two device words for the cooperative GroupNorm epilogue of ONE model on the current device (a model's forwards are serial; two models
    may run on two streams). Registered for coop_check(); kept for the life of the process (captured graphs hold the addresses). Not inside a
    graph capture."""
    dev = torch.cuda.current_device()
    w = torch.zeros((4,), dtype=torch.int32, device=torch.device("cuda", dev))
    _COOP.setdefault(dev, []).append(w)
    return w


def coop_check(where: str = "") -> None:
    """Read (synchronising) and clear the give-up flags; raise when a tile stopped waiting for its sample's other tiles (their planes are wrong)."""
    ws = _COOP.get(torch.cuda.current_device(), []) if torch.cuda.is_available() else []
    bad = False
    for w in ws:
        if int(w[1].item()):
            w[1:2].zero_()
            bad = True
    if bad:
        raise _lib.StedmHipError(f"cooperative GroupNorm epilogue{' in ' + where if where else ''}: a tile gave up waiting for the channel sums of its sample's other "
                                 f"tiles (stedm_conv_args.gn_coop); the GroupNorm planes of that launch are invalid. STEDM_NO_GN_COOP=1 runs the separate pass instead.")


# ------------------------------------------------------------------------------------------- weights
# output shape of each pack from (tn = ceil(cout / 128), cout, cin, taps); the layouts are stated in csrc/wfrag.hpp
_PACK_SHAPE = {
    "planes": lambda tn, cout, cin, taps: (cout, taps, cin),
    "up_planes": lambda tn, cout, cin, taps: (4 * cout, 4, cin),
    "frag": lambda tn, cout, cin, taps: (tn, cin // 16, taps, 4, 64, 8),
    "frag16": lambda tn, cout, cin, taps: (tn, cin // 32, taps, 8, 64, 8),
    "frag16_hl": lambda tn, cout, cin, taps: (2, tn, cin // 32, taps, 8, 64, 8),
    "up_frag": lambda tn, cout, cin, taps: (4, tn, cin // 16, 4, 4, 64, 8),
    "up_frag16_hl": lambda tn, cout, cin, taps: (2, 4, tn, cin // 32, 4, 8, 64, 8),
    "s2d_frag": lambda tn, cout, cin, taps: (tn, 4 * cin // 16, 4, 4, 64, 8),
    "s2d_frag16_hl": lambda tn, cout, cin, taps: (2, tn, 4 * cin // 32, 4, 8, 64, 8),
}


def pack_blocks(cout: int, cin: int, m16: bool) -> int:
    """blocks one tensor takes in a stedm_pack_frag_multi table (32 rows x 32 channels in the 16x16x32 order, 64 x 16 in the other)"""
    return ((cout + 127) // 128) * ((cin // 32) * 4 if m16 else (cin // 16) * 2)


def _conv_weight(w: torch.Tensor):
    """OIHW (or [O][I][1] Conv1d) parameter -> (detached contiguous fp32 [O][I][ks][ks] on the GPU, cout, cin, ks)"""
    if w.dim() == 3:
        w = w.unsqueeze(-1)
    w = w.detach().contiguous()
    _chk(w, name="conv weight")
    cout, cin, ks, ks2 = w.shape
    assert ks == ks2
    return w, cout, cin, ks


def _pack_empty(kind: str, w: torch.Tensor, cout: int, cin: int, taps: int) -> torch.Tensor:
    return torch.empty(_PACK_SHAPE[kind]((cout + 127) // 128, cout, cin, taps), dtype=torch.int16, device=w.device)


def _pack(entry: str, kind: str, w: torch.Tensor, cout: int, cin: int, taps: int, args, lo: bool = False):
    """allocate the `kind` output (and a lo twin) and make the checked call lib().<entry>(*args(out pointer, lo pointer or None))"""
    out = _pack_empty(kind, w, cout, cin, taps)
    out_lo = torch.empty_like(out) if lo else None
    check(getattr(lib(), entry)(*args(out.data_ptr(), _ptr(out_lo))), entry)
    return out, out_lo


def pack_conv_weight(w: torch.Tensor, prec: Precision) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """OIHW (or [O][I][1] Conv1d) fp32 -> ([O][taps][I] 16-bit hi, lo or None)."""
    w, cout, cin, ks = _conv_weight(w)
    return _pack("stedm_pack_conv_weight", "planes", w, cout, cin, ks * ks,
                 lambda hi, lo: (w.data_ptr(), hi, lo, cout, cin, ks, prec.mm_dtype, _stream()), lo=prec.npass == 3)


def pack_conv_weight_up(w: torch.Tensor, prec: Precision) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """OIHW 3x3 fp32 -> sub-pixel upsample planes [4*O][4][I] (parity-major), see stedm_pack_conv_weight_up."""
    w, cout, cin, ks = _conv_weight(w)
    assert ks == 3
    return _pack("stedm_pack_conv_weight_up", "up_planes", w, cout, cin, 4,
                 lambda hi, lo: (w.data_ptr(), hi, lo, cout, cin, prec.mm_dtype, _stream()), lo=prec.npass == 3)


def pack_conv_weight_frag(w: torch.Tensor, prec: Precision) -> torch.Tensor:
    """OIHW 3x3 / 1x1 fp32 -> MFMA-fragment-order 16-bit weights (see stedm_pack_conv_weight_frag)."""
    w, cout, cin, ks = _conv_weight(w)
    assert ks in (1, 3) and cin % 16 == 0
    return _pack("stedm_pack_conv_weight_frag", "frag", w, cout, cin, ks * ks,
                 lambda out, _: (w.data_ptr(), out, cout, cin, ks, prec.mm_dtype, _stream()))[0]


def pack_conv_weight_frag16(w: torch.Tensor, prec: Precision, sn: Optional[int] = None, sc: Optional[int] = None, flip: bool = False,
                            cout: Optional[int] = None, cin: Optional[int] = None, ks: Optional[int] = None) -> torch.Tensor:
    """3x3 / 1x1 fp32 filter -> fragment order of the 16x16x32 MFMA kind (stedm_pack_conv_weight_frag16). Default: a plain OIHW filter;
    sn / sc / flip / cout / cin / ks describe a strided source like pack_conv_weight_strided (the dgrad filter of the training step)."""
    if sn is None:
        w, cout, cin, ks = _conv_weight(w)
        assert ks in (1, 3)
        sn, sc = cin * ks * ks, ks * ks
    else:
        w = w.detach()
        _chk(w, name="conv weight")
    assert cin % 32 == 0
    if prec.npass == 3:      # 3-product mode: [2] = the hi stream, then the lo stream
        return _pack("stedm_pack_conv_weight_frag16_hl" if ks == 3 else "stedm_pack_conv_weight_frag16_hl1", "frag16_hl", w, cout, cin, ks * ks,
                     lambda out, _: (w.data_ptr(), sn, sc, int(flip), out, cout, cin, prec.mm_dtype, _stream()))[0]
    return _pack("stedm_pack_conv_weight_frag16", "frag16", w, cout, cin, ks * ks,
                 lambda out, _: (w.data_ptr(), sn, sc, int(flip), out, cout, cin, ks, prec.mm_dtype, _stream()))[0]


def _pack_derived(entry: str, kind: str, w: torch.Tensor, prec: Precision, cin_mod: int, *pad_br) -> torch.Tensor:
    """the 2x2 filters derived from an OIHW 3x3 (sub-pixel upsample, space-to-depth downsample), fragment order"""
    w, cout, cin, ks = _conv_weight(w)
    assert ks == 3 and cin % cin_mod == 0
    return _pack(entry, kind, w, cout, cin, 4, lambda out, _: (w.data_ptr(), out, cout, cin, prec.mm_dtype, *pad_br, _stream()))[0]


def pack_conv_weight_up_frag(w: torch.Tensor, prec: Precision) -> torch.Tensor:
    """OIHW 3x3 fp32 -> fragment-order weights of the sub-pixel upsample form (4 parities x 4 pre-summed taps)."""
    return _pack_derived("stedm_pack_conv_weight_up_frag", "up_frag", w, prec, 32)


def pack_conv_weight_s2d_frag(w: torch.Tensor, prec: Precision, pad_br: bool = False) -> torch.Tensor:
    """OIHW 3x3 fp32 (stride-2 Downsample.op) -> fragment-order weights of the equivalent 2x2 conv over space-to-depth planes.
    pad_br: the conv pads bottom/right only (the VQ encoder's Downsample, model.py:59-76) instead of 1 on every side."""
    return _pack_derived("stedm_pack_conv_weight_s2d_frag", "s2d_frag", w, prec, 8, int(pad_br))


def pack_conv_weight_up_frag16_hl(w: torch.Tensor, prec: Precision) -> torch.Tensor:
    """The sub-pixel upsample filters as hi + lo fragment streams of the 16x16x32 kind (stedm_pack_conv_weight_up_frag16_hl): the 3-product
    modes read both, the single-product modes the hi stream (RS_SUBM, conv_rs.inc)."""
    return _pack_derived("stedm_pack_conv_weight_up_frag16_hl", "up_frag16_hl", w, prec, 32)


def pack_conv_weight_s2d_frag16_hl(w: torch.Tensor, prec: Precision, pad_br: bool = False) -> torch.Tensor:
    """The space-to-depth Downsample filter as hi + lo fragment streams of the 16x16x32 kind (3-product modes: both; single-product: hi)."""
    return _pack_derived("stedm_pack_conv_weight_s2d_frag16_hl", "s2d_frag16_hl", w, prec, 8, int(pad_br))


def space_to_depth16(x: torch.Tensor, out_hi: torch.Tensor, out_lo: Optional[torch.Tensor], prec: Precision) -> None:
    """NHWC fp32 [B,H,W,C] -> 16-bit planes [B,H/2,W/2,4C] (channel block py*2+px = pixel (2y+py, 2x+px))."""
    _chk(x, name="x")
    B, H, W, C = x.shape
    assert tuple(out_hi.shape) == (B, H // 2, W // 2, 4 * C) and out_hi.dtype == torch.int16
    check(lib().stedm_space_to_depth16(x.data_ptr(), C, B, H, W, out_hi.data_ptr(), _ptr(out_lo), prec.mm_dtype, _stream()), "stedm_space_to_depth16")


def transpose(w: torch.Tensor) -> torch.Tensor:
    w = w.detach().contiguous()
    _chk(w, name="matrix")
    rows, cols = w.shape
    out = torch.empty((cols, rows), dtype=torch.float32, device=w.device)
    check(lib().stedm_transpose_f32(w.data_ptr(), out.data_ptr(), rows, cols, _stream()), "stedm_transpose_f32")
    return out


# ------------------------------------------------------------------------------------------- GroupNorm
def gn_scale_shift(x1: torch.Tensor, x2: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                   scale: torch.Tensor, shift: torch.Tensor, groups: int = 32, x2_bmod: int = 0) -> None:
    """x1 [B,H,W,c1] (+ x2 [B|bmod,H,W,c2]) NHWC -> scale/shift [B, c1+c2]."""
    _chk(x1, name="x1")
    B = x1.shape[0]
    HW = x1.numel() // (B * x1.shape[-1])
    c1 = x1.shape[-1]
    c2 = 0
    if x2 is not None:
        _chk(x2, name="x2")
        c2 = x2.shape[-1]
    assert scale.shape == (B, c1 + c2) and shift.shape == (B, c1 + c2)
    check(lib().stedm_gn_scale_shift(x1.data_ptr(), c1, _ptr(x2), c2, x2_bmod, gamma.data_ptr(), beta.data_ptr(),
                                     float(eps), groups, B, HW, scale.data_ptr(), shift.data_ptr(), _stream()),
          "stedm_gn_scale_shift")


def gn_nslab(C: int, HW: int) -> int:
    return lib().stedm_gn_nslab(C, HW)


def gn_stats(x1: torch.Tensor, x2: Optional[torch.Tensor], stats: torch.Tensor, groups: int = 32, x2_bmod: int = 0) -> None:
    """Per-slab {sum, sumsq} of the virtual concat [x1|x2] into stats (float64, >= B*gn_nslab(C,HW)*groups*2 elements)."""
    _chk(x1, name="x1")
    _chk(stats, torch.float64, "stats")
    B = x1.shape[0]
    HW = x1.numel() // (B * x1.shape[-1])
    c2 = 0 if x2 is None else x2.shape[-1]
    assert stats.numel() >= B * gn_nslab(x1.shape[-1] + c2, HW) * groups * 2
    check(lib().stedm_gn_stats(x1.data_ptr(), x1.shape[-1], _ptr(x2), c2, x2_bmod, groups, B, HW, stats.data_ptr(), _stream()),
          "stedm_gn_stats")


def gn_apply16(x1: torch.Tensor, x2: Optional[torch.Tensor], out_hi: torch.Tensor, out_lo: Optional[torch.Tensor], prec: Precision,
               gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, eps: float = 1e-5, groups: int = 32,
               act: int = 0, stats: Optional[torch.Tensor] = None, x2_bmod: int = 0) -> None:
    """y = act(GroupNorm([x1|x2])) (or plain conversion when gamma is None) -> 16-bit NHWC planes out_hi (/out_lo)."""
    _chk(x1, name="x1")
    B = x1.shape[0]
    HW = x1.numel() // (B * x1.shape[-1])
    c2 = 0 if x2 is None else x2.shape[-1]
    check(lib().stedm_gn_apply16(x1.data_ptr(), x1.shape[-1], _ptr(x2), c2, x2_bmod, _ptr(gamma), _ptr(beta), float(eps), groups,
                                 act, _ptr(stats), B, HW, out_hi.data_ptr(), _ptr(out_lo), prec.mm_dtype, _stream()),
          "stedm_gn_apply16")


def gn_chan_nslab(HW: int) -> int:
    return (HW + 255) // 256


def gn_chan_stats(x: torch.Tensor, out: torch.Tensor) -> None:
    """Per-(sample, slot, channel) {sum, sumsq} of an NHWC fp32 tensor -> out [B][nslab][C][2] fp32 (any nslab: the sample's
    pixels are cut into nslab runs)."""
    _chk(x, name="x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    assert out.dtype == torch.float32 and out.dim() == 4 and out.shape[0] == B and tuple(out.shape[2:]) == (C, 2)
    check(lib().stedm_gn_chan_stats(x.data_ptr(), C, B, HW, out.shape[1], out.data_ptr(), _stream()), "stedm_gn_chan_stats")


def gn_chan_stats16(x: torch.Tensor, out: torch.Tensor, out_hi: torch.Tensor, out_lo: Optional[torch.Tensor], prec: Precision) -> None:
    """gn_chan_stats + the plain 16-bit conversion of x (hi / lo planes of x's shape) from the same read."""
    _chk(x, name="x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    assert out.dtype == torch.float32 and out.dim() == 4 and out.shape[0] == B and tuple(out.shape[2:]) == (C, 2)
    assert out_hi.numel() == x.numel() and out_hi.element_size() == 2 and (out_lo is None or out_lo.numel() == x.numel())
    check(lib().stedm_gn_chan_stats16(x.data_ptr(), C, B, HW, out.shape[1], out.data_ptr(), out_hi.data_ptr(), _ptr(out_lo), prec.mm_dtype,
                                      _stream()), "stedm_gn_chan_stats16")


def gn_apply16c(x1: torch.Tensor, cs1: torch.Tensor, x2: Optional[torch.Tensor], cs2: Optional[torch.Tensor], out_hi: torch.Tensor,
                out_lo: Optional[torch.Tensor], prec: Precision, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                groups: int = 32, act: int = 0, x2_bmod: int = 0, raw: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None,
                mean_rstd: Optional[torch.Tensor] = None) -> None:
    """act(GroupNorm([x1|x2])) from channel partials -> 16-bit planes (+ optional plain conversion planes `raw`; + optional
    mean_rstd [B][groups][2] fp32, the group statistics the pass folds, kept for the training backward)."""
    _chk(x1, name="x1")
    B = x1.shape[0]
    HW = x1.numel() // (B * x1.shape[-1])
    c2 = 0 if x2 is None else x2.shape[-1]
    if mean_rstd is not None:
        assert mean_rstd.dtype == torch.float32 and mean_rstd.is_contiguous() and tuple(mean_rstd.shape) == (B, groups, 2)
    check(lib().stedm_gn_apply16c_mr(x1.data_ptr(), x1.shape[-1], cs1.data_ptr(), cs1.shape[1], _ptr(x2), c2, _ptr(cs2),
                                     0 if cs2 is None else cs2.shape[1], x2_bmod, gamma.data_ptr(),
                                     beta.data_ptr(), float(eps), groups, act, B, HW, out_hi.data_ptr(), _ptr(out_lo),
                                     None if raw is None else raw[0].data_ptr(), None if raw is None else _ptr(raw[1]),
                                     _ptr(mean_rstd), prec.mm_dtype, _stream()), "stedm_gn_apply16c_mr")


def gn_apply16c_film(x1: torch.Tensor, cs1: torch.Tensor, out_hi: torch.Tensor, out_lo: Optional[torch.Tensor], prec: Precision, gamma: torch.Tensor,
                     beta: torch.Tensor, film: torch.Tensor, film_off: int, film_bstride: int, eps: float = 1e-5, groups: int = 32, act: int = 0,
                     raw: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None, mean_rstd: Optional[torch.Tensor] = None) -> None:
    """act(GroupNorm(x1) * (1 + scale) + shift) -> 16-bit planes (stedm_gn_apply16c_film): sample b reads scale / shift at
    film.view(-1)[b * film_bstride + film_off + (0 | C) + c]; film_bstride 0 shares one row."""
    _chk(x1, name="x1"); _chk(film, name="film")
    B, C = x1.shape[0], x1.shape[-1]
    HW = x1.numel() // (B * C)
    assert film_off >= 0 and film.numel() >= (B - 1) * film_bstride + film_off + 2 * C, "film rows out of range"
    if mean_rstd is not None:
        assert mean_rstd.dtype == torch.float32 and mean_rstd.is_contiguous() and tuple(mean_rstd.shape) == (B, groups, 2)
    check(lib().stedm_gn_apply16c_film(x1.data_ptr(), C, cs1.data_ptr(), cs1.shape[1], None, 0, None, 0, 0, gamma.data_ptr(), beta.data_ptr(),
                                       float(eps), groups, act, B, HW, out_hi.data_ptr(), _ptr(out_lo),
                                       None if raw is None else raw[0].data_ptr(), None if raw is None else _ptr(raw[1]), _ptr(mean_rstd),
                                       film.data_ptr(), int(film_bstride), int(film_off), prec.mm_dtype, _stream()), "stedm_gn_apply16c_film")


def _drop_tail(drop):
    """(p, seed, site, step, step_ptr) of a ResBlock dropout site as the five trailing C arguments; step_ptr: int32[1] device tensor or None"""
    p, seed, site, step, step_ptr = drop
    if step_ptr is not None:
        assert step_ptr.is_cuda and step_ptr.dtype == torch.int32 and step_ptr.numel() >= 1
    return float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(site) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, _ptr(step_ptr)


def gn_apply16c_drop(x1: torch.Tensor, cs1: torch.Tensor, out_hi: torch.Tensor, out_lo: Optional[torch.Tensor], prec: Precision, gamma: torch.Tensor,
                     beta: torch.Tensor, drop, eps: float = 1e-5, groups: int = 32, act: int = 0, mean_rstd: Optional[torch.Tensor] = None,
                     film: Optional[torch.Tensor] = None, film_off: int = 0, film_bstride: int = 0) -> None:
    """Dropout(act(GroupNorm(x1) [* (1 + scale) + shift])) -> 16-bit planes (stedm_gn_apply16c_drop; with `film` stedm_gn_apply16c_film_drop).
    drop = (p, seed, site, step, step_ptr): the mask stream of include/stedm_hip.h ("train-mode dropout", ResBlock sites); the kernel uses
    step + step_ptr[0] (step_ptr: device int32[1] or None)."""
    _chk(x1, name="x1")
    B, C = x1.shape[0], x1.shape[-1]
    HW = x1.numel() // (B * C)
    if mean_rstd is not None:
        assert mean_rstd.dtype == torch.float32 and mean_rstd.is_contiguous() and tuple(mean_rstd.shape) == (B, groups, 2)
    head = (x1.data_ptr(), C, cs1.data_ptr(), cs1.shape[1], None, 0, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), float(eps), groups, act, B, HW,
            out_hi.data_ptr(), _ptr(out_lo), None, None, _ptr(mean_rstd))
    if film is None:
        check(lib().stedm_gn_apply16c_drop(*head, prec.mm_dtype, *_drop_tail(drop), _stream()), "stedm_gn_apply16c_drop")
    else:
        _chk(film, name="film")
        assert film_off >= 0 and film.numel() >= (B - 1) * film_bstride + film_off + 2 * C, "film rows out of range"
        check(lib().stedm_gn_apply16c_film_drop(*head, film.data_ptr(), int(film_bstride), int(film_off), prec.mm_dtype, *_drop_tail(drop), _stream()),
              "stedm_gn_apply16c_film_drop")


def gn_apply16c_x16(c1: int, cs1: torch.Tensor, x2: Optional[torch.Tensor], cs2: Optional[torch.Tensor], out_hi: torch.Tensor, raw_hi: torch.Tensor,
                    prec: Precision, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, groups: int = 32, act: int = 0, x2_bmod: int = 0) -> None:
    """act(GroupNorm([x1|x2])) where x1 (c1 channels) already sits as 16-bit values in channels [0, c1) of raw_hi [B,H,W,c1+c2] (written there by
    the producing convolution: conv_igemm(out=None, out16=..., out16_stride=c1+c2)); x2 fp32 as in gn_apply16c. out_hi receives the
    normalised planes, raw_hi the plain conversion of x2. Single-product modes (stedm_gn_apply16c_x16)."""
    assert prec.npass == 1 and raw_hi.dtype == torch.int16 and out_hi.dtype == torch.int16 and raw_hi.is_contiguous() and out_hi.is_contiguous()
    B, C = raw_hi.shape[0], raw_hi.shape[-1]
    HW = raw_hi.numel() // (B * C)
    c2 = 0 if x2 is None else x2.shape[-1]
    assert C == c1 + c2 and tuple(out_hi.shape) == tuple(raw_hi.shape)
    check(lib().stedm_gn_apply16c_x16(int(c1), cs1.data_ptr(), cs1.shape[1], _ptr(x2), c2, _ptr(cs2), 0 if cs2 is None else cs2.shape[1], x2_bmod,
                                      gamma.data_ptr(), beta.data_ptr(), float(eps), groups, act, B, HW, out_hi.data_ptr(), raw_hi.data_ptr(),
                                      prec.mm_dtype, _stream()), "stedm_gn_apply16c_x16")


def gn_apply16c_x16_ok(c1: int, c2: int, groups: int = 32) -> bool:
    C = c1 + c2
    return C % 8 == 0 and c1 % 8 == 0 and c1 > 0 and 3 * C * 4 <= 48 * 1024 and 0 < groups <= 64 and C % groups == 0


# ------------------------------------------------------------------------------------------- conv
class LazyPlanes:
    """[cout][tap][cin] hi (/lo) weight planes packed on first need. The register-streamed kernel reads only the fragment-order
    weights; the planes are packed when a problem falls to the LDS-operand kernels (asked through stedm_conv_rs_ok)."""

    def __init__(self, fn):
        self._fn, self._val = fn, None

    def get(self):
        if self._val is None:
            self._val = self._fn()
        return self._val

    def reset(self):
        """the source weights changed: pack again on the next need"""
        self._val = None


class PackPlan:
    """The fragment-order weight packs of a module set, recorded as they first happen and re-run later as ONE launch
    (stedm_pack_frag_multi) into the same output tensors: after an optimizer step every convolution's packs are stale, and ~130 separate
    packs of a few microseconds each are launch-bound. Valid while the source tensors keep their storage (the caller keys on data_ptr)."""

    def __init__(self, prec: Precision):
        self.prec = prec
        self.items = []          # (w tensor (kept alive), sn, sc, flip, cout, cin, taps, m16, out)
        self._table = None
        self._blocks = 0
        self._fused = frozenset()      # indices of items the optimizer kernel refreshes itself (stedm_adamw_ema_pack)
        self._rest = None              # (table, blocks, n) of the other items
        self._fresh = None             # parameter versions at the moment the fused items were last refreshed

    def frag(self, w: torch.Tensor, sn: int, sc: int, flip: bool, cout: int, cin: int, ks: int, m16: bool) -> torch.Tensor:
        """Pack now (single-tensor launch) and remember the problem. w: fp32 tensor whose element (n, ci, tap) is flat[n*sn + ci*sc + tap']."""
        if m16:
            assert self.prec.npass == 1        # stedm_pack_frag_multi writes one stream: no hi + lo form of this order here
            out = pack_conv_weight_frag16(w, self.prec, sn, sc, flip, cout, cin, ks)
        else:
            out = pack_conv_weight_strided(w, sn, sc, flip, cout, cin, ks, self.prec, want_hi=False, want_frag=True)[2]
        self.items.append((w, sn, sc, int(flip), cout, cin, ks * ks, int(m16), out))
        self._table = None
        self._rest = None
        self._fresh = None
        return out

    def frag_oihw(self, w4: torch.Tensor, m16: bool) -> torch.Tensor:
        """plain OIHW filter [cout, cin, ks, ks]"""
        cout, cin, ks, _ = w4.shape
        return self.frag(w4, cin * ks * ks, ks * ks, False, cout, cin, ks, m16)

    def _build_table(self, idxs):
        import struct
        rec, blk = [], 0
        for i in idxs:
            (w, sn, sc, flip, cout, cin, taps, m16, out) = self.items[i]
            rec.append(struct.pack("<QQqqiiiiii", w.data_ptr(), out.data_ptr(), sn, sc, cout, cin, taps, flip, m16, blk))
            blk += pack_blocks(cout, cin, m16)
        if not rec:
            return None, 0, 0
        return torch.frombuffer(bytearray(b"".join(rec)), dtype=torch.uint8).to(self.items[0][0].device), blk, len(rec)

    def set_fused(self, idxs) -> None:
        """items the optimizer kernel refreshes itself; run(versions) skips them while mark_fresh(versions) still holds"""
        self._fused = frozenset(idxs)
        self._rest = None
        self._fresh = None

    def mark_fresh(self, versions) -> None:
        self._fresh = versions

    def run(self, versions=None) -> None:
        """all recorded packs again, one launch. versions: the parameters' `_version`s now — when they are the ones mark_fresh() saw, the
        fused items already hold the current weights (written by the optimizer kernel) and only the others run"""
        if not self.items:
            return
        fresh, self._fresh = self._fresh, None
        if self._fused and versions is not None and fresh == versions:
            if self._rest is None:
                self._rest = self._build_table([i for i in range(len(self.items)) if i not in self._fused])
            table, blocks, n = self._rest
            if n:
                check(lib().stedm_pack_frag_multi(table.data_ptr(), n, blocks, self.prec.mm_dtype, _stream()), "stedm_pack_frag_multi")
            return
        if self._table is None:
            self._table, self._blocks, _ = self._build_table(range(len(self.items)))
        check(lib().stedm_pack_frag_multi(self._table.data_ptr(), len(self.items), self._blocks, self.prec.mm_dtype, _stream()), "stedm_pack_frag_multi")


def conv3x3_tiles_ok(Hout: int, Wout: int) -> bool:
    """Do the tiled 3x3 kernels have a tiling for this output grid (stedm_conv3x3_tiles_ok)? Otherwise conv_igemm takes the im2col form."""
    return bool(lib().stedm_conv3x3_tiles_ok(int(Hout), int(Wout)))


_GENERIC_COLS: dict = {}      # (device, shape) -> im2col planes of the generic-shape path (reused: one convolution at a time on a stream)


def _conv3x3_generic(src16, w_hi, w_lo, out, *, prec: Precision, mode: int, **kw):
    """A 3x3 convolution on an output grid the tiled kernels cannot tile (latent widths that are not powers of two): row-major im2col of the
    16-bit planes (stedm_im2col_rows16) + the 1x1 kind over K = 9 C with the ordinary [cout][tap][cin] weight planes. Same epilogues
    (bias / embedding / residual / statistics / the riding GroupNorm), 9x the activation bytes: a correctness path, not a fast one."""
    assert kw.get("skip") is None, "the fused skip phase belongs to the tiled kernels (stedm_conv_fused_skip_ok says so)"
    B, H, W, C = src16[0].shape
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if mode == CONV_DOWN else ((2 * H, 2 * W) if mode == CONV_UP else (H, W))
    cols = []
    for i, pl in enumerate(src16):
        if pl is None or (i == 1 and prec.npass != 3):
            cols.append(None)
            continue
        key = (pl.device, i, B, Ho, Wo, 9 * C)
        col = _GENERIC_COLS.get(key)
        if col is None:
            if len(_GENERIC_COLS) > 16:
                _GENERIC_COLS.clear()
            col = _GENERIC_COLS[key] = torch.empty((B, Ho, Wo, 9 * C), dtype=torch.int16, device=pl.device)
        check(lib().stedm_im2col_rows16(pl.data_ptr(), col.data_ptr(), B, H, W, C, {CONV_S1: 0, CONV_DOWN: 1, CONV_UP: 2}[mode], _stream()),
              "stedm_im2col_rows16")
        cols.append(col)
    if isinstance(w_hi, LazyPlanes):
        w_hi, w_lo = w_hi.get()
    cout = w_hi.shape[0]
    assert tuple(w_hi.shape) == (cout, 9, C), (tuple(w_hi.shape), cout, C)
    for k in ("w_frag", "w_frag16", "ks", "out16_stride", "cout"):
        kw.pop(k, None)
    return conv_igemm(None, w_hi.view(cout, 1, 9 * C), None if w_lo is None else w_lo.view(cout, 1, 9 * C), out, prec=prec, ks=1, mode=CONV_S1,
                      src16=(cols[0], cols[1]), **kw)


def conv_igemm(src1: Optional[torch.Tensor], w_hi: torch.Tensor, w_lo: Optional[torch.Tensor], out: torch.Tensor, *, prec: Precision,
               ks: int = 3, mode: int = CONV_S1, src2: Optional[torch.Tensor] = None, src2_bmod: int = 0,
               scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, act: int = 0,
               bias: Optional[torch.Tensor] = None, emb: Optional[torch.Tensor] = None, emb_offset: int = 0,
               emb_bstride: int = 0, res: Optional[torch.Tensor] = None,
               src16: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None, act_out: int = 0,
               out16: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None, w_frag: Optional[torch.Tensor] = None,
               chan_stats: Optional[torch.Tensor] = None,
               skip: Optional[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = None, query_fused: bool = False, query_rs: bool = False,
               ws: Optional[torch.Tensor] = None, pad_br: bool = False, w_frag16: Optional[torch.Tensor] = None,
               gn_next: Optional[tuple] = None, qkv_planes: Optional[tuple] = None, ln_after: Optional[tuple] = None, coop: Optional[tuple] = None,
               out16_stride: int = 0, cout: Optional[int] = None, res_bmod: int = 0, res2: Optional[torch.Tensor] = None, partials: bool = False):
    """src1 [B,Hin,Win,c1] NHWC fp32 (fused path) and/or src16 = (hi, lo) 16-bit NHWC planes [B,Hin,Win,Cin] from
    gn_apply16 (DMA path) -> out [B,Hout,Wout,cout] NHWC fp32 (see stedm_conv_igemm).
    src16[0] may be a channel-narrowed (and batch-narrowed) view plane[b0:b1, :, :, k0:k1] of a contiguous plane: a K window
    (stedm_conv_args.src16_cstride / k_chan0 / w_cin) - the convolution sums channels [k0, k1) only, against the matching chunks of the
    fragment pack of the full filter. res_bmod: output sample b adds the residual rows of sample b % res_bmod (stedm_conv_args.res_bmod);
    res2: a second residual, added as res + res2 (stedm_conv_args.res2).
    partials=True (stedm_conv_partials): the first half of a split-K call - the K-share partials stay in `ws` as [nshare][B][H][W][cout] raw sums,
    no reduce pass runs, `out` only names the shape; returns nshare (1: the dispatcher did not split). With query_rs: the share count the
    call would leave, or 0 when it would not run. conv_finish is the second half.
    qkv_planes = (q, k, vt, T, Tp, heads, qscale): the LSA attention's operand planes as the only output of a flat to_qkv GEMM
    (stedm_conv_args.qkv_*; out and out16 None).
    ln_after = (gamma, beta, eps, res): LayerNorm over the output row (cout <= 128) + optional fp32 residual in the epilogue
    (stedm_conv_args.ln_*): out / out16 receive LayerNorm(conv + bias) + res."""
    if src16 is not None and src1 is None and ks == 3 and mode in (CONV_S1, CONV_DOWN, CONV_UP) and not out16_stride:
        _, H_, W_, _ = src16[0].shape
        Ho_, Wo_ = ((H_ - 1) // 2 + 1, (W_ - 1) // 2 + 1) if mode == CONV_DOWN else ((2 * H_, 2 * W_) if mode == CONV_UP else (H_, W_))
        if not conv3x3_tiles_ok(Ho_, Wo_):
            if query_fused or query_rs:
                return False
            if not src16[0].is_contiguous() or res_bmod or res2 is not None or partials:
                raise _lib.StedmHipError("conv_igemm: a K window / res_bmod belongs to the tiled register-streamed kernel; this output grid takes the im2col form")
            return _conv3x3_generic(src16, w_hi, w_lo, out, prec=prec, mode=mode, scale=scale, shift=shift, act=act, bias=bias, emb=emb,
                                    emb_offset=emb_offset, emb_bstride=emb_bstride, res=res, act_out=act_out, out16=out16, chan_stats=chan_stats,
                                    skip=skip, ws=ws, gn_next=gn_next)
    if out is not None:
        _chk(out, name="out")
    a = ConvArgs()
    a.act_out = act_out
    if gn_next is not None:
        # (gamma, beta, eps, groups, act, out16): the GroupNorm (+ SiLU) reading `out`, written as 16-bit planes by the same call
        g_w, g_b, g_eps, g_groups, g_act, g_out = gn_next[:6]
        g_lo = None
        if isinstance(g_out, (tuple, list)):      # (hi, lo): the 3-product modes' planes
            g_out, g_lo = g_out[0], g_out[1]
        g_mr = gn_next[6] if len(gn_next) > 6 else None
        a.gn_only = int(bool(gn_next[7])) if len(gn_next) > 7 else 0
        if g_mr is not None:
            _chk(g_mr, name="gn mean_rstd")
            assert tuple(g_mr.shape) == (out.shape[0], int(g_groups), 2)
            a.gn_mr = g_mr.data_ptr()
        _chk(g_w, name="gn gamma"); _chk(g_b, name="gn beta")
        assert g_out.dtype == torch.int16 and g_out.is_contiguous() and tuple(g_out.shape) == tuple(out.shape) and chan_stats is not None
        # the convolution's own epilogue may write these planes while other tiles still gather their input: never the planes it reads
        assert src16 is None or all(t is None or t.data_ptr() != g_out.data_ptr() for t in src16), "gn_next planes alias the convolution's input planes"
        a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_groups, a.gn_act, a.gn_out16 = g_w.data_ptr(), g_b.data_ptr(), float(g_eps), int(g_groups), int(g_act), g_out.data_ptr()
        if g_lo is not None:
            assert g_lo.dtype == torch.int16 and g_lo.is_contiguous() and tuple(g_lo.shape) == tuple(out.shape)
            assert src16 is None or all(t is None or t.data_ptr() != g_lo.data_ptr() for t in src16), "gn_next lo planes alias the convolution's input planes"
            a.gn_out16_lo = g_lo.data_ptr()
        assert prec.npass == 1 or g_lo is not None, "gn_next in a 3-product mode needs the (hi, lo) planes"
        if coop is not None:       # (words, state): [B][4][128][2] int64 words of this call site (zero before first use) + the model's coop_words_new()
            cwd, cw = coop
            assert cwd.dtype == torch.int64 and cwd.is_contiguous() and tuple(cwd.shape) == (out.shape[0], 4, 128, 2)
            assert cw.dtype == torch.int32 and cw.numel() >= 2
            a.gn_coop, a.gn_coop_epoch, a.gn_coop_tmo = cwd.data_ptr(), cw.data_ptr(), cw.data_ptr() + 4
    a.pad_br = int(pad_br)
    a.w_frag16 = _ptr(w_frag16)      # npass 3: the hi + lo streams of pack_conv_weight_frag16 in that mode
    a.w_frag = _ptr(w_frag) if prec.npass == 1 else None
    a.chan_stats = _ptr(chan_stats)
    a.chan_nslab = 0 if chan_stats is None else chan_stats.shape[1]
    if ws is not None:   # fp32 workspace for the split-K form of small grids
        a.ws = ws.data_ptr()
        a.ws_floats = ws.numel()
    if skip is not None:   # fused skip_connection: (raw 16-bit planes of the block input, 1x1 weights in fragment order, bias)
        a.src16b_hi = skip[0].data_ptr()
        a.cb = skip[0].shape[-1]
        a.w_frag_b = skip[1].data_ptr()
        a.bias_b = _ptr(skip[2])
        a.w_frag_b16 = _ptr(skip[3]) if len(skip) > 3 and prec.npass == 1 else None
    if out16 is not None:
        a.out16_hi = out16[0].data_ptr()
        a.out16_lo = _ptr(out16[1]) if prec.npass == 3 else None
        if out16_stride:
            # the 16-bit output goes into channels [0, cout) of a wider plane (stedm_conv_args.out16_stride): `cout` names the convolution's width
            assert cout is not None and out is None and prec.npass == 1 and out16[0].shape[-1] == out16_stride and out16[0].is_contiguous()
            a.out16_stride = int(out16_stride)
    if ln_after is not None:
        l_g, l_b, l_eps, l_res = ln_after
        _chk(l_g, name="ln gamma"); _chk(l_b, name="ln beta")
        assert res is None and prec.npass == 1 and (out is not None or out16 is not None)
        a.ln_gamma, a.ln_beta, a.ln_eps = l_g.data_ptr(), l_b.data_ptr(), float(l_eps)
        if l_res is not None:
            _chk(l_res, name="ln residual")
            a.ln_res = l_res.data_ptr()
    if qkv_planes is not None:
        qq, qk, qv, qT, qTp, qH, qs = qkv_planes
        assert out is None and out16 is None and prec.npass == 1 and src16 is not None
        nb = src16[0].shape[2] // int(qT)
        for t_, shp in ((qq, (nb * qH, qTp, 64)), (qk, (nb * qH, qTp, 64)), (qv, (nb * qH, 64, qTp))):
            assert t_.dtype == torch.int16 and t_.is_contiguous() and tuple(t_.shape) == shp, (tuple(t_.shape), shp)
        a.qkv_q, a.qkv_k, a.qkv_vt = qq.data_ptr(), qk.data_ptr(), qv.data_ptr()
        a.qkv_T, a.qkv_Tp, a.qkv_heads, a.qkv_qscale = int(qT), int(qTp), int(qH), float(qs)
        oshape = (1, 1, src16[0].shape[2], 3 * int(qH) * 64)
    else:
        oshape = out.shape if out is not None else out16[0].shape
        if cout is not None:
            oshape = tuple(oshape[:-1]) + (int(cout),)
    if src1 is not None:
        _chk(src1, name="src1")
        B, Hin, Win, c1 = src1.shape
        a.src1 = src1.data_ptr()
        a.src2 = _ptr(src2)
        c2 = 0 if src2 is None else src2.shape[-1]
    else:
        B, Hin, Win, c1 = src16[0].shape
        c2 = 0
    kwin = False
    if src16 is not None:
        s16 = src16[0]
        assert s16.dtype == torch.int16 and tuple(s16.shape) == (B, Hin, Win, c1 + c2)
        a.src16_hi = s16.data_ptr()
        a.src16_lo = _ptr(src16[1]) if prec.npass == 3 else None
        if not s16.is_contiguous():
            # a K window: channels [k0, k0 + c1) of a plane whose pixel rows hold cs elements (both from the view's strides / storage offset)
            cs = s16.stride(2)
            base = s16._base if s16._base is not None else s16
            k0 = (s16.storage_offset() - base.storage_offset()) % cs
            assert src1 is None and tuple(s16.stride()) == (Hin * Win * cs, Win * cs, cs, 1) and k0 + c1 <= cs, \
                "src16[0] must be contiguous or a view plane[b0:b1, :, :, k0:k1] of a contiguous plane"
            assert cs % 32 == 0 and k0 % 32 == 0 and c1 % 32 == 0, "a K window is cut on 32-channel boundaries"
            kwin = True
            a.src16_hi = s16.data_ptr() - 2 * k0          # channel 0 of the view's first pixel row: the kernel walks from k_chan0
            if a.src16_lo is not None:
                assert tuple(src16[1].stride()) == tuple(s16.stride()) and src16[1].storage_offset() == s16.storage_offset()
                a.src16_lo = src16[1].data_ptr() - 2 * k0
            a.src16_cstride, a.k_chan0 = cs, k0
            # input channels of the pack: [.., N-tiles, chunks, taps, fragments, 64, 8] with chunks of 16 (w_frag) or 32 (w_frag16) channels
            wplanes = w_hi._val[0] if isinstance(w_hi, LazyPlanes) and w_hi._val is not None else (None if isinstance(w_hi, LazyPlanes) else w_hi)
            a.w_cin = (w_frag.shape[-5] * 16 if w_frag is not None and prec.npass == 1 else
                       w_frag16.shape[-5] * 32 if w_frag16 is not None else wplanes.shape[-1] if wplanes is not None else cs)
            assert w_frag is None or w_frag16 is None or w_frag.shape[-5] * 16 == w_frag16.shape[-5] * 32
    a.res_bmod = int(res_bmod)
    if res_bmod:
        assert res is not None and res.is_contiguous() and res.dtype == torch.float32 and B % res_bmod == 0 and res.shape[0] >= res_bmod
    if res2 is not None:
        assert res is not None and res2.is_contiguous() and res2.dtype == torch.float32 and tuple(res2.shape) == tuple(res.shape)
        a.res2 = res2.data_ptr()
    a.c1, a.c2, a.src2_bmod = c1, c2, src2_bmod
    a.B, a.Hin, a.Win = B, Hin, Win
    a.mode, a.ks = mode, ks
    a.scale, a.shift, a.act = _ptr(scale), _ptr(shift), act
    lazy = w_hi if isinstance(w_hi, LazyPlanes) else None
    if lazy is not None:
        w_hi, w_lo = lazy._val if lazy._val is not None else (w_frag if w_frag is not None else w_frag16, None)   # placeholder pointer until the planes are known to be needed
    a.w_hi, a.w_lo = _ptr(w_hi), (_ptr(w_lo) if prec.npass == 3 else None)
    a.bias = _ptr(bias)
    a.emb = None if emb is None else emb.data_ptr() + 4 * emb_offset
    a.emb_bstride = emb_bstride
    a.res = _ptr(res)
    a.out = _ptr(out)
    a.cout = oshape[-1]
    a.npass, a.mm_dtype = prec.npass, prec.mm_dtype
    if lazy is not None and lazy._val is None:
        if src16 is None or (w_frag is None and w_frag16 is None) or prec.npass != 1 or not lib().stedm_conv_rs_ok(C.byref(a)):
            w_hi, w_lo = lazy.get()
            a.w_hi, a.w_lo = _ptr(w_hi), (_ptr(w_lo) if prec.npass == 3 else None)
    elif mode == CONV_UP_SUBPIXEL:
        assert w_hi.shape == (4 * a.cout, 4, a.c1 + a.c2), (w_hi.shape, a.cout, a.c1, a.c2)
    elif mode == CONV_S2D:
        assert w_hi is None and (w_frag is not None or w_frag16 is not None) and src1 is None, \
            "the space-to-depth form runs on the register-streamed kernel only"
    else:
        assert w_hi.shape == (a.cout, ks * ks, a.w_cin if kwin else a.c1 + a.c2), (w_hi.shape, a.cout, ks, a.c1, a.c2)
    if partials:
        assert ws is not None and not query_fused
        n = C.c_int32(0)
        rc = lib().stedm_conv_partials(C.byref(a), C.byref(n), int(bool(query_rs)), _stream())
        if query_rs:
            return int(n.value) if rc == 0 else 0
        check(rc, "stedm_conv_partials")
        return int(n.value)
    if query_fused:     # capability query only: would this (fused) problem run as one kernel?
        return bool(lib().stedm_conv_fused_skip_ok(C.byref(a)))
    if query_rs:        # capability query only: would the register-streamed kernel run this problem?
        return bool(lib().stedm_conv_rs_ok(C.byref(a)))
    check(lib().stedm_conv_igemm(C.byref(a), _stream()), "stedm_conv_igemm")
    return out


def conv_finish(ws: torch.Tensor, nshare: int, out: Optional[torch.Tensor], *, prec: Precision, ws_bmod: int = 0, bias: Optional[torch.Tensor] = None,
                emb: Optional[torch.Tensor] = None, emb_offset: int = 0, emb_bstride: int = 0, res: Optional[torch.Tensor] = None,
                res2: Optional[torch.Tensor] = None, res_bmod: int = 0, chan_stats: Optional[torch.Tensor] = None,
                out16: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None, out16_stride: int = 0, cout: Optional[int] = None,
                gn_next: Optional[tuple] = None):
    """The second half of a split-K call on its own (stedm_conv_finish): out [B,H,W,cout] = sum of the `nshare` partial planes that
    conv_igemm(partials=True) left in `ws` at batch ws_bmod (0: B; output sample b sums the rows of sample b % ws_bmod) + (bias + emb row of
    sample b) + residual, with chan_stats, out16 and the riding GroupNorm gn_next as in conv_igemm."""
    shape = tuple(out.shape) if out is not None else tuple(out16[0].shape[:-1]) + (int(cout),)
    B, H, W, co = shape
    a = ConvArgs()
    _chk(ws, name="ws")
    a.ws, a.ws_floats, a.ws_bmod = ws.data_ptr(), ws.numel(), int(ws_bmod)
    a.B, a.Hin, a.Win, a.cout = B, H, W, co
    a.mode, a.ks, a.npass, a.mm_dtype = CONV_S1, 3, prec.npass, prec.mm_dtype
    if out is not None:
        _chk(out, name="out")
        a.out = out.data_ptr()
    a.bias = _ptr(bias)
    if bias is not None:
        assert bias.numel() == co
    if emb is not None:
        assert emb.dtype == torch.float32 and emb.numel() >= emb_offset + (B - 1) * emb_bstride + co
        a.emb = emb.data_ptr() + 4 * emb_offset
    a.emb_bstride = int(emb_bstride)
    for r in (res, res2):
        if r is not None:
            _chk(r, name="res")
            assert tuple(r.shape[1:]) == (H, W, co) and r.shape[0] >= (res_bmod or B)
    assert res2 is None or res is not None
    a.res, a.res2, a.res_bmod = _ptr(res), _ptr(res2), int(res_bmod)
    if chan_stats is not None:
        _chk(chan_stats, name="chan_stats")
        assert chan_stats.shape[0] == B and tuple(chan_stats.shape[2:]) == (co, 2)
        a.chan_stats, a.chan_nslab = chan_stats.data_ptr(), chan_stats.shape[1]
    if out16 is not None:
        assert out16[0].dtype == torch.int16 and out16[0].is_contiguous() and tuple(out16[0].shape) == (B, H, W, out16_stride or co)
        a.out16_hi, a.out16_stride = out16[0].data_ptr(), int(out16_stride)
    if gn_next is not None:
        g_w, g_b, g_eps, g_groups, g_act, g_out = gn_next[:6]
        g_lo = None
        if isinstance(g_out, (tuple, list)):
            g_out, g_lo = g_out[0], g_out[1]
        g_mr = gn_next[6] if len(gn_next) > 6 else None
        _chk(g_w, name="gn gamma"); _chk(g_b, name="gn beta")
        assert out is not None and chan_stats is not None and g_out.dtype == torch.int16 and g_out.is_contiguous() and tuple(g_out.shape) == shape
        a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_groups, a.gn_act, a.gn_out16 = g_w.data_ptr(), g_b.data_ptr(), float(g_eps), int(g_groups), int(g_act), g_out.data_ptr()
        if g_lo is not None:
            assert g_lo.dtype == torch.int16 and g_lo.is_contiguous() and tuple(g_lo.shape) == shape
            a.gn_out16_lo = g_lo.data_ptr()
        if g_mr is not None:
            _chk(g_mr, name="gn mean_rstd")
            assert tuple(g_mr.shape) == (B, int(g_groups), 2)
            a.gn_mr = g_mr.data_ptr()
    check(lib().stedm_conv_finish(C.byref(a), int(nshare), _stream()), "stedm_conv_finish")
    return out


def conv_in(x1: torch.Tensor, x2: Optional[torch.Tensor], w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
            x2_bmod: int = 0, chan_stats: Optional[torch.Tensor] = None) -> bool:
    """x1 [B,c1,H,W] NCHW (+ x2 [B,c2,H,W]) -> out [B,H,W,cout] NHWC. chan_stats [B, H/2, cout, 2] (optional): channel partials of
    `out` per pair of image rows; returns whether they were written (False: the shape took the generic path, which has no
    statistics epilogue, and the caller computes them with gn_chan_stats)."""
    _chk(x1, name="x1")
    B, c1, H, W = x1.shape
    c2 = 0 if x2 is None else x2.shape[1]
    if x2 is not None:
        _chk(x2, name="x2")
    args = (x1.data_ptr(), c1, _ptr(x2), c2, x2_bmod, w.data_ptr(), _ptr(bias), out.data_ptr(), B, H, W, out.shape[-1])
    if chan_stats is not None and H % 2 == 0:
        assert tuple(chan_stats.shape) == (B, H // 2, out.shape[-1], 2) and chan_stats.dtype == torch.float32
        rc = lib().stedm_conv_in(*args, chan_stats.data_ptr(), _stream())
        if rc == 0:
            return True
        if rc != 3:
            check(rc, "stedm_conv_in")
    check(lib().stedm_conv_in(*args, None, _stream()), "stedm_conv_in")
    return False


def conv_out_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW [cout,c,3,3] -> the layout stedm_conv_out reads: HWIO [3,3,c,cp] zero-padded to cp = 4 or 8 output channels."""
    cout, c = w_oihw.shape[:2]
    cp = 4 if cout <= 4 else 8
    w = torch.zeros((3, 3, c, cp), dtype=torch.float32, device=w_oihw.device)
    w[..., :cout] = w_oihw.detach().float().permute(2, 3, 1, 0)
    return w.contiguous()


def conv_out(src: torch.Tensor, norm_weight: torch.Tensor, norm_bias: torch.Tensor, eps: float, groups: int, w: torch.Tensor,
             bias: Optional[torch.Tensor], out: torch.Tensor, chan_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src [B,H,W,c] NHWC -> out [B,cout,H,W] NCHW with GroupNorm + SiLU fused into the patch load (statistics from the
    producer-side channel partials; computed here by one stedm_gn_chan_stats pass when `chan_stats` is None). `w` is the OIHW
    weight [cout,c,3,3] or, to skip the per-call permute, the tensor from conv_out_weight()."""
    _chk(src, name="src")
    B, H, W, c = src.shape
    cout = out.shape[1]
    if w.dim() == 4 and tuple(w.shape[:3]) != (3, 3, c):      # OIHW
        w = conv_out_weight(w)
    assert tuple(w.shape) == (3, 3, c, 4 if cout <= 4 else 8)
    if chan_stats is None:
        chan_stats = torch.empty((B, gn_chan_nslab(H * W), c, 2), dtype=torch.float32, device=src.device)
        gn_chan_stats(src, chan_stats)
    check(lib().stedm_conv_out(src.data_ptr(), c, chan_stats.data_ptr(), chan_stats.shape[1], norm_weight.data_ptr(), norm_bias.data_ptr(), float(eps),
                               groups, w.data_ptr(), _ptr(bias), out.data_ptr(), B, H, W, out.shape[1], _stream()), "stedm_conv_out")
    return out


# ------------------------------------------------------------------------------------------- embeddings
def time_embed(t: torch.Tensor, freqs: torch.Tensor, w0t: torch.Tensor, b0: torch.Tensor, w2t: torch.Tensor, b2: torch.Tensor,
               out: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """timestep_embedding + time_embed MLP. t: int64 [B] (stedm_time_embed) or float32 [B], fractional model times
    (stedm_time_embed_f32); any other dtype is refused."""
    if t.dtype == torch.float32:
        fn, name = lib().stedm_time_embed_f32, "stedm_time_embed_f32"
    else:
        _chk(t, torch.int64, "timesteps")
        fn, name = lib().stedm_time_embed, "stedm_time_embed"
    _chk(t, t.dtype, "timesteps")
    B = t.shape[0]
    mc, ted = w0t.shape
    if ws is None:
        ws = torch.empty((B * (mc + ted),), dtype=torch.float32, device=t.device)
    assert ws.numel() >= B * (mc + ted)
    check(fn(t.data_ptr(), freqs.data_ptr(), w0t.data_ptr(), b0.data_ptr(), w2t.data_ptr(), b2.data_ptr(),
             out.data_ptr(), ws.data_ptr(), B, mc, ted, _stream()), name)
    return out


def emb_proj(emb: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _chk(emb, name="emb")
    B, K = emb.shape
    assert wt.shape[0] == K and out.shape == (B, wt.shape[1])
    check(lib().stedm_emb_proj(emb.data_ptr(), wt.data_ptr(), bias.data_ptr(), out.data_ptr(), B, K, wt.shape[1], _stream()),
          "stedm_emb_proj")
    return out


def linear(x: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, act_in: int = 0, act_out: int = 0):
    """out = act_out(bias + act_in(x) @ wt); wt K-major [K, N]; act 0 none / 1 SiLU / 2 ReLU."""
    _chk(x, name="x")
    B, K = x.shape
    check(lib().stedm_linear(x.data_ptr(), wt.data_ptr(), _ptr(bias), out.data_ptr(), B, K, wt.shape[1], act_in, act_out, _stream()),
          "stedm_linear")
    return out


# ------------------------------------------------------------------------------------------- style path
def svit_patch_embed(img, ln_w, ln_b, eps, wt, bias, pos, cls, x, patch: int):
    _chk(img, name="style images")
    B, ns, H, W, C3 = img.shape
    assert C3 == 3
    check(lib().stedm_svit_patch_embed(img.data_ptr(), B, ns, H, W, patch, ln_w.data_ptr(), ln_b.data_ptr(), float(eps), wt.data_ptr(),
                                       bias.data_ptr(), pos.data_ptr(), cls.data_ptr(), x.data_ptr(), x.shape[-1], _stream()),
          "stedm_svit_patch_embed")
    return x


def svit_patch_ln16(img, ln_w, ln_b, eps, hi, lo, patch: int, prec: Precision):
    """patch gather + LayerNorm of SPT -> 16-bit operand planes [B*ntok, patch_dim] (the Linear then runs as a GEMM)."""
    _chk(img, name="style images")
    B, ns, H, W, C3 = img.shape
    assert C3 == 3
    check(lib().stedm_svit_patch_ln16(img.data_ptr(), B, ns, H, W, patch, ln_w.data_ptr(), ln_b.data_ptr(), float(eps), hi.data_ptr(), _ptr(lo),
                                      prec.mm_dtype, _stream()), "stedm_svit_patch_ln16")


def svit_tok_place(tok, pos, cls, x):
    """x[:, 2+t] = tok[t] + pos[2+t]; x[:, 0] = cls + pos[0]; x[:, 1] = pos[1]."""
    B, T, dim = x.shape
    check(lib().stedm_svit_tok_place(tok.data_ptr(), pos.data_ptr(), cls.data_ptr(), x.data_ptr(), B, T - 2, dim, _stream()), "stedm_svit_tok_place")


def ln_apply16(x, gamma, beta, eps, hi, lo, prec: Precision):
    _chk(x, name="x")
    rows = x.numel() // x.shape[-1]
    check(lib().stedm_ln_apply16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), hi.data_ptr(), _ptr(lo), rows, x.shape[-1],
                                 prec.mm_dtype, _stream()), "stedm_ln_apply16")


def qkv_pack(qkv, qscale: float, q, k, vt, B: int, T: int, Tp: int, heads: int, prec: Precision):
    """q, k, vt: (hi, lo) tuples of int16 tensors [B*heads, Tp, 64] / [B*heads, 64, Tp]."""
    check(lib().stedm_qkv_pack(qkv.data_ptr(), int(qkv.dtype == torch.int16), float(qscale), q[0].data_ptr(), _ptr(q[1]), k[0].data_ptr(), _ptr(k[1]),
                               vt[0].data_ptr(), _ptr(vt[1]), B, T, Tp, heads, prec.mm_dtype, _stream()), "stedm_qkv_pack")


def lsa_flash(q, k, vt, out, B: int, T: int, Tp: int, heads: int, prec: Precision):
    check(lib().stedm_lsa_flash(q[0].data_ptr(), _ptr(q[1]), k[0].data_ptr(), _ptr(k[1]), vt[0].data_ptr(), _ptr(vt[1]),
                                out[0].data_ptr(), _ptr(out[1]), B, T, Tp, heads, prec.npass, prec.mm_dtype, _stream()), "stedm_lsa_flash")


def lsa_flash_drop(q, k, vt, out, B: int, T: int, Tp: int, heads: int, prec: Precision, p: float, seed: int, site: int):
    """lsa_flash with train-mode dropout on the attention probabilities (vit_set.py:43, 62); mask stream: include/stedm_hip.h."""
    check(lib().stedm_lsa_flash_drop(q[0].data_ptr(), _ptr(q[1]), k[0].data_ptr(), _ptr(k[1]), vt[0].data_ptr(), _ptr(vt[1]),
                                     out[0].data_ptr(), _ptr(out[1]), B, T, Tp, heads, prec.npass, prec.mm_dtype, float(p), int(seed), int(site),
                                     _stream()), "stedm_lsa_flash_drop")


def dropout_rows(src: torch.Tensor, p: float, seed: int, site: int, prec: Precision, res: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, hi: Optional[torch.Tensor] = None, lo: Optional[torch.Tensor] = None) -> None:
    """out = dropout(src) (+ res) as fp32 and / or 16-bit operand planes (train-mode nn.Dropout of the elementwise sViT sites)."""
    _chk(src, name="src")
    check(lib().stedm_dropout_rows(src.data_ptr(), _ptr(res), _ptr(out), _ptr(hi), _ptr(lo), src.numel(), float(p), int(seed), int(site),
                                   prec.mm_dtype, _stream()), "stedm_dropout_rows")


def qkv_pack_mx8(qkv, qscale: float, q8, qs, k8, ks, vt8, vs, B: int, T: int, Tp: int, heads: int, prec: Precision):
    """qkv (fp32 rows, or int16 rows holding the qkv GEMM's 16-bit output) -> MX-fp8 operands of lsa_flash_mx8: e4m3 bytes + one E8M0 scale per
    32 elements (include/stedm_hip.h)."""
    check(lib().stedm_qkv_pack_mx8(qkv.data_ptr(), int(qkv.dtype == torch.int16), float(qscale), q8.data_ptr(), qs.data_ptr(), k8.data_ptr(), ks.data_ptr(),
                                   vt8.data_ptr(), vs.data_ptr(), B, T, Tp, heads, prec.mm_dtype, _stream()), "stedm_qkv_pack_mx8")


def lsa_flash_mx8(q8, qs, k8, ks, vt8, vs, out16, B: int, T: int, Tp: int, heads: int, prec: Precision):
    check(lib().stedm_lsa_flash_mx8(q8.data_ptr(), qs.data_ptr(), k8.data_ptr(), ks.data_ptr(), vt8.data_ptr(), vs.data_ptr(), out16.data_ptr(), B, T, Tp,
                                    heads, prec.mm_dtype, _stream()), "stedm_lsa_flash_mx8")


def svit_head(x, pool: int, c_old, ln_w, ln_b, eps, wt, bias, out, ws: Optional[torch.Tensor] = None):
    """ws: fp32 workspace for the slab partials of the token pooling (any size >= 2 * B * dim; 1024 * dim covers every batch)."""
    B, T, dim = x.shape
    check(lib().stedm_svit_head(x.data_ptr(), B, T, dim, pool, _ptr(c_old), ln_w.data_ptr(), ln_b.data_ptr(), float(eps), wt.data_ptr(),
                                bias.data_ptr(), out.data_ptr(), out.shape[-1], _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "stedm_svit_head")
    return out


def geglu16(g, hi, lo, prec: Precision):
    _chk(g, name="g")
    M = g.numel() // g.shape[-1]
    check(lib().stedm_geglu16(g.data_ptr(), hi.data_ptr(), _ptr(lo), M, g.shape[-1] // 2, prec.mm_dtype, _stream()), "stedm_geglu16")


def ln_bwd_ws_floats(rows: int, dim: int) -> int:
    return 2 * dim * lib().stedm_ln_bwd_blocks(rows)


def ln_bwd(x, dy, gamma, eps: float, dx, dgamma, dbeta, add=None, accumulate: bool = False, ws=None) -> None:
    """LayerNorm backward over the rows of x / dy [rows, dim]: dx = add + d(LN)/dx . dy; dgamma, dbeta (+)= column sums.
    ws: fp32 workspace of ln_bwd_ws_floats(rows, dim) elements (a caller's cached buffer; allocated here when absent)."""
    _chk(x, name="x"); _chk(dy, name="dy")
    dim = x.shape[-1]
    rows = x.numel() // dim
    need = ln_bwd_ws_floats(rows, dim)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float32, device=x.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need and ws.is_contiguous()
    check(lib().stedm_ln_bwd(x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), float(eps), _ptr(add), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                             ws.data_ptr(), rows, dim, int(accumulate), _stream()), "stedm_ln_bwd")


def geglu_bwd(g, dh, dg) -> None:
    """g [M, 2I] (value | gate), dh [M, I] -> dg [M, 2I] (GEGLU of attention.py:37-44, exact GELU)."""
    _chk(g, name="g"); _chk(dh, name="dh")
    M = g.numel() // g.shape[-1]
    check(lib().stedm_geglu_bwd(g.data_ptr(), dh.data_ptr(), dg.data_ptr(), M, g.shape[-1] // 2, _stream()), "stedm_geglu_bwd")


def lsa_bwd_ws_floats(B: int, T: int, Tp: int, heads: int) -> int:
    return lib().stedm_lsa_bwd_ws_floats(B, T, Tp, heads)


def lsa_bwd(q, k, vt, d_out, d_qkv, d_temp, qscale: float, B: int, T: int, Tp: int, heads: int, prec: Precision, p: float = 0.0, seed: int = 0,
            site: int = 0, accumulate_temp: bool = False, ws=None) -> None:
    """Backward of the LSA attention (vit_set.py:52-66) from the forward's operand planes q, k, vt ((hi, lo) tuples as qkv_pack writes them,
    lo None: hi only; q scaled by qscale = exp(temperature) * log2 e) and d_out [B*T, heads*64]: d_qkv [B*T, 3*heads*64] in to_qkv's output
    order, d_temp[0] (+)= sum dS o dots. p, seed, site: the forward's probability dropout (lsa_flash_drop); p == 0: none."""
    _chk(d_out, name="d_out"); _chk(d_qkv, name="d_qkv"); _chk(d_temp, name="d_temp")
    assert d_out.numel() == B * T * heads * 64 and d_qkv.numel() == 3 * B * T * heads * 64 and d_temp.numel() == 1
    for pl, n in ((q, B * heads * Tp * 64), (k, B * heads * Tp * 64), (vt, B * heads * 64 * Tp)):
        for t in pl:
            assert t is None or (t.dtype == torch.int16 and t.is_contiguous() and t.numel() == n and t.is_cuda)
    need = lsa_bwd_ws_floats(B, T, Tp, heads)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float32, device=d_out.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need and ws.is_contiguous()
    check(lib().stedm_lsa_bwd(q[0].data_ptr(), _ptr(q[1]), k[0].data_ptr(), _ptr(k[1]), vt[0].data_ptr(), _ptr(vt[1]), d_out.data_ptr(),
                              d_qkv.data_ptr(), d_temp.data_ptr(), int(accumulate_temp), float(qscale), B, T, Tp, heads, prec.mm_dtype, float(p),
                              int(seed), int(site), ws.data_ptr(), _stream()), "stedm_lsa_bwd")


def lsa_bwd16_ws_bytes(B: int, T: int, Tp: int, heads: int, p: float = 0.0) -> int:
    return lib().stedm_lsa_bwd16_ws_bytes(B, T, Tp, heads, float(p))


def lsa_bwd16(q, k, vt, d_out, d_qkv, d_temp, qscale: float, B: int, T: int, Tp: int, heads: int, prec: Precision, p: float = 0.0, seed: int = 0,
              site: int = 0, accumulate_temp: bool = False, ws=None) -> None:
    """lsa_bwd on the 16-bit matrix pipe (csrc/lsa_bwd16.hip) for the single-product modes: same arguments, the hi planes only (q, k, vt:
    (hi, None) tuples or the hi tensors). Three values are rounded to the mode's format - dO (times one power of two from its amax),
    P keep / (1 - p) and dS; see include/stedm_hip.h. ws: uint8 workspace of lsa_bwd16_ws_bytes(B, T, Tp, heads, p) bytes."""
    if prec.npass != 1:
        raise ValueError("lsa_bwd16 runs the single-product modes (f16, bf16); the parity mode's backward is lsa_bwd")
    _chk(d_out, name="d_out"); _chk(d_qkv, name="d_qkv"); _chk(d_temp, name="d_temp")
    assert d_out.numel() == B * T * heads * 64 and d_qkv.numel() == 3 * B * T * heads * 64 and d_temp.numel() == 1
    hi = []
    for pl, n in ((q, B * heads * Tp * 64), (k, B * heads * Tp * 64), (vt, B * heads * 64 * Tp)):
        t = pl[0] if isinstance(pl, (tuple, list)) else pl
        assert t.dtype == torch.int16 and t.is_contiguous() and t.numel() == n and t.is_cuda
        hi.append(t)
    need = lsa_bwd16_ws_bytes(B, T, Tp, heads, p)
    if ws is None:
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=d_out.device)
    assert ws.dtype == torch.uint8 and ws.numel() >= need and ws.is_contiguous()
    check(lib().stedm_lsa_bwd16(hi[0].data_ptr(), hi[1].data_ptr(), hi[2].data_ptr(), d_out.data_ptr(), d_qkv.data_ptr(), d_temp.data_ptr(),
                                int(accumulate_temp), float(qscale), B, T, Tp, heads, prec.mm_dtype, float(p), int(seed), int(site),
                                ws.data_ptr(), _stream()), "stedm_lsa_bwd16")


def gelu_bwd(pre, dh, dpre) -> None:
    """dpre = dh * gelu'(pre), the exact erf GELU of FeedForward (vit_set.py:24-31)."""
    _chk(pre, name="pre"); _chk(dh, name="dh"); _chk(dpre, name="dpre")
    assert pre.numel() == dh.numel() == dpre.numel()
    check(lib().stedm_gelu_bwd(pre.data_ptr(), dh.data_ptr(), dpre.data_ptr(), pre.numel(), _stream()), "stedm_gelu_bwd")


def widen16(hi, lo, out, prec: Precision):
    """16-bit operand planes (hi, or hi + lo) -> fp32."""
    _chk(out, name="out")
    assert hi.dtype == torch.int16 and hi.numel() == out.numel() and (lo is None or lo.numel() == out.numel())
    check(lib().stedm_widen16(hi.data_ptr(), _ptr(lo), out.data_ptr(), out.numel(), prec.mm_dtype, _stream()), "stedm_widen16")
    return out


def svit_patch_gather(img, rows, patch: int):
    """The fp32 patch rows [B*ntok, patch*patch*3*ns] that svit_patch_ln16 normalises."""
    _chk(img, name="style images"); _chk(rows, name="rows")
    B, ns, H, W, C3 = img.shape
    assert C3 == 3 and rows.numel() == B * (H // patch) * (W // patch) * patch * patch * 3 * ns
    check(lib().stedm_svit_patch_gather(img.data_ptr(), B, ns, H, W, patch, rows.data_ptr(), _stream()), "stedm_svit_patch_gather")
    return rows


def svit_tok_bwd(dx, d_pos, d_cls, d_tok, accumulate: bool = False) -> None:
    """svit_tok_place reversed: dx [B, T, dim] -> d_pos [T, dim], d_cls [dim] (batch sums, (+)=), d_tok [B*(T-2), dim]."""
    _chk(dx, name="dx"); _chk(d_pos, name="d_pos"); _chk(d_cls, name="d_cls"); _chk(d_tok, name="d_tok")
    B, T, dim = dx.shape
    assert d_pos.numel() == T * dim and d_cls.numel() == dim and d_tok.numel() == B * (T - 2) * dim
    check(lib().stedm_svit_tok_bwd(dx.data_ptr(), d_pos.data_ptr(), d_cls.data_ptr(), d_tok.data_ptr(), B, T - 2, dim, int(accumulate), _stream()),
          "stedm_svit_tok_bwd")


def svit_head_bwd(x, pool: int, ln_w, ln_b, eps: float, w, d_out, dx, d_ln_w, d_ln_b, d_w, d_bias, accumulate: bool = False, ws=None) -> None:
    """svit_head reversed (pool 0 mean / 1 cls, no c_old): x [B, T, dim], w [ncls, dim], d_out [B, ncls] -> dx [B, T, dim] and the head's
    parameter gradients ((+)=)."""
    for t, nm in ((x, "x"), (d_out, "d_out"), (dx, "dx"), (d_ln_w, "d_ln_w"), (d_ln_b, "d_ln_b"), (d_w, "d_w"), (d_bias, "d_bias"), (w, "w")):
        _chk(t, name=nm)
    B, T, dim = x.shape
    ncls = d_out.shape[-1]
    assert d_out.shape[0] == B and dx.numel() == x.numel() and d_w.numel() == w.numel() == ncls * dim and d_bias.numel() == ncls
    assert d_ln_w.numel() == dim and d_ln_b.numel() == dim
    need = lib().stedm_svit_head_bwd_ws_floats(B, dim)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float32, device=x.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need and ws.is_contiguous()
    check(lib().stedm_svit_head_bwd(x.data_ptr(), B, T, dim, pool, ln_w.data_ptr(), ln_b.data_ptr(), float(eps), w.data_ptr(), d_out.data_ptr(), ncls,
                                    dx.data_ptr(), d_ln_w.data_ptr(), d_ln_b.data_ptr(), d_w.data_ptr(), d_bias.data_ptr(), int(accumulate),
                                    ws.data_ptr(), _stream()), "stedm_svit_head_bwd")


def agg_reduce(feats, out, n: int, mode: int):
    _chk(feats, name="features")
    Bn, Fd = feats.shape
    check(lib().stedm_agg_reduce(feats.data_ptr(), out.data_ptr(), Bn // n, n, Fd, mode, _stream()), "stedm_agg_reduce")
    return out


# ------------------------------------------------------------------------------------------- Swin-V2 embedder (non-GEMM pieces)
def swin_patch16(img: torch.Tensor, hi: torch.Tensor, lo: Optional[torch.Tensor], prec: Precision) -> None:
    """img [N, 3, H, W] fp32, ANY strides (the '(b n) c h w' view of NHWC style images is read in place) -> rows [N*H/4*W/4, 64]."""
    assert img.dtype == torch.float32 and img.is_cuda and img.dim() == 4 and img.shape[1] == 3
    N, _, H, W = img.shape
    sn, sc, sh, sw = img.stride()
    check(lib().stedm_swin_patch16(img.data_ptr(), sn, sc, sh, sw, N, H, W, hi.data_ptr(), _ptr(lo), prec.mm_dtype, _stream()), "stedm_swin_patch16")


def swin_ln(y: torch.Tensor, gamma, beta, eps: float, res: Optional[torch.Tensor], out: Optional[torch.Tensor], hi: Optional[torch.Tensor],
            lo: Optional[torch.Tensor], prec: Precision, gate: Optional[torch.Tensor] = None, rows_per_gate: int = 1) -> None:
    """out = res + LayerNorm(y) as fp32 rows and / or 16-bit operand planes (row stride hi.shape[-1] >= dim; pad columns are left alone).
    gate [rows / rows_per_gate] fp32: train-mode stochastic depth, out = res + gate[row // rows_per_gate] * LayerNorm(y)."""
    _chk(y, name="y")
    dim = y.shape[-1]
    if gate is not None:
        _chk(gate, name="gate")
        assert gate.numel() * rows_per_gate == y.numel() // dim
        check(lib().stedm_swin_ln_gated(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), _ptr(res), _ptr(out), _ptr(hi), _ptr(lo),
                                        y.numel() // dim, dim, dim if hi is None else hi.shape[-1], gate.data_ptr(), rows_per_gate, prec.mm_dtype,
                                        _stream()), "stedm_swin_ln_gated")
        return
    check(lib().stedm_swin_ln(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), _ptr(res), _ptr(out), _ptr(hi), _ptr(lo),
                              y.numel() // dim, dim, dim if hi is None else hi.shape[-1], prec.mm_dtype, _stream()), "stedm_swin_ln")


def swin_window_attn(qkv: torch.Tensor, bias_kzero: torch.Tensor, scale: torch.Tensor, rpb: torch.Tensor, hi: torch.Tensor,
                     lo: Optional[torch.Tensor], N: int, H: int, W: int, heads: int, shift: int, prec: Precision) -> None:
    """rpb [heads, 64 queries, 64 keys]; hi / lo [N*H*W, ld16 >= C]. qkv: fp32 rows, or (single-product modes) int16 rows holding the
    qkv GEMM's 16-bit output."""
    C = qkv.shape[-1] // 3
    is16 = qkv.dtype == torch.int16
    _chk(qkv, torch.int16 if is16 else torch.float32, "qkv")
    check(lib().stedm_swin_window_attn(None if is16 else qkv.data_ptr(), qkv.data_ptr() if is16 else None, bias_kzero.data_ptr(), scale.data_ptr(),
                                       rpb.data_ptr(), hi.data_ptr(), _ptr(lo), hi.shape[-1], N, H, W, C, heads, shift, prec.npass, prec.mm_dtype,
                                       _stream()), "stedm_swin_window_attn")


def swin_merge16(x: torch.Tensor, hi: torch.Tensor, lo: Optional[torch.Tensor], prec: Precision) -> None:
    _chk(x, name="x")
    N, H, W, C = x.shape
    check(lib().stedm_swin_merge16(x.data_ptr(), N, H, W, C, hi.data_ptr(), _ptr(lo), prec.mm_dtype, _stream()), "stedm_swin_merge16")


def swin_rpb(cpb: torch.Tensor, index: torch.Tensor, heads: int) -> torch.Tensor:
    """cpb [ntab, heads] fp32, index [4096] int64 (query-major) -> rpb [heads, 64 queries, 64 keys] = 16 sigmoid(cpb[index])."""
    _chk(cpb, name="cpb")
    assert index.dtype == torch.int64 and index.numel() == 4096 and index.is_cuda
    out = torch.empty((heads, 64, 64), dtype=torch.float32, device=cpb.device)
    check(lib().stedm_swin_rpb(cpb.data_ptr(), index.data_ptr(), out.data_ptr(), heads, cpb.shape[0], _stream()), "stedm_swin_rpb")
    return out


def swin_token_mean(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _chk(x, name="x")
    N, T, C = x.shape
    check(lib().stedm_swin_token_mean(x.data_ptr(), out.data_ptr(), N, T, C, _stream()), "stedm_swin_token_mean")
    return out


def spatial_rescale(x, w, out, n_stages: int):
    _chk(x, name="x")
    B, cin, H, W = x.shape
    check(lib().stedm_spatial_rescale(x.data_ptr(), _ptr(w), out.data_ptr(), B, cin, out.shape[1], H, W, n_stages, _stream()),
          "stedm_spatial_rescale")
    return out


# ------------------------------------------------------------------------------------------- attention
ATTN_HEADS_FIRST, ATTN_QKV_FIRST = 0, 1     # STEDM_ATTN_*: QKVAttentionLegacy / QKVAttention (use_new_attention_order) split of the qkv channels


def attn_legacy(qkv: torch.Tensor, out: torch.Tensor, heads: int, order: int = 0) -> torch.Tensor:
    """qkv [B,T,heads*3*ch] -> out [B,T,heads*ch]. order 0: channel = h*3ch + {q,k,v}*ch + c; 1: {q,k,v}*C + h*ch + c (same out)."""
    _chk(qkv, name="qkv")
    B, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    if order == ATTN_HEADS_FIRST:
        check(lib().stedm_attn_legacy(qkv.data_ptr(), out.data_ptr(), B, T, heads, ch, _stream()), "stedm_attn_legacy")
    else:
        check(lib().stedm_attn_qkv(qkv.data_ptr(), out.data_ptr(), B, T, heads, ch, int(order), _stream()), "stedm_attn_qkv")
    return out


def attn_legacy16(qkv: torch.Tensor, out16: torch.Tensor, heads: int, prec: Precision, order: int = 0) -> torch.Tensor:
    """qkv [B,T,heads*3*ch] (fp32, or the int16 plane a conv epilogue wrote) -> out16 [B,T,heads*ch] 16-bit operand plane
    (MFMA form, single-product modes). T = 64 with ch in {32, 64, 128}; T = 64 n <= 4096 with ch in {64, 128} from the int16 plane.
    order: as attn_legacy."""
    is16 = qkv.dtype == torch.int16
    _chk(qkv, torch.int16 if is16 else torch.float32, name="qkv")
    B, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    assert out16.dtype == torch.int16 and out16.numel() == B * T * heads * ch
    if order == ATTN_HEADS_FIRST:
        check(lib().stedm_attn_legacy16(qkv.data_ptr(), 1 if is16 else 0, out16.data_ptr(), B, T, heads, ch, prec.mm_dtype, _stream()), "stedm_attn_legacy16")
    else:
        check(lib().stedm_attn_qkv16(qkv.data_ptr(), 1 if is16 else 0, out16.data_ptr(), B, T, heads, ch, prec.mm_dtype, int(order), _stream()),
              "stedm_attn_qkv16")
    return out16


def philox_normal(rows: int, shape, seed: int, stream: int, device, sample_ids: Optional[torch.Tensor] = None, first_id: int = 0) -> torch.Tensor:
    """[rows, *shape] fp32 N(0, 1) on the device; row i depends only on (seed, stream, its sample id) (stedm_philox_normal)."""
    n = 1
    for d in shape:
        n *= int(d)
    out = torch.empty((rows,) + tuple(int(d) for d in shape), dtype=torch.float32, device=device)
    if sample_ids is not None:
        assert sample_ids.dtype == torch.int64 and sample_ids.is_cuda and sample_ids.numel() == rows and sample_ids.is_contiguous()
    check(lib().stedm_philox_normal(out.data_ptr(), int(rows), n, _ptr(sample_ids), int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF,
                                    _stream()), "stedm_philox_normal")
    return out


# ------------------------------------------------------------------------------------------- DDIM
def _ddim_step_args(x, e_c, step_idx, noise, draw, same_shape):
    """The checks ddim_step, ddim_step_ex and ddim_step_rows share: x [B, C, H, W] fp32 on the device; e_c, noise and every given tensor
    of same_shape ((tensor, name) pairs) of x's shape; a given noise excludes the in-kernel draw; step_idx (when given) int32.
    -> (B, C, H, W)."""
    _chk(x, name="x")
    _chk(e_c, name="e_c")
    if x.dim() != 4:
        raise ValueError(f"x must be [B, C, H, W], got {tuple(x.shape)}")
    shp = tuple(x.shape)
    for t, nm in (((e_c, "e_c"), (noise, "noise")) + same_shape):
        if t is not None:
            _chk(t, name=nm)
            if tuple(t.shape) != shp:
                raise ValueError(f"{nm} {tuple(t.shape)} must have x's shape {shp}")
    if draw and noise is not None:
        raise ValueError("a given noise tensor and the in-kernel draw exclude each other")
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
    return shp


def ddim_step(x: torch.Tensor, e_c: torch.Tensor, e_u: Optional[torch.Tensor], coefs: torch.Tensor, x_prev: torch.Tensor,
              pred_x0: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
              step_idx: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, rescale_phi: float = 0.7) -> torch.Tensor:
    """One DDIM update with the rescaled classifier-free combine (stedm_ddim_step). x_prev may be x."""
    B, Cc, H, W = _ddim_step_args(x, e_c, step_idx, noise, False, ((e_u, "e_u"), (x_prev, "x_prev"), (pred_x0, "pred_x0")))
    check(lib().stedm_ddim_step(x.data_ptr(), e_c.data_ptr(), _ptr(e_u), _ptr(noise), coefs.data_ptr(), _ptr(step_idx),
                                float(cfg_scale), float(rescale_phi), x_prev.data_ptr(), _ptr(pred_x0), B, Cc, H, W, _stream()),
          "stedm_ddim_step")
    return x_prev


def ddim_step_ex(x: torch.Tensor, e_c: torch.Tensor, e_u: Optional[torch.Tensor], coefs: torch.Tensor, x_prev: torch.Tensor,
                 pred_x0: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, draw: bool = False,
                 step_idx: Optional[torch.Tensor] = None, n_iters: int = 0, cfg_scale: float = 1.0, rescale_phi: float = 0.7,
                 temperature: float = 1.0, noise_dropout: float = 0.0, seed: int = 0, first_id: int = 0,
                 eps_out: Optional[torch.Tensor] = None, noise_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ddim_step with the reference's temperature and noise dropout (stedm_ddim_step_ex): noise = ((sigma z) temperature) keep / (1 - p),
    x_prev = (sqrt(a_prev) x0 + dir) + noise. z: `noise`, or with draw=True row first_id + b of ops.philox_normal(seed, stream
    1 + n_iters - 1 - step_idx[0]) drawn in the kernel. The keep bits come from (seed, first_id + b, iteration); see include/stedm_hip.h.
    eps_out: the guided eps (may be e_c); noise_out: the noise term (both [B, C, H, W] fp32). x_prev may be x."""
    B, Cc, H, W = _ddim_step_args(x, e_c, step_idx, noise, draw, ((e_u, "e_u"), (x_prev, "x_prev"), (pred_x0, "pred_x0"),
                                                                  (eps_out, "eps_out"), (noise_out, "noise_out")))
    if not 0.0 <= float(noise_dropout) < 1.0:
        raise ValueError(f"noise_dropout {noise_dropout} outside [0, 1)")
    if (draw or noise_dropout > 0) and (step_idx is None or int(n_iters) <= 0):
        raise ValueError("the in-kernel draw and the noise dropout need step_idx (device int32) and n_iters > 0")
    check(lib().stedm_ddim_step_ex(x.data_ptr(), e_c.data_ptr(), _ptr(e_u), _ptr(noise), coefs.data_ptr(), _ptr(step_idx), int(n_iters),
                                   float(cfg_scale), float(rescale_phi), 1 if draw else 0, float(temperature), float(noise_dropout),
                                   int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, x_prev.data_ptr(), _ptr(pred_x0), _ptr(eps_out),
                                   _ptr(noise_out), B, Cc, H, W, _stream()), "stedm_ddim_step_ex")
    return x_prev


def ddim_step_rows(x: torch.Tensor, e_c: torch.Tensor, e_u: Optional[torch.Tensor], coefs: torch.Tensor, x_prev: torch.Tensor,
                   scales: torch.Tensor, pred_x0: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, draw: bool = False,
                   step_idx: Optional[torch.Tensor] = None, n_iters: int = 0, rescale_phi: float = 0.7, seed: int = 0,
                   first_id: int = 0) -> torch.Tensor:
    """ddim_step with one guidance scale per sample (stedm_ddim_step_rows). scales: device fp32 [B], read by the kernel when it runs, so
    a captured launch replays with what the tensor then holds. Row b with scales[b] == 1 takes the unguided branch (e = e_c) and does
    not read e_u. z: `noise`, or with draw=True row first_id + b of ops.philox_normal(seed, stream 1 + n_iters - 1 - step_idx[0]) drawn in
    the kernel; neither: no noise term. Any W and H (a sample spans ceil(W / 16) workgroups); x_prev may be x."""
    B, Cc, H, W = _ddim_step_args(x, e_c, step_idx, noise, draw, ((e_u, "e_u"), (x_prev, "x_prev"), (pred_x0, "pred_x0")))
    _chk(scales, name="scales")
    if tuple(scales.shape) != (B,):
        raise ValueError(f"scales {tuple(scales.shape)} must be [{B}]")
    if draw and (step_idx is None or int(n_iters) <= 0):
        raise ValueError("the in-kernel draw needs step_idx (device int32) and n_iters > 0")
    check(lib().stedm_ddim_step_rows(x.data_ptr(), e_c.data_ptr(), _ptr(e_u), _ptr(noise), coefs.data_ptr(), _ptr(step_idx), int(n_iters),
                                     scales.data_ptr(), float(rescale_phi), 1 if draw else 0, int(first_id),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, x_prev.data_ptr(), _ptr(pred_x0), B, Cc, H, W, _stream()),
          "stedm_ddim_step_rows")
    return x_prev


def ddim_quantize_x0(pred_x0: torch.Tensor, eps: torch.Tensor, coefs: torch.Tensor, codebook: torch.Tensor, x_prev: torch.Tensor,
                     noise: Optional[torch.Tensor] = None, step_idx: Optional[torch.Tensor] = None,
                     idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """quantize_x0 inside a DDIM step (stedm_ddim_quantize_x0): pred_x0 [B, C, H, W] -> its nearest codebook rows in place (straight-through
    value, the indices of vq_nearest), x_prev = (sqrt(a_prev) pred_x0 + dir eps) + noise. codebook [n_e, C]; idx: optional int64 [B, H, W]."""
    _chk(pred_x0, name="pred_x0"); _chk(eps, name="eps"); _chk(codebook, name="codebook"); _chk(x_prev, name="x_prev")
    if pred_x0.dim() != 4:
        raise ValueError(f"pred_x0 must be [B, C, H, W], got {tuple(pred_x0.shape)}")
    B, Cc, H, W = pred_x0.shape
    if codebook.dim() != 2 or codebook.shape[1] != Cc:
        raise ValueError(f"codebook {tuple(codebook.shape)} must be [n_e, {Cc}]")
    for t, nm in ((eps, "eps"), (noise, "noise"), (x_prev, "x_prev")):
        if t is not None:
            _chk(t, name=nm)
            if tuple(t.shape) != tuple(pred_x0.shape):
                raise ValueError(f"{nm} {tuple(t.shape)} must have pred_x0's shape {tuple(pred_x0.shape)}")
    if idx is not None:
        _chk(idx, torch.int64, "idx")
        assert idx.numel() == B * H * W
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
    check(lib().stedm_ddim_quantize_x0(pred_x0.data_ptr(), eps.data_ptr(), _ptr(noise), coefs.data_ptr(), _ptr(step_idx), codebook.data_ptr(),
                                       int(codebook.shape[0]), Cc, B, H * W, x_prev.data_ptr(), _ptr(idx), _stream()), "stedm_ddim_quantize_x0")
    return x_prev


def _mask_strides(shape, mask: torch.Tensor, x0, sqrt_ac, sqrt_1mac, T: int = 0) -> Tuple[int, int]:
    """The mask blend's operands as ddim_mask_blend, ddpm_step and ddpm_step_ex take them: x0 and the schedule buffers sqrt_ac / sqrt_1mac
    given (at least T entries each), mask [B|1, 1|C, h, w] against shape = (B, C, h, w) -> the mask's (batch, channel) strides in
    elements, 0 where it broadcasts."""
    B, Cc, H, W = shape
    if x0 is None or sqrt_ac is None or sqrt_1mac is None:
        raise ValueError("the mask blend needs x0, sqrt_ac and sqrt_1mac")
    _chk(mask, name="mask"); _chk(sqrt_ac, name="sqrt_ac"); _chk(sqrt_1mac, name="sqrt_1mac")
    if sqrt_ac.numel() < T or sqrt_1mac.numel() < T:
        raise ValueError("sqrt_ac / sqrt_1mac must hold a value for every row of the table")
    if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, Cc) or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"mask {tuple(mask.shape)} must be [B|1, 1|C, h, w] for {tuple(shape)}")
    return (0 if mask.shape[0] == 1 else mask.shape[1] * H * W), (H * W if mask.shape[1] == Cc else 0)


def ddim_mask_blend(img: torch.Tensor, x0: torch.Tensor, mask: torch.Tensor, t: torch.Tensor, sqrt_ac: torch.Tensor, sqrt_1mac: torch.Tensor,
                    noise: Optional[torch.Tensor] = None, step_idx: Optional[torch.Tensor] = None, seed: int = 0, first_id: int = 0) -> torch.Tensor:
    """ddim.py:143-146 in place: img = q_sample(x0, t) * mask + (1 - mask) * img (stedm_ddim_mask_blend). img, x0 [B, C, h, w]; mask
    [B|1, 1|C, h, w] (broadcast over batch / channel); t int64 [B]. noise [B, C, h, w], or None: row first_id + b of ops.philox_normal with
    stream 0x8000 + step_idx[0], drawn in the kernel (step_idx: device int32 [1])."""
    _chk(img, name="img"); _chk(t, torch.int64, "t")
    if img.dim() != 4:
        raise ValueError(f"img must be [B, C, h, w], got {tuple(img.shape)}")
    B, Cc, H, W = img.shape
    bstride, cstride = _mask_strides(img.shape, mask, x0, sqrt_ac, sqrt_1mac)
    _chk(x0, name="x0")
    if tuple(x0.shape) != tuple(img.shape):
        raise ValueError(f"x0 {tuple(x0.shape)} must have img's shape {tuple(img.shape)}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"t must be [B] = [{B}], got {tuple(t.shape)}")
    if noise is not None:
        _chk(noise, name="noise")
        if tuple(noise.shape) != tuple(img.shape):
            raise ValueError(f"noise {tuple(noise.shape)} must have img's shape {tuple(img.shape)}")
    elif step_idx is None:
        raise ValueError("the in-kernel noise draw needs step_idx (device int32)")
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
    check(lib().stedm_ddim_mask_blend(img.data_ptr(), x0.data_ptr(), mask.data_ptr(), bstride, cstride, _ptr(noise), t.data_ptr(),
                                      sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), _ptr(step_idx), B, Cc, H * W, int(first_id),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "stedm_ddim_mask_blend")
    return img


def _ddpm_step_args(x, eps, table, step_idx, same_shape, mask, x0, sqrt_ac, sqrt_1mac):
    """The checks ddpm_step and ddpm_step_ex share: x [B, C, h, w], eps and every given tensor of same_shape ((tensor, name) pairs) of x's
    shape, table [T, 5], step_idx (when given) int32 [1], the mask operands (_mask_strides) -> T and the mask's strides."""
    _chk(x, name="x"); _chk(eps, name="eps"); _chk(table, name="table")
    if x.dim() != 4:
        raise ValueError(f"x must be [B, C, h, w], got {tuple(x.shape)}")
    shp = tuple(x.shape)
    for v, nm in (((eps, "eps"),) + same_shape):
        if v is not None:
            _chk(v, name=nm)
            if tuple(v.shape) != shp:
                raise ValueError(f"{nm} {tuple(v.shape)} must have x's shape {shp}")
    if table.dim() != 2 or table.shape[1] != 5:
        raise ValueError(f"table must be [T, 5], got {tuple(table.shape)}")
    T = int(table.shape[0])
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
        if tuple(step_idx.shape) != (1,):
            raise ValueError(f"step_idx must be [1], got {tuple(step_idx.shape)}")
    return (T,) + ((0, 0) if mask is None else _mask_strides(shp, mask, x0, sqrt_ac, sqrt_1mac, T))


def ddpm_step(x: torch.Tensor, eps: torch.Tensor, table: torch.Tensor, step_idx: torch.Tensor, clip_denoised: bool = True,
              noise: Optional[torch.Tensor] = None, seed: int = 0, first_id: int = 0, mask: Optional[torch.Tensor] = None,
              x0: Optional[torch.Tensor] = None, mask_noise: Optional[torch.Tensor] = None, mask_seed: int = 0,
              sqrt_ac: Optional[torch.Tensor] = None, sqrt_1mac: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ancestral step in place on x [B, C, h, w] (stedm_ddpm_step: ddpm_step_ex with its options off and x_out = x), t = step_idx[0]
    (device int32 [1]):
    x0 = sr x - srm1 eps, clamped to [-1, 1] if clip_denoised; x = c1 x0 + c2 x + sigma z with row t of table [T, 5] {sr, srm1, c1, c2,
    sigma} (schedule.ddpm_step_table). z: noise, or row first_id + b of ops.philox_normal(seed, stream 0x10000 + t), drawn in the kernel.
    mask [B|1, 1|C, h, w] with x0 (and the schedule buffers sqrt_ac / sqrt_1mac): then x = q_sample(x0, t) mask + (1 - mask) x, q_sample's
    noise mask_noise or the draw of ops.ddim_mask_blend at index t with mask_seed."""
    T, bstride, cstride = _ddpm_step_args(x, eps, table, step_idx, ((noise, "noise"), (x0, "x0"), (mask_noise, "mask_noise")), mask, x0,
                                          sqrt_ac, sqrt_1mac)
    B, Cc, H, W = x.shape
    mp = _ptr if mask is not None else (lambda v: None)         # the blend's operands are passed only with a mask
    check(lib().stedm_ddpm_step(x.data_ptr(), eps.data_ptr(), table.data_ptr(), step_idx.data_ptr(), T, 1 if clip_denoised else 0,
                                _ptr(noise), _ptr(mask), bstride, cstride, mp(x0), mp(mask_noise), mp(sqrt_ac), mp(sqrt_1mac), B, Cc, H * W,
                                int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, int(mask_seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "stedm_ddpm_step")
    return x


def ddpm_step_ex(x: torch.Tensor, eps: torch.Tensor, table: torch.Tensor, step_idx: Optional[torch.Tensor] = None,
                 t: Optional[torch.Tensor] = None, clip_denoised: bool = True, noise: Optional[torch.Tensor] = None,
                 temperature: Optional[torch.Tensor] = None, noise_dropout: float = 0.0, codebook: Optional[torch.Tensor] = None,
                 seed: int = 0, first_id: int = 0, mask: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None,
                 mask_noise: Optional[torch.Tensor] = None, mask_seed: int = 0, sqrt_ac: Optional[torch.Tensor] = None,
                 sqrt_1mac: Optional[torch.Tensor] = None, x_out: Optional[torch.Tensor] = None, x0_out: Optional[torch.Tensor] = None,
                 mean_out: Optional[torch.Tensor] = None, idx_out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """ddpm_step with the options of the reference's p_sample / p_mean_variance (stedm_ddpm_step_ex): the timestep is step_idx[0] (device
    int32 [1]) or, exactly one of the two, t (device int64 [B], one table row per sample); x0 is snapped to `codebook` [n_e, C] (the
    indices and arithmetic of vq_nearest) when given; noise = ((z temperature[t]) keep) / (1 - noise_dropout) with temperature a device
    fp32 [T] table (None: 1) and the keep bits drawn from (seed, first_id + b, t) - see include/stedm_hip.h. x is read only: the sample
    goes to x_out (None: not computed; may be x), the predicted x0 after clamp and quantisation to x0_out (required with a codebook),
    the posterior mean to mean_out, the codebook indices to idx_out (int64, B h w elements). Mask arguments as ddpm_step. Returns x_out."""
    T, bstride, cstride = _ddpm_step_args(x, eps, table, step_idx, ((noise, "noise"), (x0, "x0"), (mask_noise, "mask_noise"),
                                                                    (x_out, "x_out"), (x0_out, "x0_out"), (mean_out, "mean_out")),
                                          mask, x0, sqrt_ac, sqrt_1mac)
    B, Cc, H, W = x.shape
    mp = _ptr if mask is not None else (lambda v: None)         # the blend's operands are passed only with a mask
    if (step_idx is None) == (t is None):
        raise ValueError("give step_idx (device int32 [1]) or t (device int64 [B]), not both")
    if t is not None:
        _chk(t, torch.int64, "t")
        if tuple(t.shape) != (B,):
            raise ValueError(f"t must be [B] = [{B}], got {tuple(t.shape)}")
    if temperature is not None:
        _chk(temperature, name="temperature")
        if temperature.dim() != 1 or temperature.shape[0] < T:
            raise ValueError(f"temperature must hold a value for every row of the table ([{T}]), got {tuple(temperature.shape)}")
    if not 0.0 <= float(noise_dropout) < 1.0:
        raise ValueError(f"noise_dropout {noise_dropout} outside [0, 1)")
    if codebook is not None:
        _chk(codebook, name="codebook")
        if codebook.dim() != 2 or codebook.shape[1] != Cc or codebook.shape[0] < 1:
            raise ValueError(f"codebook {tuple(codebook.shape)} must be [n_e, {Cc}]")
        if x0_out is None:
            raise ValueError("with a codebook x0_out is required (the quantised x0 passes through it)")
    elif idx_out is not None:
        raise ValueError("idx_out without a codebook")
    if idx_out is not None:
        _chk(idx_out, torch.int64, "idx_out")
        if idx_out.numel() != B * H * W:
            raise ValueError(f"idx_out must hold {B * H * W} indices, got {idx_out.numel()}")
    if x_out is None and x0_out is None and mean_out is None and idx_out is None:
        raise ValueError("no output requested")
    for v, nm in ((x0_out, "x0_out"), (mean_out, "mean_out")):
        if v is not None and any(v.data_ptr() == o.data_ptr() for o in (x, eps) if o is not None):
            raise ValueError(f"{nm} may not alias x or eps")
    check(lib().stedm_ddpm_step_ex(x.data_ptr(), eps.data_ptr(), table.data_ptr(), _ptr(step_idx), _ptr(t), T, 1 if clip_denoised else 0,
                                   _ptr(noise), _ptr(temperature), float(noise_dropout), _ptr(codebook),
                                   0 if codebook is None else int(codebook.shape[0]), _ptr(mask), bstride, cstride, mp(x0),
                                   mp(mask_noise), mp(sqrt_ac), mp(sqrt_1mac), _ptr(x_out), _ptr(x0_out), _ptr(mean_out), _ptr(idx_out),
                                   B, Cc, H * W, int(first_id), int(seed) & 0xFFFFFFFFFFFFFFFF, int(mask_seed) & 0xFFFFFFFFFFFFFFFF,
                                   _stream()), "stedm_ddpm_step_ex")
    return x_out


def step_advance(step_idx: torch.Tensor, delta: int = 1) -> None:
    check(lib().stedm_step_advance(step_idx.data_ptr(), delta, _stream()), "stedm_step_advance")


def step_set_t(ts_table: torch.Tensor, step_idx: torch.Tensor, t_buf: torch.Tensor) -> None:
    """t_buf[:] = ts_table[step_idx[0]]; int64 tables (DDIM) or float32 tables (DPM-Solver's model times, stedm_step_set_t_f32)."""
    dt = torch.float32 if ts_table.dtype == torch.float32 else torch.int64
    _chk(ts_table, dt, "ts_table")
    _chk(t_buf, dt, "t_buf")
    _chk(step_idx, torch.int32, "step_idx")
    fn, name = (lib().stedm_step_set_t_f32, "stedm_step_set_t_f32") if dt == torch.float32 else (lib().stedm_step_set_t, "stedm_step_set_t")
    check(fn(ts_table.data_ptr(), step_idx.data_ptr(), t_buf.data_ptr(), t_buf.shape[0], _stream()), name)


# ------------------------------------------------------------------------------------------- DPM-Solver++(2M)
DPM_NCOEF = 6       # STEDM_DPM_NCOEF: {alpha_i, sigma_i, r, A, inv_r0, 0.5 A}
DPMU_NCOEF = 24     # STEDM_DPMU_NCOEF: one row of the general DPM-Solver plan (dpm_solver.R_* layout)


def dpm_step(x: torch.Tensor, e_c: torch.Tensor, e_u: Optional[torch.Tensor], x0_prev: torch.Tensor, coefs: torch.Tensor,
             step_idx: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, pred_x0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One DPM-Solver++(2M) step in place on x and x0_prev (stedm_dpm_step): eps = e_u + s (e_c - e_u) (e_u None: e_c),
    x0 = (x - sigma eps) / alpha, x = (r x - A x0) - 0.5 A inv_r0 (x0 - x0_prev), x0_prev = x0 (pred_x0, if given, = x0).
    coefs: device float32 [S, DPM_NCOEF]; step_idx: device int32 [1] selecting the row (None: row 0)."""
    _chk(x, name="x"); _chk(e_c, name="e_c"); _chk(x0_prev, name="x0_prev"); _chk(coefs, name="coefs")
    shp = tuple(x.shape)
    for t, nm in ((e_c, "e_c"), (e_u, "e_u"), (x0_prev, "x0_prev"), (pred_x0, "pred_x0")):
        if t is not None:
            _chk(t, name=nm)
            if tuple(t.shape) != shp:
                raise ValueError(f"{nm} {tuple(t.shape)} must have x's shape {shp}")
    if coefs.dim() != 2 or coefs.shape[1] != DPM_NCOEF:
        raise ValueError(f"coefs must be [S, {DPM_NCOEF}], got {tuple(coefs.shape)}")
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
    check(lib().stedm_dpm_step(x.data_ptr(), e_c.data_ptr(), _ptr(e_u), x0_prev.data_ptr(), _ptr(pred_x0), coefs.data_ptr(),
                               _ptr(step_idx), float(cfg_scale), x.numel(), _stream()), "stedm_dpm_step")
    return x


DPMU_ALL, DPMU_MODEL, DPMU_COMBINE = 0, 1, 2      # STEDM_DPMU_*: the mode argument of stedm_dpm_update


def dpm_update(x: torch.Tensor, base: torch.Tensor, e_c: Optional[torch.Tensor], e_u: Optional[torch.Tensor], slots: torch.Tensor,
               rows: torch.Tensor, step_idx: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, mode: int = DPMU_ALL,
               pred_x0: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One NFE of the general DPM-Solver (stedm_dpm_update) from row step_idx[0] of the plan rows (dpm_solver.dpm_plan): the model output
    m = e_u + s (e_c - e_u) (e_u None: e_c), as x0 = (x - sigma eps) / alpha when the row asks, into slots[w]; then the row's update of the
    base and the slots into x (and into base when the row commits); pred_x0, if given, = the x0 of this NFE. x and base may be one tensor.
    slots: [3, *x.shape]; rows: device float32 [R, DPMU_NCOEF]; mode DPMU_ALL / DPMU_MODEL (slot only) / DPMU_COMBINE (update only)."""
    _chk(x, name="x"); _chk(base, name="base"); _chk(slots, name="slots"); _chk(rows, name="rows")
    shp = tuple(x.shape)
    if mode not in (DPMU_ALL, DPMU_MODEL, DPMU_COMBINE):
        raise ValueError(f"mode must be DPMU_ALL / DPMU_MODEL / DPMU_COMBINE, got {mode!r}")
    if e_c is None and mode != DPMU_COMBINE:
        raise ValueError("e_c is required unless mode is DPMU_COMBINE")
    for t, nm in ((base, "base"), (e_c, "e_c"), (e_u, "e_u"), (pred_x0, "pred_x0")):
        if t is not None:
            _chk(t, name=nm)
            if tuple(t.shape) != shp:
                raise ValueError(f"{nm} {tuple(t.shape)} must have x's shape {shp}")
    if tuple(slots.shape) != (3,) + shp:
        raise ValueError(f"slots must be [3, *x.shape] = {(3,) + shp}, got {tuple(slots.shape)}")
    if rows.dim() != 2 or rows.shape[1] != DPMU_NCOEF:
        raise ValueError(f"rows must be [R, {DPMU_NCOEF}], got {tuple(rows.shape)}")
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
    check(lib().stedm_dpm_update(x.data_ptr(), base.data_ptr(), _ptr(e_c), _ptr(e_u), slots.data_ptr(), x.numel(), _ptr(pred_x0),
                                 rows.data_ptr(), _ptr(step_idx), float(cfg_scale), int(mode), x.numel(), _stream()), "stedm_dpm_update")
    return x


def dpm_threshold(slots: torch.Tensor, max_val: float, rows: Optional[torch.Tensor] = None, step_idx: Optional[torch.Tensor] = None,
                  q_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dynamic thresholding in place (stedm_dpm_threshold): per sample b of the slot, s = max(torch.quantile(|x0_b|, 0.995), max_val)
    (the quantile bit for bit) and x0_b = clamp(x0_b, -s, s) / s. slots: [3, B, ...] with rows (the slot and whether to act come from
    row step_idx[0]), or [B, ...] without rows (acts on it). q_out: device float32 [B] for the quantiles before the max."""
    _chk(slots, name="slots")
    if rows is not None:
        _chk(rows, name="rows")
        if slots.dim() < 3 or slots.shape[0] != 3:
            raise ValueError(f"with rows, slots must be [3, B, ...], got {tuple(slots.shape)}")
        if rows.dim() != 2 or rows.shape[1] != DPMU_NCOEF:
            raise ValueError(f"rows must be [R, {DPMU_NCOEF}], got {tuple(rows.shape)}")
        B = int(slots.shape[1])
        stride = slots[0].numel()
    else:
        if slots.dim() < 2:
            raise ValueError(f"slots must be [B, ...], got {tuple(slots.shape)}")
        B = int(slots.shape[0])
        stride = slots.numel()
    if step_idx is not None:
        _chk(step_idx, torch.int32, "step_idx")
    if q_out is not None:
        _chk(q_out, name="q_out")
        if tuple(q_out.shape) != (B,):
            raise ValueError(f"q_out must be [{B}], got {tuple(q_out.shape)}")
    n = stride // B
    check(lib().stedm_dpm_threshold(slots.data_ptr(), stride, _ptr(rows), _ptr(step_idx), float(max_val), B, n, _ptr(q_out), _stream()),
          "stedm_dpm_threshold")
    return slots


# ------------------------------------------------------------------------------------------- PLMS
PLMS_EULER, PLMS_HEUN, PLMS_MULTISTEP = 0, 1, 2     # STEDM_PLMS_*: the phase argument of stedm_plms_step


def plms_step(x: torch.Tensor, e_c: torch.Tensor, e_u: Optional[torch.Tensor], ring: torch.Tensor, coefs: torch.Tensor,
              step_idx: torch.Tensor, n_iters: int, phase: int, cfg_scale: float = 1.0, pred_x0: Optional[torch.Tensor] = None,
              x_tmp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One PLMS update (stedm_plms_step). e = e_u + s (e_c - e_u) (e_u None: e_c); by phase:
      PLMS_EULER:     ring[0] = e, x_tmp = the DDIM step of x with e (x untouched);
      PLMS_HEUN:      x = the DDIM step with (ring[0] + e) / 2, in place;
      PLMS_MULTISTEP: i = n_iters - 1 - step_idx[0], order min(i, 3) over ring slots (i - j) mod 4, ring[i mod 4] = e, x in place.
    pred_x0 (HEUN / MULTISTEP, optional) = x0. ring: device float32 [4, *x.shape]; coefs: the DDIM table [n_iters, 4]; step_idx: device
    int32 [1], the table row."""
    _chk(x, name="x"); _chk(e_c, name="e_c"); _chk(ring, name="ring"); _chk(coefs, name="coefs"); _chk(step_idx, torch.int32, "step_idx")
    shp = tuple(x.shape)
    for t, nm in ((e_c, "e_c"), (e_u, "e_u"), (pred_x0, "pred_x0"), (x_tmp, "x_tmp")):
        if t is not None:
            _chk(t, name=nm)
            if tuple(t.shape) != shp:
                raise ValueError(f"{nm} {tuple(t.shape)} must have x's shape {shp}")
    if tuple(ring.shape) != (4,) + shp:
        raise ValueError(f"ring {tuple(ring.shape)} must be [4, *{shp}]")
    if coefs.dim() != 2 or coefs.shape[1] != 4 or coefs.shape[0] != int(n_iters):
        raise ValueError(f"coefs must be the DDIM table [{int(n_iters)}, 4], got {tuple(coefs.shape)}")
    if tuple(step_idx.shape) != (1,):
        raise ValueError(f"step_idx must be [1], got {tuple(step_idx.shape)}")
    if phase not in (PLMS_EULER, PLMS_HEUN, PLMS_MULTISTEP):
        raise ValueError(f"unknown PLMS phase {phase}")
    if phase == PLMS_EULER and x_tmp is None:
        raise ValueError("the Euler phase writes x_tmp")
    check(lib().stedm_plms_step(x.data_ptr(), e_c.data_ptr(), _ptr(e_u), ring.data_ptr(), coefs.data_ptr(), step_idx.data_ptr(),
                                int(n_iters), int(phase), float(cfg_scale), _ptr(pred_x0), _ptr(x_tmp), x.numel(), _stream()),
          "stedm_plms_step")
    return x



# ------------------------------------------------------------------------------------------- training step (backward)
def pack_conv_weight_strided(w: torch.Tensor, sn: int, sc: int, flip: bool, cout: int, cin: int, ks: int, prec: Precision, want_hi: bool = True,
                             want_frag: bool = False):
    """(hi, lo, frag) packs of the filter whose element (n, ci, tap) is w.flatten()[n*sn + ci*sc + tap'] (see stedm_pack_conv_weight_strided)."""
    _chk(w, name="w")
    hi = _pack_empty("planes", w, cout, cin, ks * ks) if want_hi else None
    lo = torch.empty_like(hi) if (want_hi and prec.npass == 3) else None
    frag = _pack_empty("frag", w, cout, cin, ks * ks) if want_frag else None
    check(lib().stedm_pack_conv_weight_strided(w.data_ptr(), sn, sc, int(flip), _ptr(hi), _ptr(lo), _ptr(frag), cout, cin, ks, prec.mm_dtype, _stream()),
          "stedm_pack_conv_weight_strided")
    return hi, lo, frag


def gn_fold(cs1: torch.Tensor, cs2: Optional[torch.Tensor], groups: int, HW: int, eps: float, out: torch.Tensor) -> torch.Tensor:
    """chan partials of [x1|x2] -> out [B][groups][2] = {mean, rstd}."""
    B, c1 = cs1.shape[0], cs1.shape[2]
    c2 = 0 if cs2 is None else cs2.shape[2]
    assert tuple(out.shape) == (B, groups, 2)
    check(lib().stedm_gn_fold(cs1.data_ptr(), cs1.shape[1], c1, _ptr(cs2), 0 if cs2 is None else cs2.shape[1], c2, groups, B, HW, float(eps),
                              out.data_ptr(), _stream()), "stedm_gn_fold")
    return out


def gn_bwd_ws_floats(B: int, HW: int, C: int, groups: int) -> int:
    return lib().stedm_gn_bwd_ws_floats(B, HW, C, groups)


def _gn_bwd_film_args(B: int, C: int, dx16, film=None, film_off: int = 0, film_bstride: int = 0, d_film=None, d_film_off: int = 0):
    """C arguments the gn_bwd* calls share: the (dx16_hi, dx16_lo) pointer pair and, with `film`, the checked (film, film_bstride, film_off)
    and (d_film, its row stride, d_film_off) triples (None without)."""
    d16 = (None if dx16 is None else dx16[0].data_ptr(), None if dx16 is None else _ptr(dx16[1]))
    if film is None:
        return d16, None, None
    _chk(film, name="film")
    assert film_off >= 0 and film.numel() >= (B - 1) * film_bstride + film_off + 2 * C, "film rows out of range"
    assert d_film.dtype == torch.float32 and d_film.dim() == 2 and d_film.shape[0] == B and d_film.stride(1) == 1
    assert 0 <= d_film_off and d_film_off + 2 * C <= d_film.shape[1], "d_film columns out of range"
    return d16, (film.data_ptr(), int(film_bstride), int(film_off)), (d_film.data_ptr(), d_film.stride(0), int(d_film_off))


def gn_bwd(x1, x2, mean_rstd, gamma, beta, groups: int, act: int, dA, add, ws, dx1, acc1: bool, dx2, acc2: bool, dx16, prec: Precision,
           dgamma, dbeta, acc_param: bool) -> None:
    """Backward of act(GroupNorm([x1|x2])): see stedm_gn_bwd."""
    _chk(x1, name="x1"); _chk(dA, name="dA")
    B, c1 = x1.shape[0], x1.shape[-1]
    HW = x1.numel() // (B * c1)
    c2 = 0 if x2 is None else x2.shape[-1]
    assert dA.numel() == B * HW * (c1 + c2) and ws.numel() >= gn_bwd_ws_floats(B, HW, c1 + c2, groups)
    check(lib().stedm_gn_bwd(x1.data_ptr(), c1, _ptr(x2), c2, mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), groups, act, dA.data_ptr(),
                             _ptr(add), B, HW, ws.data_ptr(), dx1.data_ptr(), int(acc1), _ptr(dx2), int(acc2),
                             None if dx16 is None else dx16[0].data_ptr(), None if dx16 is None else _ptr(dx16[1]), prec.mm_dtype,
                             dgamma.data_ptr(), dbeta.data_ptr(), int(acc_param), _stream()), "stedm_gn_bwd")


def gn_bwd_film(x1, mean_rstd, gamma, beta, groups: int, act: int, film, film_off: int, film_bstride: int, dA, add, ws, dx1, acc1: bool, dx16,
                prec: Precision, dgamma, dbeta, acc_param: bool, d_film, d_film_off: int) -> None:
    """Backward of act(GroupNorm(x1) * (1 + scale) + shift): see stedm_gn_bwd_film. d_film [B, N]: row b receives dscale | dshift at
    columns [d_film_off, d_film_off + 2 C); its row stride may exceed N (a column block of a wider matrix)."""
    _chk(x1, name="x1"); _chk(dA, name="dA")
    B, C = x1.shape[0], x1.shape[-1]
    HW = x1.numel() // (B * C)
    assert dA.numel() == B * HW * C and ws.numel() >= gn_bwd_ws_floats(B, HW, C, groups)
    d16, fl, dfl = _gn_bwd_film_args(B, C, dx16, film, film_off, film_bstride, d_film, d_film_off)
    check(lib().stedm_gn_bwd_film(x1.data_ptr(), C, mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), groups, act, *fl, dA.data_ptr(), _ptr(add),
                                  B, HW, ws.data_ptr(), dx1.data_ptr(), int(acc1), *d16, prec.mm_dtype, dgamma.data_ptr(), dbeta.data_ptr(),
                                  int(acc_param), *dfl, _stream()), "stedm_gn_bwd_film")


def gn_bwd_drop(x1, mean_rstd, gamma, beta, groups: int, act: int, dA, add, ws, dx1, acc1: bool, dx16, prec: Precision, dgamma, dbeta,
                acc_param: bool, drop, film=None, film_off: int = 0, film_bstride: int = 0, d_film=None, d_film_off: int = 0) -> None:
    """gn_bwd / gn_bwd_film (with `film`) of a GroupNorm whose activation went through gn_apply16c_drop with the same `drop` =
    (p, seed, site, step, step_ptr): dA is masked and scaled on load (stedm_gn_bwd_drop / stedm_gn_bwd_film_drop). One source tensor."""
    _chk(x1, name="x1"); _chk(dA, name="dA")
    B, C = x1.shape[0], x1.shape[-1]
    HW = x1.numel() // (B * C)
    assert dA.numel() == B * HW * C and ws.numel() >= gn_bwd_ws_floats(B, HW, C, groups)
    d16, fl, dfl = _gn_bwd_film_args(B, C, dx16, film, film_off, film_bstride, d_film, d_film_off)
    if film is None:
        check(lib().stedm_gn_bwd_drop(x1.data_ptr(), C, None, 0, mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), groups, act, dA.data_ptr(),
                                      _ptr(add), B, HW, ws.data_ptr(), dx1.data_ptr(), int(acc1), None, 0, *d16, prec.mm_dtype, dgamma.data_ptr(),
                                      dbeta.data_ptr(), int(acc_param), *_drop_tail(drop), _stream()), "stedm_gn_bwd_drop")
        return
    check(lib().stedm_gn_bwd_film_drop(x1.data_ptr(), C, mean_rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), groups, act, *fl, dA.data_ptr(), _ptr(add),
                                       B, HW, ws.data_ptr(), dx1.data_ptr(), int(acc1), *d16, prec.mm_dtype, dgamma.data_ptr(), dbeta.data_ptr(),
                                       int(acc_param), *dfl, *_drop_tail(drop), _stream()), "stedm_gn_bwd_film_drop")


def im2col_t16(src16: torch.Tensor, dst16: torch.Tensor, ks: int, mode: int) -> None:
    """16-bit NHWC plane [B,Hs,Ws,C] -> [(tap*C + c)][Ppad] (dst16 [ks*ks*C, Ppad])."""
    B, Hs, Ws, Cc = src16.shape
    assert src16.dtype == torch.int16 and dst16.dtype == torch.int16 and dst16.shape[0] == ks * ks * Cc
    check(lib().stedm_im2col_t16(src16.data_ptr(), dst16.data_ptr(), B, Hs, Ws, Cc, ks, mode, dst16.shape[1], _stream()), "stedm_im2col_t16")


def wgrad_to_oihw(dw: torch.Tensor, grad: torch.Tensor, cin_ld: int, cout_ld: int, accumulate: bool, nsplit: int = 1) -> None:
    cout, cin = grad.shape[0], grad.shape[1]
    taps = grad.numel() // (cout * cin)
    _chk(grad, name="grad")
    check(lib().stedm_wgrad_to_oihw(dw.data_ptr(), grad.data_ptr(), cout, cin, taps, cin_ld, cout_ld, int(accumulate), nsplit, _stream()),
          "stedm_wgrad_to_oihw")


def wgrad3x3_plan(B: int, H: int, W: int, cin: int, cout: int) -> int:
    """split count of the direct 3x3 weight-gradient kernel for this shape, 0 when the shape is not supported"""
    ks = C.c_int(0)
    return ks.value if lib().stedm_wgrad3x3_plan(B, H, W, cin, cout, C.byref(ks)) else 0


def wgrad3x3(x16: torch.Tensor, dy16: torch.Tensor, part: torch.Tensor, prec: Precision) -> None:
    """x16 [B,H,W,cin], dy16 [B,H,W,cout] bf16 planes -> part [ksplit, 9, cin, cout] fp32 partial weight gradients"""
    B, H, W, cin = x16.shape
    cout = dy16.shape[-1]
    assert x16.dtype == torch.int16 and dy16.dtype == torch.int16 and tuple(dy16.shape[:3]) == (B, H, W) and part.dtype == torch.float32
    assert part.numel() >= wgrad3x3_plan(B, H, W, cin, cout) * 9 * cin * cout
    check(lib().stedm_wgrad3x3(x16.data_ptr(), dy16.data_ptr(), part.data_ptr(), B, H, W, cin, cout, prec.mm_dtype, _stream()), "stedm_wgrad3x3")


def wgrad3x3_oihw(x16: torch.Tensor, dy16: torch.Tensor, out: torch.Tensor, prec: Precision) -> None:
    """x16 [B,H,W,cin], dy16 [B,H,W,cout] bf16 planes -> out [ksplit, cout, cin, 3, 3] fp32: the split-K slices in the parameter's own order
    (ksplit == 1: `out` may be the gradient itself; else sum_planes adds the slices)"""
    B, H, W, cin = x16.shape
    cout = dy16.shape[-1]
    assert x16.dtype == torch.int16 and dy16.dtype == torch.int16 and tuple(dy16.shape[:3]) == (B, H, W) and out.dtype == torch.float32
    assert out.is_contiguous() and out.numel() >= wgrad3x3_plan(B, H, W, cin, cout) * 9 * cin * cout
    check(lib().stedm_wgrad3x3_oihw(x16.data_ptr(), dy16.data_ptr(), out.data_ptr(), B, H, W, cin, cout, prec.mm_dtype, _stream()), "stedm_wgrad3x3_oihw")


def sum_planes(part: torch.Tensor, out: torch.Tensor, nsplit: int, accumulate: bool = False) -> None:
    """out (+)= part[0] + ... + part[nsplit - 1] (slices of out.numel() floats each, fixed order)"""
    n = out.numel()
    assert part.dtype == torch.float32 and out.dtype == torch.float32 and out.is_contiguous() and part.numel() >= nsplit * n
    check(lib().stedm_sum_planes(part.data_ptr(), out.data_ptr(), n, int(nsplit), int(accumulate), _stream()), "stedm_sum_planes")


def wgrad1x1_plan(P: int, cin: int, cout: int) -> int:
    """split count of the direct 1x1 weight-gradient kernel for this shape, 0 when the shape is not supported"""
    ks = C.c_int(0)
    return ks.value if lib().stedm_wgrad1x1_plan(P, cin, cout, C.byref(ks)) else 0


def wgrad1x1(x16: torch.Tensor, dy16: torch.Tensor, part: torch.Tensor, prec: Precision) -> None:
    """x16 [..., cin], dy16 [..., cout] bf16 planes over the same pixels -> part [ksplit, cin, cout] fp32 partial weight gradients"""
    cin, cout = x16.shape[-1], dy16.shape[-1]
    P = x16.numel() // cin
    assert x16.dtype == torch.int16 and dy16.dtype == torch.int16 and dy16.numel() // cout == P and part.dtype == torch.float32
    assert x16.is_contiguous() and dy16.is_contiguous() and part.numel() >= wgrad1x1_plan(P, cin, cout) * cin * cout
    check(lib().stedm_wgrad1x1(x16.data_ptr(), dy16.data_ptr(), part.data_ptr(), P, cin, cout, prec.mm_dtype, _stream()), "stedm_wgrad1x1")


def chan_sum_fold(cs: torch.Tensor, per_sample: Optional[torch.Tensor], ld: int, total: Optional[torch.Tensor], accumulate: bool,
                  total2: Optional[torch.Tensor] = None) -> None:
    """channel partials -> per-sample sums and the batch total (total2: a second destination of the same total)"""
    B, nslab, Cc, _ = cs.shape
    check(lib().stedm_chan_sum_fold2(cs.data_ptr(), B, nslab, Cc, _ptr(per_sample), ld, _ptr(total), int(accumulate), _ptr(total2), _stream()),
          "stedm_chan_sum_fold2")


def sum2x2(x: torch.Tensor, out: torch.Tensor, accumulate: bool) -> None:
    B, H, W, Cc = out.shape
    assert tuple(x.shape) == (B, 2 * H, 2 * W, Cc)
    check(lib().stedm_sum2x2(x.data_ptr(), out.data_ptr(), B, H, W, Cc, int(accumulate), _stream()), "stedm_sum2x2")


def _resample_cs(out: torch.Tensor, chan_stats: Optional[torch.Tensor]) -> int:
    """slot count of the statistics avgpool2x2 / replicate2x2 leave for `out`: gn_chan_nslab of its pixels (include/stedm_hip.h)"""
    if chan_stats is None:
        return 0
    B, Ho, Wo, Cc = out.shape
    assert chan_stats.dtype == torch.float32 and chan_stats.is_contiguous() and tuple(chan_stats.shape) == (B, gn_chan_nslab(Ho * Wo), Cc, 2), \
        f"chan_stats must be [B][gn_chan_nslab(Hout * Wout)][C][2] fp32, got {tuple(chan_stats.shape)}"
    return chan_stats.shape[1]


def avgpool2x2(x: torch.Tensor, out: torch.Tensor, chan_stats: Optional[torch.Tensor] = None) -> None:
    """out [B][H/2][W/2][C] = 2 x 2 average pool of x [B][H][W][C] (the conv-less Downsample); chan_stats: also the channel statistics of out"""
    _chk(x, name="x")
    _chk(out, name="out")
    B, H, W, Cc = x.shape
    assert tuple(out.shape) == (B, H // 2, W // 2, Cc)      # (an odd H or W is the library's argument error)
    check(lib().stedm_avgpool2x2(x.data_ptr(), out.data_ptr(), B, H, W, Cc, _ptr(chan_stats), _resample_cs(out, chan_stats), _stream()),
          "stedm_avgpool2x2")


def replicate2x2(x: torch.Tensor, out: torch.Tensor, scale: float = 1.0, accumulate: bool = False, chan_stats: Optional[torch.Tensor] = None) -> None:
    """out [B][2H][2W][C] (+)= scale * x [B][H][W][C] at all four positions: the conv-less Upsample (scale 1), the backward of avgpool2x2 (0.25)"""
    _chk(x, name="x")
    _chk(out, name="out")
    B, H, W, Cc = x.shape
    assert tuple(out.shape) == (B, 2 * H, 2 * W, Cc)
    check(lib().stedm_replicate2x2(x.data_ptr(), out.data_ptr(), B, H, W, Cc, float(scale), int(accumulate), _ptr(chan_stats),
                                   _resample_cs(out, chan_stats), _stream()), "stedm_replicate2x2")


def gn_apply16c_resample(x: torch.Tensor, cs: torch.Tensor, out_hi: torch.Tensor, out_lo: Optional[torch.Tensor], prec: Precision, gamma: torch.Tensor,
                         beta: torch.Tensor, mode: int, eps: float = 1e-5, groups: int = 32, act: int = 0, xr: Optional[torch.Tensor] = None,
                         mean_rstd: Optional[torch.Tensor] = None) -> None:
    """The front of ResBlock(up / down) (stedm_gn_apply16c_resample): act(GroupNorm(x)) of x [B][H][W][C] from its channel partials `cs`,
    resampled into the 16-bit planes out_hi (/ out_lo) at the new resolution - mode 1: 2 x 2 average pool, [B][H/2][W/2][C]; mode 2: nearest
    x2, [B][2H][2W][C] - and, with xr, the same resampling of raw x (fp32; = avgpool2x2 / replicate2x2 at scale 1). mean_rstd as gn_apply16c."""
    _chk(x, name="x")
    assert mode in (1, 2), "mode: 1 (pool) or 2 (nearest)"
    B, H, W, Cc = x.shape
    new = (B, H // 2, W // 2, Cc) if mode == 1 else (B, 2 * H, 2 * W, Cc)      # (an odd H or W in mode 1, C % 8 != 0: the library's argument errors)
    assert cs.dtype == torch.float32 and cs.is_contiguous() and cs.dim() == 4 and cs.shape[0] == B and tuple(cs.shape[2:]) == (Cc, 2), \
        f"cs must be [B][nslab][C][2] fp32, got {tuple(cs.shape)}"
    assert gamma.numel() == Cc and beta.numel() == Cc and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    for pl in (out_hi, out_lo):
        assert pl is None or (pl.element_size() == 2 and pl.is_contiguous() and tuple(pl.shape) == new), f"planes must be 16-bit {new}"
    if xr is not None:
        _chk(xr, name="xr")
        assert tuple(xr.shape) == new
    if mean_rstd is not None:
        assert mean_rstd.dtype == torch.float32 and mean_rstd.is_contiguous() and tuple(mean_rstd.shape) == (B, groups, 2)
    check(lib().stedm_gn_apply16c_resample(x.data_ptr(), Cc, cs.data_ptr(), cs.shape[1], gamma.data_ptr(), beta.data_ptr(), float(eps), groups, act,
                                           B, H, W, int(mode), out_hi.data_ptr(), _ptr(out_lo), _ptr(xr), _ptr(mean_rstd), prec.mm_dtype, _stream()),
          "stedm_gn_apply16c_resample")


def zero_insert16(x: torch.Tensor, hi: torch.Tensor, lo: Optional[torch.Tensor], prec: Precision) -> None:
    B, Ho, Wo, Cc = x.shape
    assert tuple(hi.shape) == (B, 2 * Ho, 2 * Wo, Cc)
    check(lib().stedm_zero_insert16(x.data_ptr(), hi.data_ptr(), _ptr(lo), B, Ho, Wo, Cc, prec.mm_dtype, _stream()), "stedm_zero_insert16")


def attn_legacy_bwd(qkv: torch.Tensor, d_out: torch.Tensor, d_qkv: torch.Tensor, heads: int, order: int = 0) -> None:
    """order: as attn_legacy (qkv and d_qkv both in that order)."""
    B, T, C3 = qkv.shape
    nws = lib().stedm_attn_legacy_bwd_ws_floats(B, T, heads)
    ws = torch.empty((nws,), dtype=torch.float32, device=qkv.device) if nws else None
    if order == ATTN_HEADS_FIRST:
        check(lib().stedm_attn_legacy_bwd(qkv.data_ptr(), d_out.data_ptr(), d_qkv.data_ptr(), B, T, heads, C3 // (3 * heads), _ptr(ws), _stream()),
              "stedm_attn_legacy_bwd")
    else:
        check(lib().stedm_attn_qkv_bwd(qkv.data_ptr(), d_out.data_ptr(), d_qkv.data_ptr(), B, T, heads, C3 // (3 * heads), int(order), _ptr(ws),
                                       _stream()), "stedm_attn_qkv_bwd")


def gemm_f32(A: torch.Tensor, ta: bool, Bm: torch.Tensor, tb: bool, Cm: torch.Tensor, alpha: float = 1.0, beta: float = 0.0,
             ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cm = alpha * op(A) @ op(Bm) + beta * Cm on 2-D fp32 tensors (rows may be strided views: last stride must be 1)."""
    for t in (A, Bm, Cm):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.is_cuda
    M, N = Cm.shape
    K = A.shape[0] if ta else A.shape[1]
    assert (A.shape[1] if ta else A.shape[0]) == M and (Bm.shape[0] if tb else Bm.shape[1]) == N and (Bm.shape[1] if tb else Bm.shape[0]) == K
    check(lib().stedm_gemm_f32(A.data_ptr(), A.stride(0), int(ta), Bm.data_ptr(), Bm.stride(0), int(tb), Cm.data_ptr(), Cm.stride(0), M, N, K,
                               float(alpha), float(beta), _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "stedm_gemm_f32")
    return Cm


def silu(x: torch.Tensor, out: torch.Tensor, dy: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy None: out = silu(x); else out = dy * silu'(x)."""
    _chk(x, name="x")
    check(lib().stedm_silu(x.data_ptr(), _ptr(dy), out.data_ptr(), x.numel(), 0 if dy is None else 1, _stream()), "stedm_silu")
    return out


def q_sample(x0: torch.Tensor, noise: torch.Tensor, t: torch.Tensor, sqrt_ac: torch.Tensor, sqrt_1mac: torch.Tensor) -> torch.Tensor:
    """ddpm.py:277-280: sqrt_ac[t] * x0 + sqrt_1mac[t] * noise (per-sample scalars from the fp32 schedule buffers)."""
    _chk(x0, name="x0"); _chk(noise, name="noise"); _chk(t, torch.int64, "t")
    out = torch.empty_like(x0)
    B = x0.shape[0]
    check(lib().stedm_q_sample(x0.data_ptr(), noise.data_ptr(), t.data_ptr(), sqrt_ac.data_ptr(), sqrt_1mac.data_ptr(), out.data_ptr(), B,
                               x0.numel() // B, _stream()), "stedm_q_sample")
    return out


def l1_loss(pred: torch.Tensor, target: torch.Tensor, d_pred: Optional[torch.Tensor], ws: torch.Tensor, loss: torch.Tensor, grad_scale: float = 1.0):
    _chk(pred, name="pred"); _chk(target, name="target")
    assert ws.dtype == torch.float64 and ws.numel() >= 1024 and pred.numel() == target.numel()
    check(lib().stedm_l1_loss(pred.data_ptr(), target.data_ptr(), pred.numel(), float(grad_scale), _ptr(d_pred), ws.data_ptr(), loss.data_ptr(), _stream()),
          "stedm_l1_loss")
    return loss


LOSS_KINDS = {"l1": 0, "l2": 1}


def diffusion_loss_blocks(n: int) -> int:
    """blocks per sample of stedm_diffusion_loss's first launch (256 threads each, striding over the sample's n elements)"""
    return int(lib().stedm_diffusion_loss_blocks(int(n)))


def diffusion_loss_ws_doubles(B: int, n: int) -> int:
    return int(B) * (diffusion_loss_blocks(n) + 1)


def diffusion_loss(pred: torch.Tensor, target: torch.Tensor, t: torch.Tensor, logvar: torch.Tensor, lvlb: torch.Tensor, kind,
                   l_simple_weight: float = 1.0, elbo_weight: float = 0.0, grad_scale: float = 1.0, d_pred: Optional[torch.Tensor] = None,
                   d_logvar: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's objective (ddpm.py:1015-1048) on pred / target [B, ...] (include/stedm_hip.h: stedm_diffusion_loss). kind: 'l1' / 'l2'
    (or 0 / 1). -> out [4] = {loss, loss_simple, loss_gamma, loss_vlb}; d_pred (like pred) and d_logvar [T] are filled when given."""
    _chk(pred, name="pred"); _chk(target, name="target"); _chk(t, torch.int64, "t"); _chk(logvar, name="logvar"); _chk(lvlb, name="lvlb")
    B = pred.shape[0]
    n = pred.numel() // B
    T = logvar.numel()
    assert pred.numel() == target.numel() == B * n and t.numel() == B and lvlb.numel() == T
    need = diffusion_loss_ws_doubles(B, n)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float64, device=pred.device)
    if out is None:
        out = torch.empty((4,), dtype=torch.float32, device=pred.device)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= need and out.dtype == torch.float32 and out.numel() >= 4
    if d_pred is not None:
        _chk(d_pred, name="d_pred")
        assert d_pred.numel() == pred.numel()
    if d_logvar is not None:
        _chk(d_logvar, name="d_logvar")
        assert d_logvar.numel() == T
    check(lib().stedm_diffusion_loss(pred.data_ptr(), target.data_ptr(), t.data_ptr(), logvar.data_ptr(), lvlb.data_ptr(), B, n, T,
                                     LOSS_KINDS.get(kind, kind), float(l_simple_weight), float(elbo_weight), float(grad_scale), _ptr(d_pred),
                                     _ptr(d_logvar), ws.data_ptr(), ws.numel(), out.data_ptr(), _stream()), "stedm_diffusion_loss")
    return out


def spatial_rescale_wgrad(x: torch.Tensor, d_out: torch.Tensor, dw: torch.Tensor, n_stages: int, accumulate: bool = False) -> torch.Tensor:
    """channel_mapper weight gradient of the SpatialRescaler: x [B,cin,H,W], d_out [B,cout,H>>n,W>>n] -> dw [cout,cin(,1,1)]."""
    _chk(x, name="x"); _chk(d_out, name="d_out"); _chk(dw, name="dw")
    B, cin, H, W = x.shape
    cout = d_out.shape[1]
    assert dw.numel() == cout * cin and tuple(d_out.shape) == (B, cout, H >> n_stages, W >> n_stages)
    ws = torch.empty((B * cin * cout,), dtype=torch.float32, device=x.device)
    check(lib().stedm_spatial_rescale_wgrad(x.data_ptr(), d_out.data_ptr(), ws.data_ptr(), dw.data_ptr(), B, cin, cout, H, W, n_stages, int(accumulate),
                                            _stream()), "stedm_spatial_rescale_wgrad")
    return dw


def axpby(x: torch.Tensor, y: torch.Tensor, alpha: float = 1.0, beta: float = 1.0) -> torch.Tensor:
    """y = alpha * x + beta * y (flat fp32 tensors, numel % 4 == 0)."""
    _chk(x, name="x"); _chk(y, name="y")
    assert x.numel() == y.numel()
    check(lib().stedm_axpby_f32(x.data_ptr(), y.data_ptr(), x.numel(), float(alpha), float(beta), _stream()), "stedm_axpby_f32")
    return y


# Kernels that write PARAMETERS through raw pointers (no torch version bump) count here; the epoch is part of the freshness token of the
# weight packs an optimizer pass wrote itself (UNetModel.freshness_token), so any later raw-pointer writer forces a full re-pack even if it
# forgets UNetModel.invalidate().
_RAW_WRITES = [0]


def raw_write_epoch() -> int:
    return _RAW_WRITES[0]


def note_raw_write() -> None:
    _RAW_WRITES[0] += 1


def grad_norm_blocks(n: int) -> int:
    """doubles of workspace stedm_grad_norm needs for n gradient values (one partial per block)"""
    return int(lib().stedm_grad_norm_blocks(int(n)))


def grad_norm(g: torch.Tensor, grad_scale: float = 1.0, max_norm: float = 0.0, ws: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [3] = {grad_scale * ||g||_2, clip coefficient of clip_grad_norm_(max_norm), non-finite flag} on the device (include/stedm_hip.h:
    stedm_grad_norm); g: flat contiguous fp32 (any 4-byte aligned start). max_norm <= 0: the coefficient is 1. No host read."""
    _chk(g, name="g")
    n = g.numel()
    assert n > 0
    need = grad_norm_blocks(n)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float64, device=g.device)
    if out is None:
        out = torch.empty((3,), dtype=torch.float32, device=g.device)
    assert ws.dtype == torch.float64 and ws.is_contiguous() and ws.numel() >= need and out.dtype == torch.float32 and out.numel() >= 3
    check(lib().stedm_grad_norm(g.data_ptr(), n, float(grad_scale), float(max_norm), ws.data_ptr(), out.data_ptr(), _stream()), "stedm_grad_norm")
    return out


def _coef_ptr(clip_coef: torch.Tensor) -> int:
    assert clip_coef.dtype == torch.float32 and clip_coef.numel() >= 1 and clip_coef.is_cuda, "clip_coef: a device fp32 scalar (grad_norm(...)[1:2])"
    return clip_coef.data_ptr()


def adamw_ema(table: torch.Tensor, chunk_tensor: torch.Tensor, chunk_off: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float,
              weight_decay: float, step: int, ema_decay: float, grad_scale: float = 1.0, clip_coef: Optional[torch.Tensor] = None) -> None:
    """clip_coef (here and in the three forms below): a device fp32 scalar that multiplies grad_scale inside the kernel (stedm_*_clip)"""
    if clip_coef is not None:
        check(lib().stedm_adamw_ema_clip(table.data_ptr(), chunk_tensor.data_ptr(), chunk_off.data_ptr(), chunk_tensor.numel(), float(lr), float(beta1),
                                         float(beta2), float(eps), float(weight_decay), int(step), float(ema_decay), float(grad_scale),
                                         _coef_ptr(clip_coef), _stream()), "stedm_adamw_ema_clip")
        note_raw_write()
        return
    check(lib().stedm_adamw_ema(table.data_ptr(), chunk_tensor.data_ptr(), chunk_off.data_ptr(), chunk_tensor.numel(), float(lr), float(beta1),
                                float(beta2), float(eps), float(weight_decay), int(step), float(ema_decay), float(grad_scale), _stream()), "stedm_adamw_ema")
    note_raw_write()


def adamw_ema_pack_piece() -> Tuple[int, int]:
    """(rows, ciw): a convolution weight takes (cout / rows) * (cin / ciw) blocks of stedm_adamw_ema_pack"""
    r, c = C.c_int(0), C.c_int(0)
    check(lib().stedm_adamw_ema_pack_piece(C.byref(r), C.byref(c)), "stedm_adamw_ema_pack_piece")
    return r.value, c.value


def adamw_ema_pack(descs: torch.Tensor, ndesc: int, total_blocks: int, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                   step: int, ema_decay: float, grad_scale: float = 1.0, clip_coef: Optional[torch.Tensor] = None) -> None:
    """AdamW + EMA over convolution weights, refreshing their fragment-order packs in the same pass (stedm_adamw_ema_pack)"""
    if clip_coef is not None:
        check(lib().stedm_adamw_ema_pack_clip(descs.data_ptr(), int(ndesc), int(total_blocks), float(lr), float(beta1), float(beta2), float(eps),
                                              float(weight_decay), int(step), float(ema_decay), float(grad_scale), _coef_ptr(clip_coef), _stream()),
              "stedm_adamw_ema_pack_clip")
        note_raw_write()
        return
    check(lib().stedm_adamw_ema_pack(descs.data_ptr(), int(ndesc), int(total_blocks), float(lr), float(beta1), float(beta2), float(eps),
                                     float(weight_decay), int(step), float(ema_decay), float(grad_scale), _stream()), "stedm_adamw_ema_pack")
    note_raw_write()


def adamw_ema_sched(table: torch.Tensor, chunk_tensor: torch.Tensor, chunk_off: torch.Tensor, beta1: float, beta2: float, eps: float, weight_decay: float,
                    sched: torch.Tensor, sched_idx: torch.Tensor, grad_scale: float = 1.0, clip_coef: Optional[torch.Tensor] = None) -> None:
    """stedm_adamw_ema with {bias corrections, EMA decay, learning rate} read from row *sched_idx of sched [n][4] on the device (captured step)"""
    assert sched.dtype == torch.float32 and sched.is_contiguous() and sched.shape[-1] == 4 and sched_idx.dtype == torch.int32
    if clip_coef is not None:
        check(lib().stedm_adamw_ema_sched_clip(table.data_ptr(), chunk_tensor.data_ptr(), chunk_off.data_ptr(), chunk_tensor.numel(), float(beta1),
                                               float(beta2), float(eps), float(weight_decay), sched.data_ptr(), sched_idx.data_ptr(), float(grad_scale),
                                               _coef_ptr(clip_coef), _stream()), "stedm_adamw_ema_sched_clip")
        note_raw_write()
        return
    check(lib().stedm_adamw_ema_sched(table.data_ptr(), chunk_tensor.data_ptr(), chunk_off.data_ptr(), chunk_tensor.numel(), float(beta1), float(beta2),
                                      float(eps), float(weight_decay), sched.data_ptr(), sched_idx.data_ptr(), float(grad_scale), _stream()),
          "stedm_adamw_ema_sched")
    note_raw_write()


def adamw_ema_pack_sched(descs: torch.Tensor, ndesc: int, total_blocks: int, beta1: float, beta2: float, eps: float, weight_decay: float,
                         sched: torch.Tensor, sched_idx: torch.Tensor, grad_scale: float = 1.0, clip_coef: Optional[torch.Tensor] = None) -> None:
    """stedm_adamw_ema_pack with the step-dependent scalars read on the device (see adamw_ema_sched)"""
    assert sched.dtype == torch.float32 and sched.is_contiguous() and sched.shape[-1] == 4 and sched_idx.dtype == torch.int32
    if clip_coef is not None:
        check(lib().stedm_adamw_ema_pack_sched_clip(descs.data_ptr(), int(ndesc), int(total_blocks), float(beta1), float(beta2), float(eps),
                                                    float(weight_decay), sched.data_ptr(), sched_idx.data_ptr(), float(grad_scale), _coef_ptr(clip_coef),
                                                    _stream()), "stedm_adamw_ema_pack_sched_clip")
        note_raw_write()
        return
    check(lib().stedm_adamw_ema_pack_sched(descs.data_ptr(), int(ndesc), int(total_blocks), float(beta1), float(beta2), float(eps), float(weight_decay),
                                           sched.data_ptr(), sched_idx.data_ptr(), float(grad_scale), _stream()), "stedm_adamw_ema_pack_sched")
    note_raw_write()


def ema_update(table: torch.Tensor, chunk_tensor: torch.Tensor, chunk_off: torch.Tensor, ema_decay: float) -> None:
    """LitEma.forward (ema.py:25-44) over the optimizer's pointer table: shadow -= (1 - decay) * (shadow - p)."""
    check(lib().stedm_ema_update(table.data_ptr(), chunk_tensor.data_ptr(), chunk_off.data_ptr(), chunk_tensor.numel(), float(ema_decay), _stream()),
          "stedm_ema_update")


# ------------------------------------------------------------------------------------------- first stage (VQ-f4)
def vq_nearest(z: torch.Tensor, codebook: torch.Tensor):
    """z [B,e,H,W] fp32, codebook [n_e,e] -> (indices int64 [B,H,W], z_q [B,e,H,W] = z + (e_idx - z)); see stedm_vq_nearest."""
    _chk(z, name="z"); _chk(codebook, name="codebook")
    B, e, H, W = z.shape
    assert codebook.shape[1] == e
    idx = torch.empty((B, H, W), dtype=torch.int64, device=z.device)
    zq = torch.empty_like(z)
    check(lib().stedm_vq_nearest(z.data_ptr(), codebook.data_ptr(), codebook.shape[0], e, B, H * W, idx.data_ptr(), zq.data_ptr(), _stream()),
          "stedm_vq_nearest")
    return idx, zq


def conv1x1_nchw(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """1x1 conv over a few channels, NCHW -> NCHW (quant_conv / post_quant_conv)."""
    _chk(x, name="x")
    B, cin, H, W = x.shape
    cout = w.shape[0]
    w2 = w.detach().float().reshape(cout, cin).contiguous()
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    check(lib().stedm_conv1x1_nchw(x.data_ptr(), w2.data_ptr(), _ptr(None if bias is None else bias.detach().float().contiguous()), out.data_ptr(),
                                   B, cin, cout, H * W, _stream()), "stedm_conv1x1_nchw")
    return out


def gauss_sample(moments: torch.Tensor, noise: Optional[torch.Tensor] = None, *, scale: float = 1.0, mode: bool = False, seed: Optional[int] = None,
                 first_id: int = 0) -> torch.Tensor:
    """moments [B,2C,H,W] fp32 (mean | log-variance) -> z [B,C,H,W] = scale * (mean + exp(0.5 clamp(logvar, -30, 20)) noise): the KL
    posterior's sample (distributions.py:24-37) with get_first_stage_encoding's scale (ddpm.py:552) folded in. noise [B,C,H,W], or None:
    drawn in the kernel as row first_id + b of philox_normal(seed, stream STREAM_POSTERIOR), the same bits. mode=True: z = scale * mean,
    nothing read or drawn. See stedm_gauss_sample."""
    _chk(moments, name="moments")
    if moments.dim() != 4 or moments.shape[1] % 2:
        raise ValueError(f"moments must be [B, 2C, H, W], got {tuple(moments.shape)}")
    B, C2, H, W = moments.shape
    C = C2 // 2
    if not mode:
        if noise is not None:
            _chk(noise, name="noise")
            if tuple(noise.shape) != (B, C, H, W):
                raise ValueError(f"noise {tuple(noise.shape)} does not match the sample's shape {(B, C, H, W)}")
        elif seed is None:
            raise ValueError("gauss_sample: give noise, a seed for the in-kernel draw, or mode=True")
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=moments.device)
    check(lib().stedm_gauss_sample(moments.data_ptr(), None if mode else _ptr(noise), out.data_ptr(), B, C, H * W, float(scale), 1 if mode else 0,
                                   int(first_id), int(seed or 0) & 0xFFFFFFFFFFFFFFFF, _stream()), "stedm_gauss_sample")
    return out


def softmax_rows16(x: torch.Tensor, scale: float, hi: torch.Tensor, lo: Optional[torch.Tensor], prec: Precision) -> None:
    """x [rows, n] fp32 (row stride x.stride(0)) -> softmax(scale * x) as 16-bit planes hi (/lo) [rows, ld_out >= n], zero beyond n."""
    assert x.dim() == 2 and x.stride(1) == 1 and hi.dim() == 2 and hi.is_contiguous() and hi.shape[0] == x.shape[0] and hi.shape[1] >= x.shape[1]
    check(lib().stedm_softmax_rows16(x.data_ptr(), x.stride(0), float(scale), hi.data_ptr(), _ptr(lo), x.shape[0], x.shape[1], hi.shape[1],
                                     prec.mm_dtype, _stream()), "stedm_softmax_rows16")


# ------------------------------------------------------------------------------------------- image epilogue
def image_to_uint8(x: torch.Tensor) -> torch.Tensor:
    """((clip(x, -1, 1).permute(0, 2, 3, 1) + 1) * 127.5).astype(uint8) — x [B,C,H,W] fp32 -> [B,H,W,C] uint8 (ldm_diffusion.py:93-95)."""
    _chk(x, name="x")
    B, Cc, H, W = x.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
    check(lib().stedm_image_to_uint8(x.data_ptr(), out.data_ptr(), B, Cc, H, W, _stream()), "stedm_image_to_uint8")
    return out


def seg_merge(seg_nchw: torch.Tensor) -> torch.Tensor:
    """seg [B,K,H,W] one-hot -> [B,H,W,2] = {class 0, sum of the other classes} (prepare_batch, ldm_diffusion.py:52-56)."""
    _chk(seg_nchw, name="segmentation")
    B, K, H, W = seg_nchw.shape
    out = torch.empty((B, H, W, 2), dtype=torch.float32, device=seg_nchw.device)
    check(lib().stedm_seg_merge(seg_nchw.data_ptr(), out.data_ptr(), B, K, H, W, _stream()), "stedm_seg_merge")
    return out


def argmax_u8(seg: torch.Tensor) -> torch.Tensor:
    """torch.argmax(seg, dim=-1) as uint8 (ldm_diffusion.py:98): seg [..., ncls] fp32."""
    _chk(seg, name="seg")
    out = torch.empty(tuple(seg.shape[:-1]), dtype=torch.uint8, device=seg.device)
    check(lib().stedm_argmax_u8(seg.data_ptr(), out.data_ptr(), out.numel(), seg.shape[-1], _stream()), "stedm_argmax_u8")
    return out


# ------------------------------------------------------------------------------------------- patch-distributed first stage
def unfold_tiles(x: torch.Tensor, ks: Tuple[int, int], stride: Tuple[int, int], l0: int = 0, nl: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """crops l0 .. l0+nl-1 (l = ly*Lx + lx, nn.Unfold's order; nl None: all that follow l0) of x [B,C,H,W] fp32 -> [nl,B,C,kh,kw]; see
    stedm_unfold_tiles."""
    _chk(x, name="x")
    B, Cc, H, W = x.shape
    (kh, kw), (sy, sx) = (int(ks[0]), int(ks[1])), (int(stride[0]), int(stride[1]))
    if not (0 < kh <= H and 0 < kw <= W and sy > 0 and sx > 0):
        raise ValueError(f"unfold_tiles: crop {kh} x {kw}, stride {sy} x {sx} over {H} x {W}")
    L = ((H - kh) // sy + 1) * ((W - kw) // sx + 1)
    nl = L - int(l0) if nl is None else int(nl)
    if l0 < 0 or nl < 1 or l0 + nl > L:
        raise ValueError(f"unfold_tiles: crops {l0} .. {l0 + nl - 1} outside 0 .. {L - 1}")
    if out is None:
        out = torch.empty((nl, B, Cc, kh, kw), dtype=torch.float32, device=x.device)
    else:
        _chk(out, name="out")
        if tuple(out.shape) != (nl, B, Cc, kh, kw):
            raise ValueError(f"unfold_tiles: out {tuple(out.shape)} != {(nl, B, Cc, kh, kw)}")
    check(lib().stedm_unfold_tiles(x.data_ptr(), out.data_ptr(), B, Cc, H, W, kh, kw, sy, sx, int(l0), nl, _stream()), "stedm_unfold_tiles")
    return out


def fold_blend(tiles: torch.Tensor, w_tile: torch.Tensor, w_tie: torch.Tensor, stride: Tuple[int, int], grid: Tuple[int, int],
               want_f32: bool = True, want_u8: bool = False):
    """tiles [Ly*Lx,B,C,th,tw] fp32, w_tile [th,tw], w_tie [Ly*Lx], stride (sy, sx) and grid (Ly, Lx) in output pixels ->
    (out [B,C,Ho,Wo] fp32 or None, out_u8 [B,Ho,Wo,C] uint8 or None); see stedm_fold_blend. out_u8 equals image_to_uint8(out) bit for bit."""
    _chk(tiles, name="tiles"); _chk(w_tile, name="w_tile"); _chk(w_tie, name="w_tie")
    L, B, Cc, th, tw = tiles.shape
    (sy, sx), (Ly, Lx) = (int(stride[0]), int(stride[1])), (int(grid[0]), int(grid[1]))
    if Ly < 1 or Lx < 1 or Ly * Lx != L or tuple(w_tile.shape) != (th, tw) or w_tie.numel() != L:
        raise ValueError(f"fold_blend: tiles {tuple(tiles.shape)}, grid {Ly} x {Lx}, w_tile {tuple(w_tile.shape)}, w_tie {tuple(w_tie.shape)} disagree")
    if not (want_f32 or want_u8):
        raise ValueError("fold_blend: nothing to write (want_f32 or want_u8)")
    Ho, Wo = (Ly - 1) * sy + th, (Lx - 1) * sx + tw
    out = torch.empty((B, Cc, Ho, Wo), dtype=torch.float32, device=tiles.device) if want_f32 else None
    out8 = torch.empty((B, Ho, Wo, Cc), dtype=torch.uint8, device=tiles.device) if want_u8 else None
    check(lib().stedm_fold_blend(tiles.data_ptr(), w_tile.data_ptr(), w_tie.data_ptr(), _ptr(out), _ptr(out8), B, Cc, th, tw, sy, sx, Ly, Lx,
                                 _stream()), "stedm_fold_blend")
    return out, out8


# ------------------------------------------------------------------------------------------- graphs
class Graph:
    """hipGraph captured on the current torch stream (all buffers must be allocated beforehand)."""

    def __init__(self):
        self._exec = C.c_void_p()

    def __enter__(self):
        check(lib().stedm_graph_begin(_stream()), "stedm_graph_begin")
        return self

    def __exit__(self, et, ev, tb):
        rc = lib().stedm_graph_end(_stream(), C.byref(self._exec))
        if et is None:
            check(rc, "stedm_graph_end")
        return False

    def launch(self):
        check(lib().stedm_graph_launch(self._exec, _stream()), "stedm_graph_launch")

    def __del__(self):
        try:
            if self._exec:
                lib().stedm_graph_destroy(self._exec)
        except Exception:
            pass
