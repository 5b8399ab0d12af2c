"""HIP-backed denoising U-Net with the reference's module surface.

Drop-in for `ldm.modules.diffusionmodules.openaimodel.UNetModel` (reference openaimodel.py:435-806):
same constructor kwargs, same `forward(x, timesteps, context, y)` contract, same state-dict names
and fp32 OIHW parameter shapes — so reference checkpoints load with `load_state_dict` — but
`forward` runs entirely in hand-written HIP kernels through the C ABI (stedm_amd/ops.py).
torch.nn modules below are *parameter containers*; their own forward is never used.

Internal data layout: activations NHWC fp32 in HBM; conv weights pre-packed 16-bit (hi/lo planes
[cout][tap][cin], or MFMA-fragment order for the register-streamed kernels); GroupNorm statistics
ride on the producing conv's epilogue, and one normalise / SiLU / convert pass writes the 16-bit
operand planes the consuming conv reads; the skip concat is never materialised (that pass reads
two sources).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import BF16, F16, CONV_S2D, CONV_DOWN, CONV_S1, CONV_UP, CONV_UP_SUBPIXEL, StedmHipError
from .ops import Precision


def zero_module(module: nn.Module) -> nn.Module:
    """util.py:174-180."""
    for p in module.parameters():
        p.detach().zero_()
    return module


class GroupNorm32(nn.GroupNorm):
    """util.py:214-216 (container; eps 1e-5, 32 groups)."""


class TimestepBlock(nn.Module):
    """openaimodel.py:64-73 marker: forward(x, emb)."""


class StyleBlock(nn.Module):
    """openaimodel.py:75-84 marker: forward(x, context)."""


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    """openaimodel.py:87-101 (container; routing is done by UNetModel._run_block)."""


class Upsample(nn.Module):
    """openaimodel.py:104-132: nearest x2 then 3x3 conv (fused: the conv's patch loader reads src//2). use_conv=False (conv_resample=False):
    the bare nearest x2, no parameters (stedm_replicate2x2)."""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        assert dims == 2, "only the 2-D form is implemented (shipped configs)"
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv = bool(use_conv)
        if self.use_conv:
            self.conv = nn.Conv2d(self.channels, self.out_channels, 3, padding=padding)


class Downsample(nn.Module):
    """openaimodel.py:147-173: 3x3 stride-2 pad-1 conv. use_conv=False (conv_resample=False): the 2 x 2 average pool, no parameters
    (stedm_avgpool2x2)."""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1):
        super().__init__()
        assert dims == 2, "only the 2-D form is implemented (shipped configs)"
        self.channels = channels
        self.out_channels = out_channels or channels
        self.use_conv = bool(use_conv)
        if self.use_conv:
            self.op = nn.Conv2d(self.channels, self.out_channels, 3, stride=2, padding=padding)
        else:
            assert self.channels == self.out_channels      # openaimodel.py:162
            self.op = nn.AvgPool2d(kernel_size=2, stride=2)


class ResBlock(TimestepBlock):
    """openaimodel.py:176-288. up / down (:220-229, resblock_updown): both branches are resampled without parameters - h_upd = x_upd = the
    conv-less Upsample / Downsample, up wins when both are set - between in_layers' SiLU and its convolution (:268-275); one pass writes the
    resampled activation planes and the resampled input (stedm_gn_apply16c_resample). use_scale_shift_norm (:199, :280-284): emb_layers emits 2 * out_channels values and the block
    computes h = out_norm(h) * (1 + scale) + shift in place of h + emb_out (AdaGN / FiLM). dropout (:241): out_layers[2], live in train();
    drop_site is the block's ordinal in execution order over all ResBlocks of its UNetModel (the mask stream's site, include/stedm_hip.h)."""

    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False, use_scale_shift_norm=False,
                 dims=2, use_checkpoint=False, up=False, down=False):
        super().__init__()
        if dims != 2 or use_conv:
            raise NotImplementedError("ResBlock: use_conv / dims != 2 are not "
                                      "exercised by the reference configs and are not implemented in the HIP path")
        if (up or down) and (out_channels or channels) != channels:
            raise NotImplementedError("ResBlock(up / down) with out_channels != channels: UNetModel never builds one, and the 1x1 skip_connection "
                                      "would need raw 16-bit planes of the resampled input")
        self.channels = channels
        self.emb_channels = emb_channels
        self.dropout = dropout
        self.drop_site = 0
        self.out_channels = out_channels or channels
        self.use_scale_shift_norm = bool(use_scale_shift_norm)
        self.in_layers = nn.Sequential(GroupNorm32(32, channels), nn.SiLU(), nn.Conv2d(channels, self.out_channels, 3, padding=1))
        self.up = bool(up)
        self.down = bool(down) and not self.up       # openaimodel.py:222-229: `if up ... elif down`
        self.updown = self.up or self.down
        if self.up:
            self.h_upd = Upsample(channels, False, dims)
            self.x_upd = Upsample(channels, False, dims)
        elif self.down:
            self.h_upd = Downsample(channels, False, dims)
            self.x_upd = Downsample(channels, False, dims)
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * self.out_channels if use_scale_shift_norm else self.out_channels))
        self.out_layers = nn.Sequential(GroupNorm32(32, self.out_channels), nn.SiLU(), nn.Dropout(p=dropout),
                                        zero_module(nn.Conv2d(self.out_channels, self.out_channels, 3, padding=1)))
        if self.out_channels == channels:
            self.skip_connection = nn.Identity()
        else:
            self.skip_connection = nn.Conv2d(channels, self.out_channels, 1)


class ResBlockStyle(StyleBlock):
    """openaimodel.py:291-297."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.block = ResBlock(*args, **kwargs)


class AttentionBlock(nn.Module):
    """openaimodel.py:300-346. `attn_order`: how the qkv convolution's 3C channels split into heads - 0: QKVAttentionLegacy (heads
    first, :369-394), 1: QKVAttention (q | k | v first, :401-428; use_new_attention_order=True). Same parameters in both."""

    def __init__(self, channels, num_heads=1, num_head_channels=-1, use_checkpoint=False, use_new_attention_order=False):
        super().__init__()
        self.attn_order = ops.ATTN_QKV_FIRST if use_new_attention_order else ops.ATTN_HEADS_FIRST
        self.channels = channels
        if num_head_channels == -1:
            self.num_heads = num_heads
        else:
            assert channels % num_head_channels == 0
            self.num_heads = channels // num_head_channels
        self.norm = GroupNorm32(32, channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = zero_module(nn.Conv1d(channels, channels, 1))

    def order_kw(self) -> dict:
        """keyword arguments of the ops.attn_legacy* calls: none in order 0, so that the default order issues the call it always issued
        (bench.py's AttnTimer and other tools replace ops.attn_legacy16 by a function of its four original arguments)"""
        return {"order": self.attn_order} if self.attn_order != ops.ATTN_HEADS_FIRST else {}


class _Packed:
    __slots__ = ("hi", "lo", "bias", "frag", "frag16")

    def __init__(self, hi, lo, bias, frag=None, frag16=None):
        self.hi, self.lo, self.bias, self.frag, self.frag16 = hi, lo, bias, frag, frag16


class UNetModel(nn.Module):
    """openaimodel.py:435-806. Extra (non-reference) attribute: `precision` (ops.Precision)."""

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False,
                 use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False,
                 resblock_updown=False, use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1,
                 context_dim=None, n_embed=None, legacy=True, style_imgs=1, precision: str = "parity"):
        super().__init__()
        if use_spatial_transformer:
            assert context_dim is not None, "use_spatial_transformer=True needs context_dim (width of the conditioning vector)"
        if context_dim is not None:
            assert use_spatial_transformer, "context_dim is only meaningful with use_spatial_transformer=True"
            if not isinstance(context_dim, int):
                context_dim = list(context_dim)
        if num_classes is not None or n_embed is not None or dims != 2:
            raise NotImplementedError("num_classes / n_embed / dims != 2: "
                                      "not used by the reference configs, not implemented")
        if resblock_updown and not conv_resample:
            raise NotImplementedError("resblock_updown=True with conv_resample=False: the reference ignores conv_resample there (a no-op), but the "
                                      "combination stays refused until the follow-up that lifts it together with the dropout one (DESIGN.md 4.6)")
        if resblock_updown and float(dropout) > 0:
            raise NotImplementedError("resblock_updown=True with dropout > 0: the up / down blocks would take the ordinary drop pass, but the "
                                      "combination stays refused until the follow-up that lifts it together with conv_resample=False (DESIGN.md 4.6)")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        if num_heads == -1:
            assert num_head_channels != -1, "Either num_heads or num_head_channels has to be set"
        if num_head_channels == -1:
            assert num_heads != -1, "Either num_heads or num_head_channels has to be set"

        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = attention_resolutions
        self.dropout = dropout
        self.channel_mult = channel_mult
        self.conv_resample = conv_resample
        self.resblock_updown = bool(resblock_updown)
        self.num_classes = num_classes
        self.use_checkpoint = use_checkpoint
        self.dtype = torch.float32
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.num_heads_upsample = num_heads_upsample
        self.predict_codebook_ids = False
        self.use_scale_shift_norm = bool(use_scale_shift_norm)
        ssn = self.use_scale_shift_norm
        self.precision = Precision.parse(precision) if isinstance(precision, str) else precision

        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(nn.Conv2d(in_channels, model_channels, 3, padding=1))])
        input_block_chans = [model_channels]
        ch, ds = model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                if ds in attention_resolutions:
                    # the reference executes `layers.append()` here (openaimodel.py:580-590) -> TypeError
                    raise TypeError("list.append() takes exactly one argument (0 given) "
                                    "[reference openaimodel.py:580: ds in attention_resolutions is not constructible]")
                self.input_blocks.append(TimestepEmbedSequential(ResBlock(ch, ted, dropout, out_channels=mult * model_channels,
                                                                                  use_scale_shift_norm=ssn)))
                ch = mult * model_channels
                input_block_chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(
                    ResBlock(ch, ted, dropout, out_channels=ch, use_scale_shift_norm=ssn, down=True) if resblock_updown
                    else Downsample(ch, conv_resample, out_channels=ch)))
                input_block_chans.append(ch)
                ds *= 2
        if num_head_channels != -1:
            num_heads = ch // num_head_channels
        # legacy=True (openaimodel.py:624-626): dim_head = ch // num_heads with the spatial transformer, else num_head_channels
        dim_head = ch // num_heads if use_spatial_transformer else num_head_channels
        if use_spatial_transformer:
            from .attention import SpatialTransformer
            mid_attn = SpatialTransformer(ch, num_heads, dim_head, depth=transformer_depth, context_dim=context_dim)
        else:
            mid_attn = AttentionBlock(ch, num_heads=num_heads, num_head_channels=dim_head, use_new_attention_order=use_new_attention_order)
        self.middle_block = TimestepEmbedSequential(
            ResBlock(ch, ted, dropout, use_scale_shift_norm=ssn),
            ResBlockStyle(ch, ted, dropout, use_scale_shift_norm=ssn),
            mid_attn,
            ResBlock(ch, ted, dropout, use_scale_shift_norm=ssn),
        )
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = input_block_chans.pop()
                layers: List[nn.Module] = [ResBlock(ch + ich, ted, dropout, out_channels=model_channels * mult, use_scale_shift_norm=ssn)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    raise TypeError("reference output block with ds in attention_resolutions is not runnable (openaimodel.py:689-698)")
                if level and i == num_res_blocks:
                    layers.append(ResBlock(ch, ted, dropout, out_channels=ch, use_scale_shift_norm=ssn, up=True) if resblock_updown
                                  else Upsample(ch, conv_resample, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = nn.Sequential(GroupNorm32(32, ch), nn.SiLU(), zero_module(nn.Conv2d(model_channels, out_channels, 3, padding=1)))
        for k, rb in enumerate(self._all_resblocks()):
            rb.drop_site = k
        # train-mode dropout (out_layers[2] of every ResBlock, live iff the block is in train() and dropout > 0). The masks are counter-based
        # (include/stedm_hip.h, "train-mode dropout"): seed - None: drawn once from torch's generator at first use, so torch.manual_seed governs
        # it -, site 0x55000000 + drop_site, and a forward counter that UNetTrainer.forward advances by one device launch (eager or captured)
        self.dropout_seed: Optional[int] = None
        self._drop_ctr: Optional[torch.Tensor] = None      # device int32[1]: the forward counter the kernels read
        self._drop_step = 0                                 # its host mirror
        self._drop_used: Dict[int, tuple] = {}              # id(block) -> the drop arguments of the last training forward (the backward's)
        self.last_dropout: Optional[Tuple[int, int]] = None   # (effective seed, step) of the last training forward with live dropout

        # ---- engine state (not part of the state dict)
        self._packed: Dict[int, _Packed] = {}
        self._pack_key = None
        self._bufs: Dict[Tuple, torch.Tensor] = {}
        self._emb_layout: List[Tuple[ResBlock, int]] = []
        self._consts: Dict[str, torch.Tensor] = {}
        self._m16 = True             # 3x3 convs from 256 input channels on v_mfma_f32_16x16x32 (conv_rs.inc RS_3X3M)
        self._gn_slot = 0
        self._style_cache: Dict[Tuple, torch.Tensor] = {}
        self._cs: Dict[int, torch.Tensor] = {}
        self._raw16: Dict[int, Tuple] = {}
        self._saved16: Dict = {}
        self._saved_mr: Dict = {}
        self._mr_ctr = 0
        self._plane_ctr = 0
        self._tape: Optional[list] = None     # training forward (stedm_amd/train.py): one record per layer for the backward pass
        # forward_cfg: the skip half of a decoder concat convolution once per CFG pair (_shared_skip). None: the rule of
        # _shared_skip_rule decides per site; True / False: every admissible site / none
        self.cfg_shared_skip: Optional[bool] = None
        # forward_cfg: the style block's in_layers GroupNorm and convolution once per CFG pair (_shared_front / _res_front). None: the rule of
        # _shared_front_rule decides; True / False: wherever admissible / never
        self.cfg_shared_front: Optional[bool] = None
        # _in_conv: where a routed shared-skip launch splits K two ways, its two partials may go to the 2B launch as res / res2 with no
        # reduce pass. True: wherever that is the case; None / False: never (the reduce pass forms the partial first) - measured on the
        # headline step the form gains nothing, so no rule admits it
        self.cfg_skip_partials: Optional[bool] = None

    # ------------------------------------------------------------------------------------ engine plumbing
    def convert_to_fp16(self):  # openaimodel.py:745-751 — a no-op in the reference too (openaimodel.py:25-29)
        pass

    def convert_to_fp32(self):
        pass

    def set_precision(self, precision) -> None:
        self.precision = Precision.parse(precision) if isinstance(precision, str) else precision
        self.invalidate()

    def invalidate(self) -> None:
        """The parameters' VALUES changed (e.g. in place through raw pointers, without a version bump): the next forward packs again — as one
        multi-tensor launch into the same buffers when the storage is still the same (_prepare), from scratch otherwise."""
        self._style_cache.clear()
        self._consts.clear()
        self._pack_key = None
        self._values_gen = getattr(self, "_values_gen", 0) + 1     # part of the freshness token of packs written by the optimizer kernel

    def check_f16_range(self, where: str = "UNetModel.forward") -> None:
        """Synchronise and raise StedmHipError if any fp16 operand plane written since the last check held an inf / NaN (ops.f16_guard_check).
        The sampling loops call it once at their end; call it after an eager forward in the `f16` / `parity` modes when in doubt."""
        ops.f16_guard_check(where)

    def freshness_token(self, versions=None):
        """What must be unchanged for weight packs written by the optimizer kernel to still be current: every parameter's torch version, this
        model's value generation (invalidate()) and the process-wide count of raw-pointer parameter writes (ops.note_raw_write)."""
        if versions is None:
            versions = tuple(p._version for p in self.parameters())
        return (versions, getattr(self, "_values_gen", 0), ops.raw_write_epoch())

    def _buf(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            dev = next(self.parameters()).device
            t = torch.empty(tuple(shape), dtype=dtype, device=dev)
            self._bufs[key] = t
        return t

    def _timestep_blocks(self) -> List[ResBlock]:
        """ResBlocks conditioned on the timestep embedding, in execution order."""
        out = []
        for blk in list(self.input_blocks) + [self.middle_block] + list(self.output_blocks):
            for layer in blk:
                if isinstance(layer, ResBlock):
                    out.append(layer)
        return out

    def _all_resblocks(self) -> List[ResBlock]:
        """Every ResBlock in execution order, the inner block of ResBlockStyle included: the order of the dropout sites."""
        out = []
        for blk in list(self.input_blocks) + [self.middle_block] + list(self.output_blocks):
            for layer in blk:
                if isinstance(layer, ResBlock):
                    out.append(layer)
                elif isinstance(layer, ResBlockStyle):
                    out.append(layer.block)
        return out

    @staticmethod
    def _drop_live(rb: ResBlock) -> bool:
        return bool(rb.training and rb.dropout > 0)

    def dropout_live(self) -> bool:
        """Is train-mode dropout live in any ResBlock (the block in train() and dropout > 0)?"""
        return self.dropout > 0 and any(self._drop_live(rb) for rb in self._all_resblocks())

    @staticmethod
    def rank_dropout_seed(seed: int, rank: int) -> int:
        """The seed rank `rank` uses under torch.distributed, so that ranks do not drop the same pattern on their shards"""
        return (int(seed) ^ ((int(rank) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF

    def set_dropout_step(self, step: int) -> None:
        """Set the forward counter (device word and host mirror): the next training forward advances it and uses step + 1."""
        dev = next(self.parameters()).device
        step = int(step) & 0xFFFFFFFF
        if self._drop_ctr is None or self._drop_ctr.device != dev:
            self._drop_ctr = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._drop_ctr.fill_(step - (1 << 32) if step >= (1 << 31) else step)
        self._drop_step = step

    def _dropout_seed_now(self) -> int:
        """dropout_seed, drawn from torch's generator first when it is still None (once: it stays)"""
        if self.dropout_seed is None:
            self.dropout_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        return self.dropout_seed

    def _dropout_begin(self) -> None:
        """Start of a training forward with live dropout: one launch advances the device counter (the same launch eager or captured), the
        host mirror follows, and the seed is fixed (drawn once when dropout_seed is None)."""
        import torch.distributed as dist
        if self._drop_ctr is None or self._drop_ctr.device != next(self.parameters()).device:
            self.set_dropout_step(self._drop_step)
        seed = self._dropout_seed_now()
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        ops.step_advance(self._drop_ctr, 1)
        self._drop_step = (self._drop_step + 1) & 0xFFFFFFFF
        self.last_dropout = (self.rank_dropout_seed(seed, rank), self._drop_step)

    def _drop_args(self, rb: ResBlock) -> tuple:
        """(p, seed, site, step, step_ptr) of a live block for ops.gn_apply16c_drop / ops.gn_bwd_drop: the step is read from the device counter"""
        return (float(rb.dropout), self.last_dropout[0], 0x55000000 + rb.drop_site, 0, self._drop_ctr)

    def _emb_columns(self) -> Tuple[List[Tuple[ResBlock, int]], int]:
        """([(block, first column)], columns) of the concatenated emb_layers projection: every timestep block takes the width of its own
        emb_layers[1] - out_channels, or 2 * out_channels = [scale | shift] for a scale-shift-norm block."""
        layout, off = [], 0
        for rb in self._timestep_blocks():
            layout.append((rb, off))
            off += rb.emb_layers[1].out_features
        return layout, off

    def _prepare(self) -> None:
        """(Re)pack weights when any parameter changed (cheap version fingerprint)."""
        params = list(self.parameters())
        dev = params[0].device
        if dev.type != "cuda":
            raise StedmHipError("UNetModel.forward needs its parameters on the GPU; there is no CPU fallback")
        ptrs = tuple(p.data_ptr() for p in params)
        key = (self.precision, dev, tuple(p._version for p in params), ptrs)
        if key == self._pack_key:
            return
        prec = self.precision
        if prec.mm_dtype == F16:
            ops.f16_guard_enable()        # fp16 operand planes: the kernels flag an overflow, the sampling loops / check_f16_range() raise
        # Same storage, new values (an optimizer step): the fragment-order packs recorded last time run again as ONE launch into the same
        # tensors (ops.PackPlan); the few other packs below are redone as before. Anything else: pack from scratch and record.
        ptr_key = (prec, dev, ptrs, self._m16)
        plan = getattr(self, "_plan", None)
        replay = plan is not None and self._plan_key == ptr_key and len(self._packed) > 0
        if not replay:
            self._packed.clear()
            plan = self._plan = ops.PackPlan(prec)
            self._plan_key = ptr_key
        self._consts.clear()
        self._style_cache.clear()

        def pack(conv):
            if replay:
                pk = self._packed[id(conv)]
                if isinstance(pk.hi, ops.LazyPlanes):
                    pk.hi.reset()
                else:
                    pk.hi, pk.lo = ops.pack_conv_weight(conv.weight.float(), prec)
                    if pk.frag16 is not None:     # 3-product mode: the hi + lo fragment streams
                        wf = conv.weight.detach().float()
                        pk.frag16 = ops.pack_conv_weight_frag16((wf.unsqueeze(-1) if wf.dim() == 3 else wf).contiguous(), prec)
                return
            hi = lo = frag = None
            w4 = conv.weight.detach().float()
            if w4.dim() == 3:     # Conv1d qkv / proj_out of the AttentionBlock
                w4 = w4.unsqueeze(-1)
            in_place = w4.is_contiguous() and w4.data_ptr() == conv.weight.data_ptr()    # the plan re-reads the parameter's own storage
            if not in_place:
                self._plan_key = None
            k3 = tuple(w4.shape[2:]) == (3, 3) and conv.stride == (1, 1) and conv.in_channels % 16 == 0
            k1 = tuple(w4.shape[2:]) == (1, 1) and conv.in_channels % 64 == 0
            frag16 = None
            if prec.npass == 1 and (k3 or k1):
                # register-streamed weights, packed in the fragment order of the MFMA shape the dispatcher will pick: 16x16x32 for a 3x3 from
                # 256 input channels on (conv_rs.inc RS_3X3M), 32x32x16 otherwise; a 1x1 (skip_connection, qkv, proj_out) gets both: fused
                # into an RS_3X3M launch it is read in the 16x16x32 order, on its own in the other
                m16 = self._m16 and conv.in_channels % 32 == 0 and (k1 or conv.in_channels >= 256)
                if not (m16 and k3):
                    frag = plan.frag_oihw(w4, False) if in_place else ops.pack_conv_weight_frag(w4, prec)
                if m16:
                    frag16 = plan.frag_oihw(w4, True) if in_place else ops.pack_conv_weight_frag16(w4, prec)
                # the [cout][tap][cin] planes are read only by the LDS-operand kernels: packed on first need
                hi = ops.LazyPlanes(lambda w=conv.weight: ops.pack_conv_weight(w.float(), prec))
            elif prec.npass == 1 and conv.stride == (2, 2) and conv.in_channels % 8 == 0:
                # Downsample.op: runs as the space-to-depth form below; the plain planes serve odd sizes only
                hi = ops.LazyPlanes(lambda w=conv.weight: ops.pack_conv_weight(w.float(), prec))
            else:
                hi, lo = ops.pack_conv_weight(conv.weight.float(), prec)
                if prec.npass == 3 and self._m16 and conv.in_channels % 32 == 0 and (
                        (k3 and conv.in_channels >= 128) or (tuple(w4.shape[2:]) == (1, 1) and conv.in_channels >= 64)):
                    # 3-product mode on the register-streamed kernel (conv_rs.inc P3: 3x3, and 1x1 = RS_1X1M): hi + lo fragment streams; the
                    # planes above stay for the problems it does not take
                    frag16 = ops.pack_conv_weight_frag16(w4.contiguous(), prec)
            self._packed[id(conv)] = _Packed(hi, lo, None if conv.bias is None else conv.bias.detach().float().contiguous(), frag, frag16)

        for m in self.modules():
            if isinstance(m, ResBlock):
                pack(m.in_layers[2])
                pack(m.out_layers[3])
                if not isinstance(m.skip_connection, nn.Identity):
                    pack(m.skip_connection)
            elif isinstance(m, (Downsample, Upsample)) and not m.use_conv:
                pass          # conv_resample=False: the pool and the nearest x2 have no weights
            elif isinstance(m, Downsample):
                pack(m.op)
                if prec.npass == 1 and m.op.in_channels % 8 == 0:
                    # stride-2 conv as a stride-1 2x2 conv over space-to-depth planes (register-streamed kernel)
                    self._packed[(id(m.op), "s2d")] = _Packed(None, None, self._packed[id(m.op)].bias,
                                                              ops.pack_conv_weight_s2d_frag(m.op.weight.float(), prec))
                elif prec.npass == 3 and self._m16 and m.op.in_channels % 32 == 0:
                    # ... in the 3-product modes with hi + lo planes and fragment streams (conv_rs.inc RS_SUBM)
                    self._packed[(id(m.op), "s2d")] = _Packed(None, None, self._packed[id(m.op)].bias, None,
                                                              ops.pack_conv_weight_s2d_frag16_hl(m.op.weight.float(), prec))
            elif isinstance(m, Upsample):
                pack(m.conv)
                # sub-pixel form: 4 parity 2x2 convs with pre-summed taps
                frag = ops.pack_conv_weight_up_frag(m.conv.weight.float(), prec) if prec.npass == 1 and m.conv.in_channels % 32 == 0 else None
                if frag is not None:     # the planes are read only when a problem falls to the LDS-operand kernel: packed on first need
                    hi, lo = ops.LazyPlanes(lambda w=m.conv.weight: ops.pack_conv_weight_up(w.float(), prec)), None
                else:
                    hi, lo = ops.pack_conv_weight_up(m.conv.weight.float(), prec)
                # 16x16x32 fragment order (RS_SUBM): the 3-product modes (single product: the 32x32x16 RS_SUB form measured faster)
                frag16 = (ops.pack_conv_weight_up_frag16_hl(m.conv.weight.float(), prec)
                          if prec.npass == 3 and self._m16 and m.conv.in_channels % 32 == 0 and m.conv.in_channels >= 128 else None)
                self._packed[(id(m.conv), "up")] = _Packed(hi, lo, self._packed[id(m.conv)].bias, frag, frag16)
            elif isinstance(m, AttentionBlock):
                pack(m.qkv)
                pack(m.proj_out)
            elif type(m).__name__ == "SpatialTransformer":
                self._packed[id(m)] = m.pack(prec)
        if replay:
            plan.run(versions=self.freshness_token(key[2]))
        c = self._consts
        half = self.model_channels // 2
        # host-built frequency table (util.py:162-164 builds it on the CPU in fp32)
        fq = getattr(self, "_freqs", None)        # (kept across re-packs: a host-to-device copy has no place in a captured training step)
        if fq is None or fq.device != dev or fq.numel() != half:
            fq = self._freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).to(dev)
        c["freqs"] = fq
        c["te_w0t"] = ops.transpose(self.time_embed[0].weight.float())
        c["te_b0"] = self.time_embed[0].bias.detach().float().contiguous()
        c["te_w2t"] = ops.transpose(self.time_embed[2].weight.float())
        c["te_b2"] = self.time_embed[2].bias.detach().float().contiguous()
        # all timestep emb_layers concatenated along N (SiLU -> Linear, openaimodel.py:231-237)
        tblocks = self._timestep_blocks()
        self._emb_layout, off = self._emb_columns()
        wcat = torch.cat([rb.emb_layers[1].weight.detach().float() for rb in tblocks], dim=0)  # [Ntot, ted]
        c["emb_w"] = wcat.contiguous()                          # [Ntot][ted]: K-major operand of the embedding path's backward
        c["emb_wt"] = ops.transpose(c["emb_w"])
        c["emb_b"] = torch.cat([rb.emb_layers[1].bias.detach().float() for rb in tblocks]).contiguous()
        self._emb_off = {id(rb): o for rb, o in self._emb_layout}
        self._emb_ntot = off
        srb = self.middle_block[1].block
        c["out_w_hwio"] = ops.conv_out_weight(self.out[2].weight)   # conv_out reads [3][3][c][4|8]
        c["style_wt"] = ops.transpose(srb.emb_layers[1].weight.float())
        c["style_b"] = srb.emb_layers[1].bias.detach().float().contiguous()
        self._pack_key = key

    # ------------------------------------------------------------------------------------ block runners (NHWC)
    # ---- 16-bit operand planes ---------------------------------------------------------------------------------
    def _planes(self, B, H, W, C, kind="a16"):
        hi = self._buf(f"{kind}hi.{B}x{H}x{W}x{C}", (B, H, W, C), torch.int16)
        lo = self._buf(f"{kind}lo.{B}x{H}x{W}x{C}", (B, H, W, C), torch.int16) if self.precision.npass == 3 else None
        return hi, lo

    # Split-K workspace (small grids only) for an output of `nel` fp32 elements. Two rules, tuned separately: keep them apart.
    def _splitk_ws_res(self, nel: int) -> Optional[torch.Tensor]:
        """ResBlock convolutions: room for up to 16 partial tiles when the tensor is small, 4 or 2 above that, none above 2^23 elements"""
        if nel > (1 << 23):
            return None
        return self._buf("conv_ws", ((16 if nel <= (1 << 20) else (4 if nel <= (1 << 22) else 2)) * nel,))

    def _splitk_ws(self, nel: int) -> torch.Tensor:
        """proj_out, Downsample, Upsample: room for up to 16 partial tiles when the tensor is small, 2 otherwise"""
        return self._buf("conv_ws", ((16 if nel <= (1 << 20) else 2) * nel,))

    # Producer-side GroupNorm statistics: tensors written by a conv epilogue carry per-(sample, slab, channel) partial sums
    # (stedm_conv_args.chan_stats); tensors from other producers get them lazily from one stedm_gn_chan_stats pass. One set of
    # partials serves every GroupNorm that reads the tensor (next block, decoder concat with its straddling groups).
    def _cs_new(self, t: torch.Tensor, nslab: Optional[int] = None) -> torch.Tensor:
        """statistics buffer of tensor `t` ([B][nslab][C][2]; any partition of a sample's pixels into nslab slots serves)"""
        B, C = t.shape[0], t.shape[-1]
        HW = t.numel() // (B * C)
        cs = self._buf(f"cs.{t.data_ptr()}", (B, nslab or ops.gn_chan_nslab(HW), C, 2))
        self._cs[t.data_ptr()] = cs
        return cs

    def _chan_stats(self, t: torch.Tensor) -> torch.Tensor:
        cs = self._cs.get(t.data_ptr())
        if cs is None:
            cs = self._cs_new(t)
            ops.gn_chan_stats(t, cs)
        return cs

    def _norm16(self, norm: Optional[nn.GroupNorm], act: int, x1, x2=None, x2_bmod=0, want_raw=False):
        """act(GroupNorm([x1|x2])) (norm None: plain conversion) written once as 16-bit planes. want_raw: also return the
        plain conversion of [x1|x2] (operand of the 1x1 skip_connection) produced by the same pass."""
        B, H, W, _ = x1.shape
        C = x1.shape[-1] + (0 if x2 is None else x2.shape[-1])
        pre = self._pre16.pop(x1.data_ptr(), None) if self._pre16 else None
        if pre is not None and norm is not None and pre[0] == id(norm) and pre[1] == act and x2 is None and not want_raw and self._tape is None:
            return pre[2]          # the producing convolution's call wrote this GroupNorm's planes already (_res: next_norm)
        x16 = self._x16.pop(x1.data_ptr(), None)
        if x16 is not None:
            # x1 was never stored in fp32: its producer wrote the 16-bit values into channels [0, c1) of this block's raw plane and left the
            # channel statistics (conv_igemm out16_stride); the pass reads 2 B per element of that half and writes its normalised plane only
            rawp, c1 = x16
            assert norm is not None and want_raw and tuple(rawp.shape) == (B, H, W, C) and c1 == x1.shape[-1]
            hi = self._planes(B, H, W, C)[0]
            ops.gn_apply16c_x16(c1, self._cs[x1.data_ptr()], x2, None if x2 is None else self._chan_stats(x2), hi, rawp, self.precision,
                                norm.weight, norm.bias, norm.eps, norm.num_groups, act, x2_bmod)
            return (hi, None), (rawp, None)
        if norm is None:
            hi, lo = self._planes(B, H, W, C)
            ops.gn_apply16(x1, x2, hi, lo, self.precision, x2_bmod=x2_bmod)
            return hi, lo
        (hi, lo), raw, mr = self._keep(norm, x1, (B, H, W, C), want_raw=want_raw)
        self._gn_site(norm, act, x1, x2, x2_bmod, hi=hi, lo=lo, prec=self.precision, raw=raw, mean_rstd=mr)
        return ((hi, lo), raw) if want_raw else (hi, lo)

    def _keep(self, norm: nn.GroupNorm, x, shape, kind="a16", want_raw=False):
        """(planes, raw, mean_rstd) a normalise site of `norm` over x writes: THE statement of what a forward keeps for the backward
        (UNetTrainer._kept16 / _kept_mr read it back). A training forward in the backward's operand format (bf16 single product) gives each
        normalised plane - and, with want_raw, the plain conversion beside it - its own buffer, kept for the weight-gradient pass instead of
        being recomputed there; every training forward keeps the group statistics the pass folds (the backward needs them again).
        Otherwise: the shape-keyed buffers of `kind` (raw: "raw16"), and no statistics buffer."""
        B, H, W, C = shape
        key = (id(norm), x.data_ptr())
        keep = self._tape is not None and self.precision.npass == 1 and self.precision.mm_dtype == BF16
        if keep:
            self._plane_ctr += 1
            planes = self._saved16[key] = self._planes(B, H, W, C, f"keep{self._plane_ctr}.a16")
        else:
            planes = self._planes(B, H, W, C, kind)
        raw = None
        if want_raw and keep:
            raw = self._saved16[("raw", x.data_ptr())] = self._planes(B, H, W, C, f"keep{self._plane_ctr}.raw16")
        elif want_raw:
            raw = self._planes(B, H, W, C, "raw16")
        mr = None
        if self._tape is not None:
            self._mr_ctr += 1
            mr = self._saved_mr[key] = self._buf(f"keep{self._mr_ctr}.mr", (B, norm.num_groups, 2))
        return planes, raw, mr

    def _gn_site(self, norm: nn.GroupNorm, act: int, x1, x2=None, x2_bmod=0, *, hi, lo, prec, raw=None, mean_rstd=None, film=None, film_off=0,
                 film_bstride=0, drop=None, resample=0, xr=None) -> None:
        """One normalise site, act(GroupNorm([x1|x2]) [* (1 + scale) + shift] [dropout]) [resampled], into the 16-bit planes hi (/ lo) in
        format `prec` - the forward with its own precision and the outputs of _keep, the backward's recompute with its own. The library pass:
        resample (1: 2 x 2 average pool, 2: nearest x2; the front of an up / down ResBlock, openaimodel.py:268-275; xr: x1 resampled the
        same way, the block's residual, from the same read) -> gn_apply16c_resample; drop (_drop_args: the block's dropout is live - the
        pass masks and scales the activation; film may be None) -> gn_apply16c_drop; film (scale | shift = columns [film_off, film_off + 2 C)
        of sample b's row, row stride film_bstride, 0: one shared row) -> gn_apply16c_film; else gn_apply16c."""
        w, b, eps, G = norm.weight, norm.bias, norm.eps, norm.num_groups
        if resample:
            assert x2 is None and film is None and drop is None and raw is None
            ops.gn_apply16c_resample(x1, self._chan_stats(x1), hi, lo, prec, w, b, resample, eps, G, act, xr=xr, mean_rstd=mean_rstd)
        elif drop is not None:
            ops.gn_apply16c_drop(x1, self._chan_stats(x1), hi, lo, prec, w, b, drop, eps, G, act, mean_rstd=mean_rstd, film=film,
                                 film_off=film_off, film_bstride=film_bstride)
        elif film is not None:
            ops.gn_apply16c_film(x1, self._chan_stats(x1), hi, lo, prec, w, b, film, film_off, film_bstride, eps, G, act, mean_rstd=mean_rstd)
        else:
            ops.gn_apply16c(x1, self._chan_stats(x1), x2, None if x2 is None else self._chan_stats(x2), hi, lo, prec, w, b, eps, G, act,
                            x2_bmod, raw, mean_rstd=mean_rstd)

    def _gn_next(self, norm: nn.GroupNorm, act: int, planes, mr, only: bool) -> tuple:
        """conv_igemm's gn_next: `norm` + act of the launch's output ride on it, into `planes` - the (hi, lo) pair in the 3-product modes, the
        hi plane otherwise - with the group statistics into mr (or None); only: nothing else reads the output, its fp32 store is skipped"""
        return (norm.weight, norm.bias, norm.eps, norm.num_groups, act, planes if self.precision.npass == 3 else planes[0], mr, only)

    def _asked(self, key: tuple, ask):
        """the answer filed in _consts under `key`, asked (ask()) the first time: the library is asked once per shape whether it takes a launch"""
        hit = self._consts.get(key)
        if hit is None:
            hit = self._consts[key] = ask()
        return hit

    def _coop_for(self, site: str, B, H, W, co, prec):
        """(words, state) for stedm_conv_args.gn_coop at call site `site`, or None: a sample of 2 .. 4 tiles at 128 channels on a grid that fills
        the chip (smaller ones split K or take other kernels and end with the pass anyway), single product. The first use in a forward advances
        the epoch: a device word, moved by a one-thread launch so that a replayed graph moves it too."""
        if not (prec.npass == 1 and co == 128 and 256 < H * W <= 1024 and B * H * W // 256 >= ops.device_cus() and not os.environ.get("STEDM_NO_GN_COOP")):
            return None
        ck = (site, B)
        words = self._coop_bufs.get(ck)
        if words is None:
            words = self._coop_bufs[ck] = torch.zeros((B, 4, 128, 2), dtype=torch.int64, device=self._coop_state.device)
        if not self._coop_advanced:
            ops.step_advance(self._coop_state, 1)
            self._coop_advanced = True
        return words, self._coop_state

    def _cat_plane(self, B, H, W, co, next_cat):
        """The raw plane [B,H,W,next_cat] of the NEXT block's concat input, whose channels [0, co) a producer fills (two buffers per shape in
        turn: the block that writes the next one's plane is still reading its own through the fused skip_connection)."""
        self._catpp ^= 1
        return self._buf(f"cat16.{self._catpp}.{B}x{H}x{W}x{next_cat}", (B, H, W, next_cat), torch.int16)

    def _res(self, tag: str, rb: ResBlock, x1, x2, emb_all, emb_off, emb_bstride, x2_bmod=0, want16=False, next_cat=None, next_norm=None):
        """ResBlock._forward openaimodel.py:268-288 on NHWC tensors; [x1|x2] is the virtual concat input.
        next_cat (inference, single product): the channel count of the NEXT block's th.cat([h, hs.pop()]) input (openaimodel.py:800) when nothing
        but that block's GroupNorm and skip_connection read this block's output: the tail convolution then writes it as 16-bit values straight
        into that concat's raw plane and stores no fp32 tensor (the returned tensor is only the handle the statistics are filed under)."""
        prec = self.precision
        B, H, W, _ = x1.shape
        co = rb.out_channels
        pk = self._packed[id(rb.in_layers[2])]
        has_skip = not isinstance(rb.skip_connection, nn.Identity)
        xres = x1                      # the residual of a block without a skip_connection convolution
        if rb.updown:
            # openaimodel.py:268-275: one pass leaves in_layers' activation planes and the input at the NEW resolution, which is H, W from here on
            # (ops.gn_apply16c_resample: both from one read of x1)
            assert x2 is None and not has_skip
            H, W = (2 * H, 2 * W) if rb.up else (H // 2, W // 2)
            a16, _, mr = self._keep(rb.in_layers[0], x1, (B, H, W, x1.shape[-1]))
            xres = self._buf(f"xr.{B}x{H}x{W}x{x1.shape[-1]}", (B, H, W, x1.shape[-1]))
            self._gn_site(rb.in_layers[0], 1, x1, hi=a16[0], lo=a16[1], prec=prec, mean_rstd=mr, resample=2 if rb.up else 1, xr=xres)
        # training keeps every block's intermediate (the backward pass reads it); inference shares one buffer per shape
        h = self._buf(tag + ".h" if self._tape is not None else f"h.{B}x{H}x{W}x{co}", (B, H, W, co))
        self._last_h = h
        h16_next = gn_next = None
        if has_skip:
            a16, x16 = self._norm16(rb.in_layers[0], 1, x1, x2, x2_bmod, want_raw=True)
        elif not rb.updown:
            a16 = self._norm16(rb.in_layers[0], 1, x1, x2, x2_bmod)
        ws = self._splitk_ws_res(B * H * W * co)
        # out_layers' GroupNorm + SiLU of h rides on this call (inference, single product): where the convolution splits K, the reduce pass
        # that sums the partial tiles owns whole groups of a sample and writes the normalised planes itself; otherwise the call ends with the
        # same stedm_gn_apply16c pass as before
        gn2 = rb.out_layers[0]
        # A scale-shift-norm block (FiLM): the embedding row does not add onto h (no epilogue term) but modulates out_layers' GroupNorm per
        # sample, so none of the producer-side forms of that GroupNorm applies (gn_next in the epilogue / reduce pass, gn_coop, the
        # 16-bit-only h): the convolution writes fp32 h and its statistics, and one stedm_gn_apply16c_film pass writes the planes (_gn_site)
        # Live dropout (train(), dropout > 0) sits between that GroupNorm's SiLU and the 16-bit rounding: the same treatment - fp32 h and its
        # statistics, then one stedm_gn_apply16c_drop / _film_drop pass; the embedding row still adds onto h in the epilogue of a plain block
        film = rb.use_scale_shift_norm
        drop = None
        if self._tape is not None and self._drop_live(rb):
            drop = self._drop_used[id(rb)] = self._drop_args(rb)
        if not film and drop is None and ((prec.npass == 1 and (self._tape is None or prec.mm_dtype == BF16)) or (prec.npass == 3 and self._tape is None)):
            # inference: NOT the planes _norm16 would hand out ("g16"): for cin == cout those are the planes this convolution is reading, and
            # an epilogue that writes the GroupNorm output would overwrite rows other tiles still gather
            h16_next, _, mr2 = self._keep(gn2, h, (B, H, W, co), "g16")
            # (inference: nothing but that GroupNorm reads h — an epilogue that writes the planes itself skips h's fp32 store)
            gn_next = self._gn_next(gn2, 1, h16_next, mr2, self._tape is None)
        done1 = False
        # (where a sample spans 2 .. 4 tiles - 32 x 32 pixels at 128 channels - the tiles exchange their channel sums inside the launch
        #  and the GroupNorm still rides on the epilogue: stedm_conv_args.gn_coop; one word block per call site)
        coop = self._coop_for(tag, B, H, W, co, prec) if gn_next is not None and self._tape is None else None
        coop_runs = coop is not None
        if (gn_next is not None and self._tape is None and prec.npass == 1 and prec.mm_dtype == BF16 and H * W > 256 and B >= 8 and not coop_runs and
                not os.environ.get("STEDM_NO_H16ONLY") and ops.gn_apply16c_x16_ok(co, 0, gn2.num_groups)):
            # Levels whose samples exceed a tile (32 x 32 and up): out_layers' GroupNorm cannot ride on the epilogue and nothing else reads h, so
            # the convolution stores h as 16-bit values only (+ the channel statistics) and the GroupNorm pass reads 2 B per element.
            # bf16 mode only: in f16 - the mode that carries the 1e-3 tolerance - the extra rounding in front of five more GroupNorms moved the
            # forward's rel-L2 from 7.55e-4 to 7.86e-4 for +0.5 % of a step (6.165 -> 6.135 ms); the margin is worth more
            hraw = self._buf(f"h16raw.{B}x{H}x{W}x{co}", (B, H, W, co), torch.int16)
            kw1 = dict(prec=prec, src16=a16, bias=pk.bias, emb=emb_all, emb_offset=emb_off, emb_bstride=emb_bstride, w_frag=pk.frag,
                       chan_stats=self._cs_new(h), ws=ws, w_frag16=pk.frag16, out16=(hraw, None), out16_stride=co, cout=co)
            if self._asked(("h16only", id(rb), B, H, W), lambda: bool(ops.conv_igemm(None, pk.hi, pk.lo, None, query_rs=True, **kw1))):
                ops.conv_igemm(None, pk.hi, pk.lo, None, **kw1)
                ops.gn_apply16c_x16(co, self._cs[h.data_ptr()], None, None, h16_next[0], hraw, prec, gn2.weight, gn2.bias, gn2.eps, gn2.num_groups, 1)
                done1 = True
        if not done1:
            kw1 = dict(prec=prec, bias=pk.bias, emb=None if film else emb_all, emb_offset=emb_off, emb_bstride=emb_bstride, w_frag=pk.frag,
                       chan_stats=self._cs_new(h), ws=ws, w_frag16=pk.frag16, gn_next=gn_next, coop=coop)
            self._in_conv(tag, rb, pk, a16, x1.shape[-1], x2_bmod if x2 is not None else 0, h, kw1)
        if film or drop is not None:
            h16_next, _, mr2 = self._keep(gn2, h, (B, H, W, co), "g16")
            self._gn_site(gn2, 1, h, hi=h16_next[0], lo=h16_next[1], prec=prec, mean_rstd=mr2, film=emb_all if film else None, film_off=emb_off,
                          film_bstride=emb_bstride, drop=drop)
        out = self._buf(tag + ".out", (B, H, W, co))
        pk2 = self._packed[id(rb.out_layers[3])]
        o16 = None
        if want16:     # the consumer (Upsample) reads plain 16-bit planes: the conv epilogue writes them, no conversion pass
            o16 = self._planes(B, H, W, co, "up16")
            self._raw16[out.data_ptr()] = o16
        # next_norm = (GroupNorm32, act) of the layer that reads this block's output alone (the next ResBlock's in_layers without a
        # skip_connection convolution, an AttentionBlock's norm): the tail convolution's call writes that GroupNorm's planes too - in its
        # epilogue / split-K reduce pass where a workgroup owns whole groups of whole samples, by the same trailing pass otherwise - and
        # _norm16 hands them out instead of running its own pass (inference)
        gnn, npl, coop2 = None, None, None
        if next_norm is not None and self._tape is None and o16 is None and next_cat is None and not os.environ.get("STEDM_NO_NEXT_GN"):
            npl = self._planes(B, H, W, co)
            gnn = self._gn_next(*next_norm, npl, None, False)
            coop2 = self._coop_for(tag + ".c2", B, H, W, co, prec)     # (32 x 32 at 128 channels: the in-launch hand-off, as for out_layers' GroupNorm)

        def filed():
            if gnn is not None:
                self._pre16[out.data_ptr()] = (id(next_norm[0]), next_norm[1], npl)
            return out
        if has_skip:
            # conv2 + skip_connection(x) in one kernel when the register-streamed kernel covers the problem (asked once per shape)
            ps = self._packed[id(rb.skip_connection)]
            h16 = h16_next if h16_next is not None else self._norm16(rb.out_layers[0], 1, h)
            kw = dict(prec=prec, src16=h16, bias=pk2.bias, w_frag=pk2.frag, chan_stats=self._cs_new(out), ws=ws, out16=o16, w_frag16=pk2.frag16)
            kwf = dict(kw, skip=(x16[0], ps.frag, ps.bias, ps.frag16))
            fused = self._asked(("fuse", id(rb), B, H, W), lambda: bool((pk2.frag is not None or pk2.frag16 is not None) and ps.frag is not None and
                                                                        ops.conv_igemm(None, pk2.hi, pk2.lo, out, query_fused=True, **kwf)))
            if fused and next_cat is not None and o16 is None:
                rawn = self._cat_plane(B, H, W, co, next_cat)
                kwc = dict(kwf, out16=(rawn, None), out16_stride=next_cat, cout=co)
                if self._asked(("fusecat", id(rb), B, H, W, next_cat), lambda: bool(ops.conv_igemm(None, pk2.hi, pk2.lo, None, query_fused=True, **kwc))):
                    ops.conv_igemm(None, pk2.hi, pk2.lo, None, **kwc)
                    self._x16[out.data_ptr()] = (rawn, co)
                    return out
            if fused and o16 is not None and self._tape is None and prec.npass == 1:
                # inference: the Upsample that follows reads the 16-bit planes only — the fp32 tensor and its statistics need not be written.
                # A launch that splits K (small grids) has to write the fp32 tensor, though: asked once per shape
                kw16 = dict(kwf, chan_stats=None)
                if self._asked(("fuse16", id(rb), B, H, W), lambda: bool(ops.conv_igemm(None, pk2.hi, pk2.lo, None, query_fused=True, **kw16))):
                    # (`out` stays the handle the planes are filed under)
                    self._cs.pop(out.data_ptr(), None)          # (no statistics are written for the handle: nothing may find a buffer for it)
                    ops.conv_igemm(None, pk2.hi, pk2.lo, None, **kw16)
                    return out
            if fused:
                ops.conv_igemm(None, pk2.hi, pk2.lo, out, gn_next=gnn, **kwf)
            else:
                ops.conv_igemm(None, ps.hi, ps.lo, out, prec=prec, ks=1, src16=x16, bias=ps.bias, w_frag=ps.frag, ws=ws,
                               w_frag16=ps.frag16 if prec.npass == 3 else None)
                ops.conv_igemm(None, pk2.hi, pk2.lo, out, res=out, gn_next=gnn, **kw)
            return filed()
        # no skip_connection convolution: the residual is the block's input itself
        assert x2 is None
        h16 = h16_next if h16_next is not None else self._norm16(rb.out_layers[0], 1, h)
        if next_cat is not None and o16 is None:
            rawn = self._cat_plane(B, H, W, co, next_cat)
            kwc = dict(prec=prec, src16=h16, bias=pk2.bias, res=xres, w_frag=pk2.frag, chan_stats=self._cs_new(out), ws=ws, w_frag16=pk2.frag16,
                       out16=(rawn, None), out16_stride=next_cat, cout=co)
            if self._asked(("rescat", id(rb), B, H, W, next_cat), lambda: bool(ops.conv_igemm(None, pk2.hi, pk2.lo, None, query_rs=True, **kwc))):
                ops.conv_igemm(None, pk2.hi, pk2.lo, None, **kwc)
                self._x16[out.data_ptr()] = (rawn, co)
                return out
        ops.conv_igemm(None, pk2.hi, pk2.lo, out, prec=prec, src16=h16, bias=pk2.bias, res=xres, w_frag=pk2.frag,
                       chan_stats=self._cs_new(out), ws=ws, out16=o16, w_frag16=pk2.frag16, gn_next=gnn, coop=coop2)
        return filed()

    def _in_conv(self, tag: str, rb: ResBlock, pk, a16, c1: int, x2_bmod: int, h, kw) -> None:
        """in_layers' convolution of a ResBlock over the normalised planes a16 of [x1 | x2] (c1 = channels of x1). Under forward_cfg the
        decoder runs at batch 2B = [cond | uncond] while x2, the encoder's skip tensor, is read modulo B: every skip channel whose
        GroupNorm group holds skip channels only carries the same bits in samples b and b + B, and the convolution is linear in its input
        channels. Where _shared_skip admits the site, that K range is summed once, over batch B, into an fp32 partial P, and the 2B launch
        walks the remaining channels and adds P[b % B] as its residual - two launches on the same stream, nothing repacked."""
        plan = self._shared_skip(rb, pk, a16, c1, x2_bmod, h, kw)
        if plan is None:
            ops.conv_igemm(None, pk.hi, pk.lo, h, src16=a16, **kw)
            return
        seam, P, P2 = plan
        if P2 is not None:
            # the shared launch splits K two ways: its two partials stay where the kernel wrote them and the 2B launch adds p0 + p1 as its
            # residual (stedm_conv_args.res2) - the bits of the reduced P without the reduce launch, its store and its re-read
            shared, rest = self._skip_kw(pk, a16, kw, seam, P.shape[0], P2.view(-1), res=P2[0], res2=P2[1])
            n = ops.conv_igemm(None, pk.hi, pk.lo, P, partials=True, **shared)
            assert n == 2, n
        else:
            shared, rest = self._skip_kw(pk, a16, kw, seam, P.shape[0], kw["ws"], res=P)
            ops.conv_igemm(None, pk.hi, pk.lo, P, **shared)
        ops.conv_igemm(None, pk.hi, pk.lo, h, **rest)

    @staticmethod
    def _skip_kw(pk, a16, kw, seam: int, Bs: int, ws, **res):
        """keyword sets of _in_conv's pair, for its launches and for _shared_skip's dry queries: the shared launch over the skip channels
        [seam, C) at batch Bs with workspace ws, and the 2B launch over [0, seam) with the residual(s) `res` read modulo Bs"""
        return (dict(prec=kw["prec"], src16=(a16[0][:Bs, :, :, seam:], None), w_frag=pk.frag, w_frag16=pk.frag16, ws=ws),
                dict(kw, src16=(a16[0][:, :, :, :seam], None), res_bmod=Bs, **res))

    def _shared_skip(self, rb: ResBlock, pk, a16, c1: int, x2_bmod: int, h, kw):
        """(seam, P, P2) when the in_layers convolution of `rb` runs as shared launch + 2B launch (_in_conv), else None. Inference, one CFG pair
        (decoder batch = 2 x2_bmod), single product, both launches admitted by stedm_conv_rs_ok; then cfg_shared_skip or the rule.
        P2 [2, B, H, W, co] (or None): the shared launch splits K two ways and leaves its partials there, no reduce pass (_in_conv)."""
        Bd, H, W, co = h.shape
        if (self.cfg_shared_skip is False or self._tape is not None or self.precision.npass != 1 or x2_bmod <= 0 or Bd != 2 * x2_bmod or
                a16[0].shape[0] != Bd or not a16[0].is_contiguous()):
            return None
        key = ("sskip", id(rb), Bd, H, W, self.cfg_shared_skip, self.cfg_skip_partials)

        def ask():
            C = a16[0].shape[-1]
            cpg = C // rb.in_layers[0].num_groups
            # first 32-channel boundary from which every GroupNorm group holds skip channels only; one chunk further when that makes the
            # shared chunk count even (the K split of a small grid halves it: 15 chunks would not split, 14 do)
            seam = -(-(-(-c1 // cpg) * cpg) // 32) * 32
            if (C - seam) // 32 > 1 and ((C - seam) // 32) % 2:
                seam += 32
            if not (32 <= seam <= C - 32 and (pk.frag is not None or pk.frag16 is not None)):
                return 0
            P = self._buf(f"sskip.P.{x2_bmod}x{H}x{W}x{co}", (x2_bmod, H, W, co))
            shared, rest = self._skip_kw(pk, a16, kw, seam, x2_bmod, kw["ws"], res=P)
            if not (ops.conv_igemm(None, pk.hi, pk.lo, P, query_rs=True, **shared) and ops.conv_igemm(None, pk.hi, pk.lo, h, query_rs=True, **rest) and
                    (self.cfg_shared_skip or self._shared_skip_rule(Bd, H, W, co, C, seam))):
                return 0
            # a two-way K split of the shared launch (asked with the workspace the plain form would use): partials as res / res2
            two = (self.cfg_skip_partials is True and kw["ws"] is not None and
                   ops.conv_igemm(None, pk.hi, pk.lo, P, partials=True, query_rs=True, **shared) == 2)
            if two:
                P2 = self._buf(f"sskip.P2.{x2_bmod}x{H}x{W}x{co}", (2, x2_bmod, H, W, co))
                shared, rest = self._skip_kw(pk, a16, kw, seam, x2_bmod, P2.view(-1), res=P2[0], res2=P2[1])
                two = (ops.conv_igemm(None, pk.hi, pk.lo, P, partials=True, query_rs=True, **shared) == 2 and
                       bool(ops.conv_igemm(None, pk.hi, pk.lo, h, query_rs=True, **rest)))
            self._consts[("sskip2",) + key[1:]] = bool(two)
            return seam
        seam = self._asked(key, ask)
        if not seam:
            return None
        P2 = self._buf(f"sskip.P2.{x2_bmod}x{H}x{W}x{co}", (2, x2_bmod, H, W, co)) if self._consts[("sskip2",) + key[1:]] else None
        return seam, self._buf(f"sskip.P.{x2_bmod}x{H}x{W}x{co}", (x2_bmod, H, W, co)), P2

    @staticmethod
    def _shared_skip_rule(Bd: int, H: int, W: int, co: int, C: int, seam: int) -> bool:
        """Does the pair beat the single launch at this site? From the per-site measurement (tools/shared_skip_sites.py):
        the saving is the shared channels' MFMA work at half the batch, the cost a second launch's per-tile fixed cost (tables, first patch,
        epilogue), the partial's store and its read. Measured at decoder batch 128: 14 shared chunks of 32 channels win where the shared
        launch fills the chip without a K split (16^2: +27 us of 337) and break even where it needs one (8^2: -2 us of 181: the reduce pass
        eats the gain); 32 chunks win either way (+28 .. +34 us of 235); 2 .. 4 chunks lose 10 .. 15 us everywhere. A decoder batch whose
        own launch does not fill the chip (K-split grids, priced by their fixed cost) was not measured and stays on the single launch."""
        cus = ops.device_cus()

        def fills(b):      # conv_rs_pick's own test: 256-row x 128-channel tiles against 3/4 of the chip
            tiles_m = -(-b * H * W // 256) if H * W >= 256 else -(-b // (256 // (H * W)))
            return tiles_m * -(-co // 128) * 4 >= cus * 3
        if not fills(Bd):
            return False
        return (C - seam) // 32 >= (14 if fills(Bd // 2) else 32)

    def _replicate(self, h, nrep: int):
        """the shared tensor h [B,...] and its channel statistics at batch nrep x B = [cond | uncond] (the style-conditioned remainder's input)"""
        h2 = self._buf("mid.rep", (nrep * h.shape[0],) + tuple(h.shape[1:]))
        cs1 = self._cs.get(h.data_ptr())
        cs2 = self._cs_new(h2, nslab=cs1.shape[1]) if cs1 is not None else None
        # (one broadcast copy per tensor instead of nrep device-to-device memcpys: four launches of ~5 us were 0.4 % of the bench step)
        h2.view((nrep,) + tuple(h.shape)).copy_(h.unsqueeze(0).expand((nrep,) + tuple(h.shape)))
        if cs2 is not None:      # the replicas share the statistics of the shared-encoder tensor
            cs2.view((nrep,) + tuple(cs1.shape)).copy_(cs1.unsqueeze(0).expand((nrep,) + tuple(cs1.shape)))
        return h2

    # ---- the CFG seam: the style block's shared front --------------------------------------------------------------
    def _front_ws(self, nel: int) -> torch.Tensor:
        """workspace of the style block's partials (its own buffer: conv_ws is rewritten by the launches between the two halves)"""
        return self._buf("sfront.ws", ((16 if nel <= (1 << 20) else (4 if nel <= (1 << 22) else (2 if nel <= (1 << 23) else 1))) * nel,))

    def _front_kw(self, tag: str, rb: ResBlock, x1, next_norm):
        """operands of _res_front's launches for the shared input x1 [B,H,W,C] (buffers are the model's own, made on first use)"""
        prec = self.precision
        B, H, W, _ = x1.shape
        Bd, co = 2 * B, rb.out_channels
        pk, pk2 = self._packed[id(rb.in_layers[2])], self._packed[id(rb.out_layers[3])]
        h = self._buf(f"h.{Bd}x{H}x{W}x{co}", (Bd, H, W, co))
        out = self._buf(tag + ".out", (Bd, H, W, co))
        h16 = self._planes(Bd, H, W, co, "g16")
        gnn = npl = coop2 = None
        if next_norm is not None and not os.environ.get("STEDM_NO_NEXT_GN"):
            npl = self._planes(Bd, H, W, co)
            gnn = self._gn_next(*next_norm, npl, None, False)
            coop2 = self._coop_for(tag + ".c2", Bd, H, W, co, prec)
        part = dict(prec=prec, w_frag=pk.frag, w_frag16=pk.frag16, ws=self._front_ws(B * H * W * co), partials=True)
        fin = dict(prec=prec, ws_bmod=B, bias=pk.bias, gn_next=self._gn_next(rb.out_layers[0], 1, h16, None, True))
        tail = dict(prec=prec, src16=h16, bias=pk2.bias, res=x1, res_bmod=B, w_frag=pk2.frag, ws=self._splitk_ws_res(Bd * H * W * co), w_frag16=pk2.frag16,
                    gn_next=gnn, coop=coop2)
        return pk, pk2, h, out, npl, part, fin, tail

    def _shared_front(self, tag: str, rb: ResBlock, x1shape, next_norm) -> bool:
        """Does the style block `rb` run as _res_front over the shared tensor of shape x1shape [B,H,W,C]? Inference, single product, identity
        residual, both convolution launches admitted by a dry query; then cfg_shared_front or the rule. The answer is filed in _consts
        under ("sfront", ...): the share count of the partials-only launch, 0 when the block is not routed."""
        B, H, W, C = x1shape
        if (self.cfg_shared_front is False or self._tape is not None or self.precision.npass != 1 or not isinstance(rb.skip_connection, nn.Identity) or
                rb.out_channels != C or rb.use_scale_shift_norm or self._drop_live(rb)):
            # (a scale-shift-norm style block: the finish pass adds the style row onto h, which that block does not do; a block with live
            #  dropout: the finish pass writes out_layers' planes without the mask)
            return False
        key = ("sfront", id(rb), 2 * B, H, W, self.cfg_shared_front)

        def ask():
            pk, pk2, h, out, npl, part, fin, tail = self._front_kw(tag, rb, self._buf("mid.a.0.out", x1shape), next_norm)      # (the shared tensor's own buffer)
            if (pk.frag is not None or pk.frag16 is not None) and C % 4 == 0 and (self.cfg_shared_front or self._shared_front_rule(2 * B, H, W, C)):
                a16 = self._planes(B, H, W, C)
                n = ops.conv_igemm(None, pk.hi, pk.lo, self._buf(f"h.{B}x{H}x{W}x{C}", (B, H, W, C)), src16=a16, query_rs=True, **part)
                if n and ops.conv_igemm(None, pk2.hi, pk2.lo, out, chan_stats=self._cs_new(out), query_rs=True, **tail):
                    return int(n)
            return 0
        return bool(self._asked(key, ask))

    @staticmethod
    def _shared_front_rule(Bd: int, H: int, W: int, co: int) -> bool:
        """Does the shared front beat the 2B block? The saving is half of the in_layers convolution's MFMA work, its GroupNorm pass and the two
        broadcast copies; the cost is the finish pass at 2B. From the per-site measurement (tools/shared_front_site.py; DESIGN.md section
        10.14), 1024 channels: decoder batch 128 / 96 / 64 at 8 x 8 win 70 / 51 / 35 us of 480 / 386 / 299, batch 128 at 16 x 16 wins 214 of
        1571. The smallest grid measured is the decoder batch's own launch on half the chip (128 tiles of 256 rows x 128 channels on 256
        CUs); smaller ones were not measured and stay on the launches they have."""
        cus = ops.device_cus()
        tiles_m = -(-Bd * H * W // 256) if H * W >= 256 else -(-Bd // (256 // (H * W)))
        return tiles_m * -(-co // 128) * 2 >= cus

    def _res_front(self, tag: str, rb: ResBlock, x1, style_all, next_norm):
        """The ResBlockStyle at the CFG seam over the SHARED tensor x1 [B,H,W,C] (output of middle_block[0]) -> [2B,H,W,C] = [cond | uncond].
        The two style vectors first enter as the embedding row added to in_layers' convolution, so that block's GroupNorm, its 3x3
        convolution and the identity residual carry the same bits in samples b and b + B: the GroupNorm planes come from
        middle_block[0]'s tail convolution at batch B, the convolution runs once at batch B and leaves its K-share partials
        (stedm_conv_partials), the finish pass at 2B adds bias and the style row of each sample and writes h's statistics and out_layers'
        GroupNorm + SiLU planes (stedm_conv_finish, ws_bmod = B), and the tail convolution at 2B reads x1 as its residual modulo B."""
        B, H, W, C = x1.shape
        pk, pk2, h, out, npl, part, fin, tail = self._front_kw(tag, rb, x1, next_norm)
        a16 = self._norm16(rb.in_layers[0], 1, x1)
        n = ops.conv_igemm(None, pk.hi, pk.lo, self._buf(f"h.{B}x{H}x{W}x{C}", (B, H, W, C)), src16=a16, **part)
        self._last_h = h
        ops.conv_finish(part["ws"], n, h, emb=style_all, emb_bstride=style_all.shape[1], chan_stats=self._cs_new(h), **fin)
        ops.conv_igemm(None, pk2.hi, pk2.lo, out, chan_stats=self._cs_new(out), **tail)
        if npl is not None:
            self._pre16[out.data_ptr()] = (id(next_norm[0]), next_norm[1], npl)
        return out

    def _attn(self, tag: str, ab: AttentionBlock, x):
        """AttentionBlock._forward openaimodel.py:340-346 on NHWC (tokens = H*W)."""
        prec = self.precision
        B, H, W, Cc = x.shape
        pq = self._packed[id(ab.qkv)]
        pp = self._packed[id(ab.proj_out)]
        out = self._buf(tag + ".out", (B, H, W, Cc))
        ch = Cc // ab.num_heads
        if prec.npass == 1 and self._tape is None and ch in (16, 32, 64, 128):
            # 64 tokens (64 n tokens: key tiles with an online softmax around the same products): the qkv conv writes its result as a 16-bit plane, the whole attention of a (sample, head) runs on one wave's
            # MFMAs and is written as proj_out's 16-bit operand plane (same operand rounding as everywhere in these modes)
            qkv16 = self._planes(B, H, W, 3 * Cc, "qkv16")
            ops.conv_igemm(None, pq.hi, pq.lo, None, prec=prec, ks=1, src16=self._norm16(ab.norm, 0, x), bias=pq.bias, w_frag=pq.frag,
                           out16=qkv16)
            a16 = self._planes(B, H, W, Cc, "attn16")
            ops.attn_legacy16(qkv16[0].view(B, H * W, 3 * Cc), a16[0], ab.num_heads, prec, **ab.order_kw())
            ops.conv_igemm(None, pp.hi, pp.lo, out, prec=prec, ks=1, src16=a16, bias=pp.bias, res=x, w_frag=pp.frag,
                           chan_stats=self._cs_new(out), ws=self._splitk_ws(out.numel()))
            return out
        qkv = self._buf(tag + ".qkv", (B, H, W, 3 * Cc))
        ops.conv_igemm(None, pq.hi, pq.lo, qkv, prec=prec, ks=1, src16=self._norm16(ab.norm, 0, x), bias=pq.bias, w_frag=pq.frag,
                       w_frag16=pq.frag16 if prec.npass == 3 else None)
        a = self._buf(tag + ".a", (B, H, W, Cc))
        ops.attn_legacy(qkv.view(B, H * W, 3 * Cc), a.view(B, H * W, Cc), ab.num_heads, **ab.order_kw())
        if self._tape is not None:
            self._tape.append(("attn", ab, x, qkv, a, out))
        ops.conv_igemm(None, pp.hi, pp.lo, out, prec=prec, ks=1, src16=self._norm16(None, 0, a), bias=pp.bias, res=x, w_frag=pp.frag,
                       chan_stats=self._cs_new(out), w_frag16=pp.frag16 if prec.npass == 3 else None)
        return out

    def _down(self, ltag: str, layer: Downsample, h):
        """Downsample.forward openaimodel.py:165-167: the stride-2 3x3 convolution, or (conv_resample=False) the 2 x 2 average pool."""
        B, H, W, _ = h.shape
        out = self._buf(ltag + ".out", (B, H // 2, W // 2, layer.out_channels))
        if self._tape is not None:
            self._tape.append(("down", layer, h, out))
        if not layer.use_conv:
            # one pass: the pooled tensor and its channel statistics (the next ResBlock's GroupNorm and a decoder concat GroupNorm read them)
            ops.avgpool2x2(h, out, self._cs_new(out))
            return out
        pk = self._packed[id(layer.op)]
        ps2 = self._packed.get((id(layer.op), "s2d"))
        if H % 2 == 0 and W % 2 == 0 and not ops.conv3x3_tiles_ok(H // 2, W // 2):
            # an output grid the tiled kernels cannot tile (latent widths that are not powers of two): im2col + flat GEMM (ops.conv_igemm)
            return ops.conv_igemm(None, pk.hi, pk.lo, out, prec=self.precision, mode=CONV_DOWN, src16=self._norm16(None, 0, h), bias=pk.bias,
                                  chan_stats=self._cs_new(out))
        elif ps2 is not None and H % 2 == 0 and W % 2 == 0 and (H // 2) * (W // 2) >= 16:
            C = h.shape[-1]
            planes = self._buf(f"s2d16.{B}x{H}x{W}x{C}", (B, H // 2, W // 2, 4 * C), torch.int16)
            planes_lo = self._buf(f"s2d16lo.{B}x{H}x{W}x{C}", (B, H // 2, W // 2, 4 * C), torch.int16) if self.precision.npass == 3 else None
            ws = self._splitk_ws(out.numel())
            kw2 = dict(prec=self.precision, mode=CONV_S2D, src16=(planes, planes_lo), bias=ps2.bias, w_frag=ps2.frag, w_frag16=ps2.frag16, ws=ws)
            if self.precision.npass == 3 and not ops.conv_igemm(None, None, None, out, query_rs=True, **kw2):
                # (a problem the register-streamed 3-product kernel does not take: the fused fp32-source kernel, as before)
                return ops.conv_igemm(h, pk.hi, pk.lo, out, prec=self.precision, mode=CONV_DOWN, bias=pk.bias)
            else:
                ops.space_to_depth16(h, planes, planes_lo, self.precision)
                return ops.conv_igemm(None, None, None, out, chan_stats=self._cs_new(out), **kw2)
        else:
            # fused fp32-source kernel (parity mode / odd sizes)
            return ops.conv_igemm(h, pk.hi, pk.lo, out, prec=self.precision, mode=CONV_DOWN, bias=pk.bias)

    def _up(self, ltag: str, layer: Upsample, h, nxt, cat_ok, next_skip_c):
        """Upsample.forward openaimodel.py:124-132: nearest x2 + 3x3 convolution. cat_ok / next_skip_c as in _run_block: as the block's last layer
        (nxt is None) it may write its output as 16-bit values into the next block's concat plane. conv_resample=False: the bare nearest x2 -
        an fp32 tensor and its statistics in every mode (the next block's concat GroupNorm reads both)."""
        B, H, W, _ = h.shape
        out = self._buf(ltag + ".out", (B, H * 2, W * 2, layer.out_channels))
        if self._tape is not None:
            self._tape.append(("up", layer, h, out))
        if not layer.use_conv:
            ops.replicate2x2(h, out, 1.0, False, self._cs_new(out))
            return out
        pk = self._packed[id(layer.conv)]
        pu = self._packed[(id(layer.conv), "up")]
        src16 = self._raw16.get(h.data_ptr()) or self._norm16(None, 0, h)
        if not ops.conv3x3_tiles_ok(H, W):
            # (the sub-pixel form tiles the low-resolution grid) generic shapes: nearest x2 + 3x3 as im2col + flat GEMM from the plain filter
            return ops.conv_igemm(None, pk.hi, pk.lo, out, prec=self.precision, mode=CONV_UP, src16=src16, bias=pk.bias,
                                  chan_stats=self._cs_new(out))
        # statistics slots of the sub-pixel form: (256-pixel run of the low-res grid) x (output parity)
        # (small grids — a sampling batch of up to 8 — split K over the workspace like the other kinds)
        ws = self._splitk_ws(out.numel()) if self.precision.npass == 1 else None
        kwu = dict(prec=self.precision, mode=CONV_UP_SUBPIXEL, src16=src16, bias=pu.bias, w_frag=pu.frag,
                   chan_stats=self._cs_new(out, 4 * ops.gn_chan_nslab(H * W)), w_frag16=pu.frag16, ws=ws)
        if cat_ok and nxt is None and ops.gn_apply16c_x16_ok(layer.out_channels, next_skip_c):
            # the next block's GroupNorm and skip_connection are this tensor's only readers: 16-bit values into its concat's raw plane
            ncat = layer.out_channels + next_skip_c
            rawn = self._cat_plane(B, 2 * H, 2 * W, layer.out_channels, ncat)
            kwc = dict(kwu, out16=(rawn, None), out16_stride=ncat, cout=layer.out_channels)
            if self._asked(("upcat", id(layer), B, H, W, ncat), lambda: bool(ops.conv_igemm(None, pu.hi, pu.lo, None, query_rs=True, **kwc))):
                ops.conv_igemm(None, pu.hi, pu.lo, None, **kwc)
                self._x16[out.data_ptr()] = (rawn, layer.out_channels)
                return out
        return ops.conv_igemm(None, pu.hi, pu.lo, out, **kwu)

    @staticmethod
    def _first_norm(layer):
        """(GroupNorm32, act) of the first thing `layer` does with its input when it reads that tensor alone and needs no raw copy of it, else None"""
        if isinstance(layer, ResBlockStyle):
            layer = layer.block
        if isinstance(layer, ResBlock):
            # (an up / down block resamples between its GroupNorm and its convolution: no producer can write same-resolution planes for it)
            return (layer.in_layers[0], 1) if isinstance(layer.skip_connection, nn.Identity) and not layer.updown else None
        if isinstance(layer, AttentionBlock):
            return (layer.norm, 0)
        return None

    def _run_block(self, tag: str, blk, h, skip, emb_all, emb_bstride, style_all, skip_bmod=0, li0=0, next_skip_c=None, next_layer=None):
        """TimestepEmbedSequential.forward openaimodel.py:93-101 (+ the th.cat of :800 folded into the first layer).
        next_skip_c: channels of the skip tensor the NEXT block concatenates to this block's output (decoder), when that block starts with a
        ResBlock that has a skip_connection convolution: the last layer here may then write its output as 16-bit values into that concat's
        raw plane instead of an fp32 tensor (_res / Upsample below)."""
        layers = list(blk)
        # (from 8 decoder rows on: at a sampling batch of 1 the 16-bit-only form measured 40.2 against 38.6 ms per DDIM-20 loop - launches
        #  of that size are latency, not bytes)
        cat_ok = (next_skip_c is not None and self._tape is None and self.precision.npass == 1 and
                  h.shape[0] >= 8 and not os.environ.get("STEDM_NO_CAT16"))
        for li, layer in enumerate(layers, start=li0):
            ltag = f"{tag}.{li}"
            nxt = layers[li - li0 + 1] if li - li0 + 1 < len(layers) else None
            if isinstance(layer, ResBlock):
                x1 = h
                ncat = None
                if cat_ok and nxt is None and ops.gn_apply16c_x16_ok(layer.out_channels, next_skip_c):
                    ncat = layer.out_channels + next_skip_c
                h = self._res(ltag, layer, h, skip, emb_all, self._emb_off[id(layer)], emb_bstride, x2_bmod=skip_bmod,
                              want16=isinstance(nxt, Upsample) and nxt.use_conv, next_cat=ncat, next_norm=self._first_norm(nxt if nxt is not None else next_layer))
                if self._tape is not None:
                    self._tape.append(("res", layer, x1, skip, self._last_h, h, self._emb_off[id(layer)]))
                skip = None
            elif isinstance(layer, ResBlockStyle):
                x1 = h
                h = self._res(ltag, layer.block, h, None, style_all, 0, style_all.shape[1],       # (never the last layer of its block: no next_cat)
                              next_norm=self._first_norm(nxt if nxt is not None else next_layer))
                if self._tape is not None:
                    self._tape.append(("res", layer.block, x1, None, self._last_h, h, None))
            elif isinstance(layer, AttentionBlock):
                h = self._attn(ltag, layer, h)
            elif type(layer).__name__ == "SpatialTransformer":
                # routed without context, exactly like the reference (openaimodel.py:99-100)
                if self._tape is not None:
                    saved = {}
                    x_in = h
                    h = layer.run(h, self._packed[id(layer)], self.precision, self._buf, save=saved)
                    self._tape.append(("st", layer, x_in, saved, h))
                else:
                    h = layer.run(h, self._packed[id(layer)], self.precision, self._buf)
            elif isinstance(layer, Downsample):
                h = self._down(ltag, layer, h)
            elif isinstance(layer, Upsample):
                h = self._up(ltag, layer, h, nxt, cat_ok, next_skip_c)
            else:
                raise TypeError(f"unexpected layer {type(layer).__name__} in {tag}")
        return h

    # ------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        """openaimodel.py:761-806. x [B,C,H,W] fp32 NCHW (already concatenated with c_concat by the
        DiffusionWrapper), timesteps [B] (integer: int64; floating: float32, fractional model times allowed), context [B, 4*model_channels]
        style vector -> eps [B,out,H,W]."""
        assert (y is not None) == (self.num_classes is not None), \
            "must specify y if and only if the model is class-conditional"
        return self.forward_parts(x, None, timesteps, context)

    @torch.no_grad()
    def forward_parts(self, x, c_concat, timesteps, context, out: Optional[torch.Tensor] = None, uniform_t: bool = False) -> torch.Tensor:
        """Same as forward, but takes the latent and the concat-conditioning separately (the cat of
        ddpm.py:1415 is folded into the first conv's loader). uniform_t=True promises that all timesteps are equal
        (DDIM sampling, ddim.py:141): the timestep-embedding path is then evaluated for one row and broadcast."""
        return self._forward_impl(x, c_concat, timesteps, [context], out, uniform_t)

    @torch.no_grad()
    def forward_cfg(self, x, c_concat, timesteps, context_cond, context_uncond, out: Optional[torch.Tensor] = None,
                    uniform_t: bool = False):
        """Both classifier-free-guidance evaluations of ddim.py:177-178 in one pass: returns (e_t, e_t_uncond).

        The reference runs the U-Net twice on the same (x, t, c_concat) with two style vectors. The style vector only
        enters at middle_block[1] (ResBlockStyle, openaimodel.py:636-643), so everything before it — the 9 input blocks
        and middle_block[0] — is bit-identical in the two runs and is evaluated once (batch B); from the style block on
        the batch is 2B = [cond | uncond], with the skip tensors of the shared encoder read modulo B. Per-sample
        arithmetic (GroupNorm is per sample) is exactly that of two sequential forwards."""
        o = self._forward_impl(x, c_concat, timesteps, [context_cond, context_uncond], out, uniform_t)
        B = x.shape[0]
        return o[:B], o[B:]

    def _style_proj(self, contexts, B, ted):
        """emb_layers of the ResBlockStyle applied to the style vector(s) (openaimodel.py:277 with emb = context). The
        style vectors do not change during a sampling run: cached per (storage, version) of the context tensors. An entry keeps
        its context tensors alive, so a freed tensor's address cannot come back under a stale entry."""
        c = self._consts
        key = tuple((cx.data_ptr(), cx._version, tuple(cx.shape)) for cx in contexts) + (self._pack_key is not None and id(c["style_wt"]),)
        hit = self._style_cache.get(key)
        if hit is not None:
            return hit[0]
        nrep = len(contexts)
        if nrep == 1:
            ctx_all = contexts[0].float().contiguous()
        else:
            ctx_all = torch.cat([cx.float() for cx in contexts], dim=0).contiguous()
        style_all = ops.emb_proj(ctx_all, c["style_wt"], c["style_b"],
                                 torch.empty((B * nrep, c["style_wt"].shape[1]), dtype=torch.float32, device=ctx_all.device))
        if len(self._style_cache) > 8:
            self._style_cache.clear()
        self._style_cache[key] = (style_all, tuple(contexts))
        return style_all

    def _forward_impl(self, x, c_concat, timesteps, contexts, out, uniform_t=False):
        if self._tape is None and self.dropout_live():
            raise RuntimeError("UNetModel: dropout is live (train() with dropout > 0) and this is an inference entry point - call .eval() first; "
                               "train-mode dropout runs through UNetTrainer only")
        self._drop_used = {}
        self._prepare()
        self._cs = {}
        self._raw16 = {}
        self._x16 = {}          # fp32 handle -> (raw plane of the next block's concat, channels): tensors that exist in 16 bits only
        self._catpp = 0
        self._pre16 = {}        # fp32 handle -> (id(norm), act, planes): GroupNorm planes written ahead by the producing convolution's call
        if getattr(self, "_coop_state", None) is None or self._coop_state.device != x.device:
            self._coop_bufs, self._coop_state = {}, ops.coop_words_new()
        self._coop_advanced = False
        self._saved16 = {}
        self._saved_mr = {}
        self._plane_ctr = 0
        self._mr_ctr = 0
        x = x.float().contiguous()
        B, c1, H, W = x.shape
        nrep = len(contexts)
        Bd = B * nrep                      # decoder batch

        c2 = 0
        if c_concat is not None:
            c_concat = c_concat.float().contiguous()
            c2 = c_concat.shape[1]
        assert c1 + c2 == self.in_channels, f"expected {self.in_channels} input channels, got {c1}+{c2}"
        if any(cx is None for cx in contexts):
            raise ValueError("context (style vector) is required: middle_block[1] is a ResBlockStyle (openaimodel.py:636-643)")
        # integer timesteps run as int64 (training, DDIM); floating ones stay float32: DPM-Solver's fractional model times
        # (dpm_solver.py:246-253), which timestep_embedding allows (util.py:151-171). No truncation either way.
        if not isinstance(timesteps, torch.Tensor):
            timesteps = torch.as_tensor(timesteps)
        t_float = timesteps.is_floating_point()
        if t_float and self._tape is not None:
            raise TypeError("fractional (floating) timesteps are an inference path: the training forward takes integer timesteps")
        timesteps = timesteps.to(device=x.device, dtype=torch.float32 if t_float else torch.int64).contiguous()
        c = self._consts
        ted = self.model_channels * 4
        for cx in contexts:
            assert tuple(cx.shape) == (B, ted), f"context must be [B,{ted}] (ResBlockStyle uses it as the embedding)"
        Bt = 1 if uniform_t else B          # rows of the timestep-embedding path
        emb = ops.time_embed(timesteps[:Bt], c["freqs"], c["te_w0t"], c["te_b0"], c["te_w2t"], c["te_b2"], self._buf("emb", (Bt, ted)),
                             self._buf("emb_ws", (Bt * (self.model_channels + ted),)))
        emb_e = ops.emb_proj(emb, c["emb_wt"], c["emb_b"], self._buf("emb_all", (Bt, self._emb_ntot)))
        emb_stride = 0 if uniform_t else self._emb_ntot
        if nrep == 1 or uniform_t:
            emb_d = emb_e
        else:  # decoder rows b and b+B share timestep row b
            emb_d = self._buf("emb_all_d", (Bd, self._emb_ntot))
            emb_d.view(nrep, B, self._emb_ntot).copy_(emb_e.unsqueeze(0).expand(nrep, B, self._emb_ntot))
        style_all = self._style_proj(contexts, B, ted)

        conv0 = self.input_blocks[0][0]
        h = self._buf("in0.out", (B, H, W, self.model_channels))
        if H % 2 == 0:
            cs0 = self._cs_new(h, H // 2)                     # one slot per pair of image rows, from the kernel's epilogue
            if not ops.conv_in(x, c_concat, conv0.weight, conv0.bias, h, chan_stats=cs0):
                del self._cs[h.data_ptr()]                    # generic path: statistics on first use
        else:
            ops.conv_in(x, c_concat, conv0.weight, conv0.bias, h)
        if self._tape is not None:
            self._tape.append(("conv_in", x, c_concat, h))
            self._tape_emb = (timesteps, emb, contexts[0])
            self._tape_film = (emb_e, style_all)          # scale | shift rows of the scale-shift-norm blocks (the backward reads them again)
        hs = [h]
        mid = list(self.middle_block)
        nblk = len(self.input_blocks)
        for i, blk in enumerate(self.input_blocks[1:], start=1):
            # (the layer that reads this block's output alone, if any: its GroupNorm may ride on this block's tail convolution)
            nl = list(self.input_blocks[i + 1])[0] if i + 1 < nblk else mid[0]
            h = self._run_block(f"in{i}", blk, h, None, emb_e, emb_stride, None, next_layer=nl)
            hs.append(h)
        # middle block: [0] shared, then replicate the batch for the style-conditioned remainder
        # (under one CFG pair the style block's front may stay at batch B: _shared_front / _res_front)
        front = (nrep == 2 and len(mid) > 2 and isinstance(mid[1], ResBlockStyle) and
                 self._shared_front("mid.b.1", mid[1].block, tuple(h.shape), self._first_norm(mid[2])))
        h = self._run_block("mid.a", mid[:1], h, None, emb_e, emb_stride, None, next_layer=mid[1] if (nrep == 1 or front) and len(mid) > 1 else None)
        if front:
            h = self._res_front("mid.b.1", mid[1].block, h, style_all, self._first_norm(mid[2]))
        elif nrep > 1:
            h = self._replicate(h, nrep)

        def first_takes_cat(blk):      # a decoder block whose first layer is a ResBlock with a skip_connection convolution (always, in this net)
            l0 = list(blk)[0]
            return isinstance(l0, ResBlock) and not isinstance(l0.skip_connection, nn.Identity)

        ob = list(self.output_blocks)
        h = self._run_block("mid.b", mid[2:] if front else mid[1:], h, None, emb_d, emb_stride, style_all, li0=2 if front else 1,
                            next_skip_c=hs[-1].shape[-1] if ob and first_takes_cat(ob[0]) else None)
        bmod = B if nrep > 1 else 0
        for i, blk in enumerate(ob):
            skip = hs.pop()
            nsc = hs[-1].shape[-1] if (i + 1 < len(ob) and first_takes_cat(ob[i + 1])) else None
            h = self._run_block(f"out{i}", blk, h, skip, emb_d, emb_stride, style_all, skip_bmod=bmod, next_skip_c=nsc)
        if out is None:
            out = torch.empty((Bd, self.out_channels, H, W), dtype=torch.float32, device=x.device)
        gn = self.out[0]
        cs = self._chan_stats(h)     # left by the last ResBlock's conv epilogue
        ops.conv_out(h, gn.weight, gn.bias, gn.eps, gn.num_groups, c["out_w_hwio"], self.out[2].bias, out, cs)
        if self._tape is not None:
            self._tape.append(("conv_out", h, out))
        return out
