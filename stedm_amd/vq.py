"""First stage of the latent diffusion model: the frozen VQ-f4 autoencoder, HIP-backed.

Drop-in for `ldm.models.autoencoder.VQModelInterface` (reference autoencoder.py:264-282 over VQModel :14-110) with
`ldm.modules.diffusionmodules.model.Encoder / Decoder` (model.py:368-459, 462-568: ResnetBlock :82-140, AttnBlock :143-199,
Upsample :43-57, Downsample :59-79, GroupNorm eps 1e-6 :38-39) and taming-transformers' `VectorQuantizer2` (un-vendored third-party
dependency, autoencoder.py:6; its published forward is restated: nearest codebook entry + straight-through value). Same constructor
arguments (`embed_dim, n_embed, ddconfig, lossconfig, ckpt_path, ...`), same `encode(x)` / `decode(h, force_not_quantize=False)`,
same state-dict names (`encoder.down.0.block.0.norm1.weight`, `decoder.up.2.upsample.conv.weight`, `quantize.embedding.weight`,
`quant_conv.*`, `post_quant_conv.*`), so the reference's `vq-f4.ckpt` loads with `load_state_dict`.

The architecture is written down once: `first_stage_layout(**ddconfig)` lists, for the encoder and for the decoder, the rows that run
(ResNet block, attention block, downsample, upsample) in execution order with their state-dict prefixes and channel counts.
`_containers` builds the parameter containers from it, `_prepare` packs the weights row by row and `_walk` runs the rows. That engine
(`FirstStageEngine`) is shared by the two frozen stages built on it: `VQModelInterface` and `AutoencoderKL` (autoencoder.py:285-342, the
KL stage: the encoder emits 2 * z_channels moments and `encode` returns their `DiagonalGaussianDistribution`). `IdentityFirstStage`
(autoencoder.py:426-443) passes its input through.

torch.nn modules are parameter containers; the arithmetic runs in the kernels the U-Net uses: GroupNorm(+SiLU) from producer-side
channel statistics into 16-bit operand planes (stedm_gn_apply16c), 3x3 / 1x1 / fused-shortcut / sub-pixel-upsample /
space-to-depth-downsample convolutions on MFMA (stedm_conv_igemm), the boundary convs (stedm_conv_in / stedm_conv_out), and for the
single-head attention of width C two GEMMs around a row softmax (stedm_softmax_rows16). Activations are NHWC fp32 inside, NCHW at the
surface like the reference."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import CONV_S2D, CONV_UP_SUBPIXEL, StedmHipError
from .ops import Precision


class Row(NamedTuple):
    """One step of the encoder or of the decoder."""
    kind: str        # "res" | "attn" | "down" | "up": FirstStageEngine._res / _attn / _down / _up runs it
    prefix: str      # where its parameters live in the state dict, under `encoder.` / `decoder.` (`down.1.block.0`, `mid.attn_1`, ...)
    cin: int
    cout: int


class Half(NamedTuple):
    """The encoder or the decoder: conv_in, the rows in execution order, GroupNorm + SiLU + conv_out."""
    stack: str                   # name of its list of levels: "down" (registered before `mid`) or "up" (after it)
    conv_in: Tuple[int, int]     # channels in, out
    rows: Tuple[Row, ...]
    norm_out: int
    conv_out: Tuple[int, int]


class Layout(NamedTuple):
    levels: int                  # resolutions; the stage's downsampling factor is 2 ** (levels - 1)
    encoder: Half
    decoder: Half


def first_stage_layout(*, ch, out_ch, num_res_blocks, attn_resolutions, in_channels, resolution, z_channels, ch_mult=(1, 2, 4, 8), dropout=0.0,
                       resamp_with_conv=True, double_z=True, give_pre_end=False, tanh_out=False, use_linear_attn=False, attn_type="vanilla",
                       **unused) -> Layout:
    """The first stage's architecture from its `ddconfig` (the keyword arguments of the reference's Encoder / Decoder), written down once:
    the containers, the weight packing and the forward walk all read it. Pure Python, no tensors. Options the kernels do not cover are
    refused here, before any module or device work."""
    widths = [ch * m for m in ch_mult]
    n = len(widths)
    for option, refused in (("resamp_with_conv=False", n > 1 and not resamp_with_conv), ("use_linear_attn=True", use_linear_attn),
                            ('attn_type="linear"', attn_type == "linear"),
                            (f"attn_type={attn_type!r} (unknown)", attn_type not in ("vanilla", "linear", "none")),
                            ("give_pre_end", give_pre_end), ("tanh_out", tanh_out), (f"dropout={dropout}", dropout != 0)):
        if refused:
            raise NotImplementedError(f"first stage ddconfig: {option} is not supported (vq-f4.yaml does not use it)")
    attends = attn_type == "vanilla"

    def level(name, k, c, blocks, side):
        """level k of `down` / `up` at image side `side`: (its rows, its output width)"""
        rows = []
        for b in range(blocks):
            rows.append(Row("res", f"{name}.{k}.block.{b}", c, widths[k]))
            c = widths[k]
            if attends and side in attn_resolutions:
                rows.append(Row("attn", f"{name}.{k}.attn.{b}", c, c))
        return rows, c

    def mid(c):
        attn = [Row("attn", "mid.attn_1", c, c)] if attends else []
        return [Row("res", "mid.block_1", c, c)] + attn + [Row("res", "mid.block_2", c, c)]

    enc = []
    for k in range(n):                             # finest level first; every level but the coarsest ends in a stride-2 conv
        rows, c = level("down", k, widths[k - 1] if k else ch, num_res_blocks, resolution >> k)
        enc += rows + ([Row("down", f"down.{k}.downsample", c, c)] if k < n - 1 else [])
    encoder = Half("down", (in_channels, ch), tuple(enc + mid(c)), c, (c, 2 * z_channels if double_z else z_channels))
    c = widths[-1]
    dec = mid(c)
    for k in reversed(range(n)):                   # coarsest level first: `up.{n-1}` runs first though the state dict lists `up.0` first
        rows, c = level("up", k, c, num_res_blocks + 1, (resolution // 2 ** (n - 1)) << (n - 1 - k))
        dec += rows + ([Row("up", f"up.{k}.upsample", c, c)] if k else [])
    return Layout(n, encoder, Half("up", (z_channels, widths[-1]), tuple(dec), c, (c, out_ch)))


def _containers(name: str, half: Half, levels: int):
    """The parameter containers of one half (`name`: encoder / decoder) under the reference's state-dict names, and
    [(buffer tag, row, the row's leaves)] in execution order. Levels are registered by index, not in row order, so `state_dict()`
    lists `up.0` first."""
    gn = lambda c: nn.GroupNorm(32, c, eps=1e-6)
    net, stack = nn.Module(), nn.ModuleList()
    for _ in range(levels):
        lv = nn.Module()
        lv.block, lv.attn = nn.ModuleList(), nn.ModuleList()
        stack.append(lv)
    net.conv_in = nn.Conv2d(*half.conv_in, 3, padding=1)
    for child in ("down", "mid") if half.stack == "down" else ("mid", "up"):
        setattr(net, child, stack if child == half.stack else nn.Module())
    steps = []
    for row in half.rows:
        m, ci, co = nn.Module(), row.cin, row.cout
        if row.kind == "res":
            m.norm1, m.conv1, m.norm2, m.conv2 = gn(ci), nn.Conv2d(ci, co, 3, padding=1), gn(co), nn.Conv2d(co, co, 3, padding=1)
            if ci != co:
                m.nin_shortcut = nn.Conv2d(ci, co, 1)
        elif row.kind == "attn":
            m.norm = gn(ci)
            m.q, m.k, m.v, m.proj_out = (nn.Conv2d(ci, ci, 1) for _ in range(4))
        else:                                      # "down": zero pad bottom / right by one, then 3x3 stride 2; "up": nearest x2, then 3x3
            m.conv = nn.Conv2d(ci, ci, 3, stride=2, padding=0) if row.kind == "down" else nn.Conv2d(ci, ci, 3, padding=1)
        where = row.prefix.split(".")
        if where[0] == "mid":
            setattr(net.mid, where[1], m)
        elif len(where) == 4:                      # down.1.block.0: the blocks of a level come in index order
            getattr(stack[int(where[1])], where[2]).append(m)
        else:                                      # up.2.upsample
            setattr(stack[int(where[1])], where[2], m)
        steps.append((f"{name}.{row.prefix}", row, m))
    net.norm_out = gn(half.norm_out)
    net.conv_out = nn.Conv2d(*half.conv_out, 3, padding=1)
    return net, steps


class VectorQuantizer(nn.Module):
    """taming.modules.vqvae.quantize.VectorQuantizer2 (third-party, not under /root/reference; call sites autoencoder.py:39-41, 277):
    codebook `embedding` [n_e, e_dim]; forward(z) -> (z_q, loss, (perplexity, min_encodings, min_encoding_indices)). The eval path
    computes d = |z|^2 + |e|^2 - 2 z.e per latent pixel, takes argmin, looks the entry up and returns z + (z_q - z).detach()."""

    def __init__(self, n_e, e_dim, beta=0.25, remap=None, unknown_index="random", sane_index_shape=False, legacy=True):
        super().__init__()
        if remap is not None:
            raise NotImplementedError("VectorQuantizer remap is not used by vq-f4.yaml")
        self.n_e, self.e_dim, self.beta, self.legacy = n_e, e_dim, beta, legacy
        self.sane_index_shape = sane_index_shape
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)

    @torch.no_grad()
    def forward(self, z, temp=None, rescale_logits=False, return_logits=False):
        idx, z_q = ops.vq_nearest(z.float().contiguous(), self.embedding.weight.detach().float().contiguous())
        ind = idx if self.sane_index_shape else idx.reshape(-1)
        return z_q, None, (None, None, ind)

    @torch.no_grad()
    def get_codebook_entry(self, indices, shape):
        z_q = self.embedding.weight[indices.reshape(-1)]
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q


class _Packed:
    __slots__ = ("hi", "lo", "bias", "frag", "extra", "frag16", "extra_src")

    def __init__(self, hi, lo, bias, frag=None, extra=None, frag16=None, extra_src=None):
        self.hi, self.lo, self.bias, self.frag, self.extra, self.frag16, self.extra_src = hi, lo, bias, frag, extra, frag16, extra_src


class FirstStageEngine(nn.Module):
    """What the frozen first stages share (VQModelInterface, AutoencoderKL): the reference's Encoder / Decoder (model.py:368-568) built from
    `first_stage_layout`, their weight packing (`_prepare`) and the walk over the layout's rows on the HIP kernels (`_encoder`, `_decoder`).
    A subclass calls `_build_halves` first (it registers `encoder` and `decoder`, so they lead the state dict as in the reference), then
    registers its own modules — `quant_conv` and `post_quant_conv` among them — and ends its constructor with `_freeze`."""

    def _build_halves(self, ddconfig, precision):
        self.layout = first_stage_layout(**dict(ddconfig))
        self._steps = {}                              # per half: [(buffer tag, row, leaves)] in execution order
        for name in ("encoder", "decoder"):
            net, self._steps[name] = _containers(name, getattr(self.layout, name), self.layout.levels)
            setattr(self, name, net)
        self.encoder.num_resolutions = self.layout.levels      # latent_diffusion.latent_mask checks an image mask's factor against it
        self.precision = Precision.parse(precision) if isinstance(precision, str) else precision
        self.batch_invariant = False                  # True: encode / decode give a sample the same bits in every batch (see _ws)
        self._packed: Dict = {}
        self._pack_key = None
        self._bufs: Dict[Tuple, torch.Tensor] = {}
        self._cs: Dict[int, torch.Tensor] = {}

    def _freeze(self, ckpt_path, ignore_keys):
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)
        for p in self.parameters():                   # instantiate_first_stage freezes it (ddpm.py:530-535)
            p.requires_grad = False

    def init_from_ckpt(self, path, ignore_keys=()):
        """autoencoder.py:78-90, 313-322."""
        # a third-party checkpoint (vq-f4.ckpt, kl-f8's model.ckpt): tensors only, never a full unpickle — if the safe loader refuses the file, say so and stop
        try:
            ck = torch.load(path, map_location="cpu", weights_only=True)
        except Exception as e:
            raise RuntimeError(f"{path}: torch.load(weights_only=True) refused this checkpoint ({type(e).__name__}: {e}); it is not loaded "
                               f"with a full unpickle — re-save its state_dict as plain tensors (e.g. safetensors)") from e
        sd = ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        missing, unexpected = self.load_state_dict(sd, strict=False)
        print(f"Restored from {path} with {len(missing)} missing and {len(unexpected)} unexpected keys")

    def set_precision(self, precision) -> None:
        self.precision = Precision.parse(precision) if isinstance(precision, str) else precision
        self._packed.clear()
        self._pack_key = None

    # ------------------------------------------------------------------------------------------------ engine plumbing
    def _buf(self, name, shape, dtype=torch.float32):
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = torch.empty(tuple(shape), dtype=dtype, device=self.quant_conv.weight.device)
            self._bufs[key] = t
        return t

    def _planes(self, shape, kind="a16"):
        hi = self._buf(f"{kind}.hi", shape, torch.int16)
        lo = self._buf(f"{kind}.lo", shape, torch.int16) if self.precision.npass == 3 else None
        return hi, lo

    def _cs_new(self, t, nslab=None):
        B, C = t.shape[0], t.shape[-1]
        HW = t.numel() // (B * C)
        cs = self._buf(f"cs.{t.data_ptr()}", (B, nslab or ops.gn_chan_nslab(HW), C, 2))
        self._cs[t.data_ptr()] = cs
        return cs

    def _chan_stats(self, t):
        cs = self._cs.get(t.data_ptr())
        if cs is None:
            cs = self._cs_new(t)
            ops.gn_chan_stats(t, cs)
        return cs

    def _norm16(self, norm: Optional[nn.GroupNorm], act: int, x, want_raw=False, kind="a16"):
        """act(GroupNorm(x)) (norm None: plain conversion) as 16-bit operand planes; want_raw: also the plain conversion of x (operand of
        the 1x1 nin_shortcut), from the same pass."""
        hi, lo = self._planes(tuple(x.shape), kind)
        if norm is None:
            ops.gn_apply16(x, None, hi, lo, self.precision)
            return hi, lo
        raw = self._planes(tuple(x.shape), "raw16") if want_raw else None
        ops.gn_apply16c(x, self._chan_stats(x), None, None, hi, lo, self.precision, norm.weight, norm.bias, norm.eps, norm.num_groups, act, 0, raw)
        return ((hi, lo), raw) if want_raw else (hi, lo)

    def _ws(self, nel):
        # batch_invariant: no split-K workspace, so no convolution splits its K walk. The split is chosen from the number of tiles in the launch,
        # i.e. from the batch; without it a sample's result does not depend on which other samples share its call.
        if nel > (1 << 23) or self.batch_invariant:
            return None
        return self._buf("conv_ws", ((16 if nel <= (1 << 20) else (4 if nel <= (1 << 22) else 2)) * nel,))

    def _prepare(self):
        params = list(self.parameters())
        dev = params[0].device
        if dev.type != "cuda":
            raise StedmHipError(f"{type(self).__name__} needs its parameters on the GPU; there is no CPU fallback")
        key = (self.precision, dev, tuple(p._version for p in params), tuple(p.data_ptr() for p in params))
        if key == self._pack_key:
            return
        self._packed.clear()
        prec = self.precision
        one = Precision(prec.mm_dtype, 1)

        def pack(conv):
            w4 = conv.weight.detach().float().contiguous()
            ks = w4.shape[-1]
            hi = lo = frag = None
            ok = (ks == 3 and conv.in_channels % 16 == 0) or (ks == 1 and conv.in_channels % 64 == 0)
            frag16 = None
            if prec.npass == 1 and ok and conv.stride == (1, 1):
                # both fragment orders (the stage is frozen: packed once): the 16x16x32 MFMA kind takes a 3x3 from 256 input channels on
                # unless its two-plane chunk ring does not fit LDS (rows of 256+ pixels), where the 32x32x16 kind runs
                frag = ops.pack_conv_weight_frag(w4, prec)
                if conv.in_channels % 32 == 0:
                    frag16 = ops.pack_conv_weight_frag16(w4, prec)
                hi = ops.LazyPlanes(lambda w=w4: ops.pack_conv_weight(w, prec))
            else:
                hi, lo = ops.pack_conv_weight(w4, prec)
            self._packed[id(conv)] = _Packed(hi, lo, None if conv.bias is None else conv.bias.detach().float().contiguous(), frag, None, frag16,
                                             extra_src=w4 if (prec.npass == 3 and ks == 3) else None)

        for _, row, m in self._steps["encoder"] + self._steps["decoder"]:
            if row.kind == "res":
                pack(m.conv1); pack(m.conv2)
                if row.cin != row.cout:
                    pack(m.nin_shortcut)
            elif row.kind == "attn":
                for c in (m.q, m.k, m.v, m.proj_out):
                    pack(c)
            elif row.kind == "up":
                pack(m.conv)                                   # the plain 3x3 form, for inputs too wide for the sub-pixel kernel's LDS ring
                self._packed[("plain", id(m.conv))] = self._packed.pop(id(m.conv))
                w = m.conv.weight.detach().float().contiguous()
                hi, lo = ops.pack_conv_weight_up(w, prec)
                frag = ops.pack_conv_weight_up_frag(w, prec) if prec.npass == 1 and row.cin % 32 == 0 else None
                self._packed[id(m.conv)] = _Packed(hi, lo, m.conv.bias.detach().float().contiguous(), frag)
            else:
                # "down": bottom/right-padded stride-2 conv as a 2x2 conv over space-to-depth planes (register-streamed kernel, single
                # product); the 3-product parity mode runs it as hi*hi + lo*hi + hi*lo with the residual weights packed beside
                w = m.conv.weight.detach().float().contiguous()
                frag = ops.pack_conv_weight_s2d_frag(w, one, pad_br=True)
                extra = None
                if prec.npass == 3:
                    wh = w.to(torch.float16 if prec.mm_dtype == 0 else torch.bfloat16).float()
                    extra = ops.pack_conv_weight_s2d_frag((w - wh).contiguous(), one, pad_br=True)
                self._packed[id(m.conv)] = _Packed(None, None, m.conv.bias.detach().float().contiguous(), frag, extra)
        ci = self.decoder.conv_in
        wpad = torch.zeros((ci.out_channels, 32, 3, 3), dtype=torch.float32, device=dev)
        wpad[:, :ci.in_channels].copy_(ci.weight.detach().float())
        hi, lo = ops.pack_conv_weight(wpad, prec)
        self._packed[id(ci)] = _Packed(hi, lo, ci.bias.detach().float().contiguous(),
                                       ops.pack_conv_weight_frag(wpad, prec) if prec.npass == 1 else None)
        self._out_w = {id(c): ops.conv_out_weight(c.weight) for c in (self.encoder.conv_out, self.decoder.conv_out)}
        self._pack_key = key

    # ------------------------------------------------------------------------------------------------ block runners (NHWC fp32)
    def _wide3(self, pk, src16, out, res, stats):
        """3x3 on rows of 256+ pixels in the 3-product parity mode: only the register-streamed kernel tiles such rows and it is a
        single-product kernel, so the three products run as three launches over the hi / lo planes (lo*hi + hi*lo + hi*hi, fp32
        accumulation through `res`), with the weight's hi part and residual packed in fragment order on first use"""
        prec = self.precision
        one = Precision(prec.mm_dtype, 1)
        if pk.extra is None:
            w = pk.extra_src
            wh = w.to(torch.float16 if prec.mm_dtype == 0 else torch.bfloat16).float()
            pk.extra = (ops.pack_conv_weight_frag(wh, one), ops.pack_conv_weight_frag((w - wh).contiguous(), one))
        fh, fl = pk.extra
        lazy = lambda: ops.LazyPlanes(lambda: (_ for _ in ()).throw(StedmHipError("wide 3-product conv: the register-streamed kernel refused the shape")))
        ws = self._ws(out.numel())
        ops.conv_igemm(None, lazy(), None, out, prec=one, src16=(src16[1], None), w_frag=fh, res=res, ws=ws)
        ops.conv_igemm(None, lazy(), None, out, prec=one, src16=(src16[0], None), w_frag=fl, res=out, ws=ws)
        return ops.conv_igemm(None, lazy(), None, out, prec=one, src16=(src16[0], None), w_frag=fh, bias=pk.bias, res=out, ws=ws,
                              chan_stats=self._cs_new(out) if stats else None)

    def _conv(self, pk, src16, out, ks=3, res=None, stats=True, **kw):
        if self.precision.npass == 3 and ks == 3 and out is not None and src16[0].shape[2] >= 256 and not kw:
            return self._wide3(pk, src16, out, res, stats)
        nel = out.numel() if out is not None else src16[0].numel() // src16[0].shape[-1] * kw["out16"][0].shape[-1]
        return ops.conv_igemm(None, pk.hi, pk.lo, out, prec=self.precision, ks=ks, src16=src16, bias=pk.bias, res=res, w_frag=pk.frag,
                              chan_stats=self._cs_new(out) if (stats and out is not None) else None, ws=self._ws(nel),
                              w_frag16=pk.frag16 if ks == 3 else None, **kw)

    def _res(self, tag, row, rb, x):
        """ResnetBlock.forward model.py:117-140 with temb None."""
        B, H, W, _ = x.shape
        co = row.cout
        has_skip = row.cin != co
        if has_skip:
            a16, x16 = self._norm16(rb.norm1, 1, x, want_raw=True)
        else:
            a16 = self._norm16(rb.norm1, 1, x)
        h = self._buf(f"h.{B}x{H}x{W}x{co}", (B, H, W, co))
        self._conv(self._packed[id(rb.conv1)], a16, h)
        out = self._buf(tag + ".out", (B, H, W, co))
        pk2 = self._packed[id(rb.conv2)]
        h16 = self._norm16(rb.norm2, 1, h, kind="h16")
        if not has_skip:
            return self._conv(pk2, h16, out, res=x)
        ps = self._packed[id(rb.nin_shortcut)]
        fkey = ("fuse", id(rb), B, H, W)
        fused = self._packed.get(fkey)
        kw = dict(prec=self.precision, src16=h16, bias=pk2.bias, w_frag=pk2.frag, chan_stats=self._cs_new(out), ws=self._ws(out.numel()),
                  w_frag16=pk2.frag16)
        if fused is None:
            fused = bool((pk2.frag is not None or pk2.frag16 is not None) and ps.frag is not None and
                         ops.conv_igemm(None, pk2.hi, pk2.lo, out, skip=(x16[0], ps.frag, ps.bias, ps.frag16), query_fused=True, **kw))
            self._packed[fkey] = fused
        if fused:
            return ops.conv_igemm(None, pk2.hi, pk2.lo, out, skip=(x16[0], ps.frag, ps.bias, ps.frag16), **kw)
        M = B * H * W        # the unfused 1x1 as one long "image" (per-pixel work: no sample structure needed, any H*W admitted)
        flat = lambda t: None if t is None else t.view(1, 1, M, t.shape[-1])
        self._conv(ps, (flat(x16[0]), flat(x16[1])), flat(out), ks=1, stats=False)
        if self.precision.npass == 3 and W >= 256:
            return self._wide3(pk2, h16, out, out, True)
        return ops.conv_igemm(None, pk2.hi, pk2.lo, out, res=out, **kw)

    def _attn(self, tag, row, ab, x):
        """AttnBlock.forward model.py:168-199: single head of width C over T = H*W tokens, logits scaled by C^-0.5, fp32 softmax.
        Per sample: S = Q K^T and O = P V as GEMMs on the convolution kernels (K and V^T packed as their weight operand), the
        T x T logits materialised once per sample (as the reference's bmm does)."""
        prec = self.precision
        B, H, W, C = x.shape
        T = H * W
        if T % 64 != 0 or C % 64 != 0:
            raise StedmHipError(f"VQ AttnBlock: H*W = {T} and C = {C} must be multiples of 64")
        n16 = self._norm16(ab.norm, 0, x)
        q16 = self._planes((B, H, W, C), "q16")
        self._conv(self._packed[id(ab.q)], n16, None, ks=1, stats=False, out16=q16)
        k = self._buf(f"{tag}.k", (B, H, W, C)); v = self._buf(f"{tag}.v", (B, H, W, C))
        self._conv(self._packed[id(ab.k)], n16, k, ks=1, stats=False)
        self._conv(self._packed[id(ab.v)], n16, v, ks=1, stats=False)
        att = self._buf(f"{tag}.att", (B, H, W, C))
        S = self._buf("attn.S", (T, T))
        P16 = self._planes((T, T), "attn.P")
        frag_ok = prec.npass == 1

        def operand(mat, sn, sc, cout, cin):
            """(w_hi, w_lo, w_frag) of the GEMM's weight operand W[n][ci] = mat.flatten()[n * sn + ci * sc]: fragment order for the
            register-streamed kernel (its [cout][cin] planes only when a problem falls to the LDS-operand kernels), hi / lo planes in
            the 3-product mode"""
            args = (mat, sn, sc, False, cout, cin, 1, prec)
            if frag_ok:
                frag = ops.pack_conv_weight_strided(*args, want_hi=False, want_frag=True)[2]
                return ops.LazyPlanes(lambda: ops.pack_conv_weight_strided(*args, want_hi=True, want_frag=False)[:2]), None, frag
            hi, lo, _ = ops.pack_conv_weight_strided(*args, want_hi=True, want_frag=False)
            return hi, lo, None

        for b in range(B):
            kh, kl, kf = operand(k[b], C, 1, T, C)                      # W[key t][channel c] = K[t][c]
            src = (q16[0][b].view(1, 1, T, C), None if q16[1] is None else q16[1][b].view(1, 1, T, C))
            ops.conv_igemm(None, kh, kl, S.view(1, 1, T, T), prec=prec, ks=1, src16=src, w_frag=kf, ws=self._ws(T * T))
            ops.softmax_rows16(S, float(C) ** -0.5, P16[0], P16[1], prec)
            vh, vl, vf = operand(v[b], 1, C, C, T)                      # W[channel c][key t] = V[t][c]
            ops.conv_igemm(None, vh, vl, att[b].view(1, 1, T, C), prec=prec, ks=1,
                           src16=(P16[0].view(1, 1, T, T), None if P16[1] is None else P16[1].view(1, 1, T, T)), w_frag=vf, ws=self._ws(T * C))
        out = self._buf(tag + ".out", (B, H, W, C))
        return self._conv(self._packed[id(ab.proj_out)], self._norm16(None, 0, att, kind="att16"), out, ks=1, res=x)

    def _up(self, tag, row, up, x):
        """Upsample.forward model.py:53-57: nearest x2 then conv 3x3, evaluated in the sub-pixel form (4 output parities x 2x2 taps)."""
        B, H, W, C = x.shape
        pk = self._packed[id(up.conv)]
        out = self._buf(tag + ".out", (B, 2 * H, 2 * W, C))
        src16 = self._norm16(None, 0, x, kind="up16")
        if W >= 256:
            # input rows of 256+ pixels (the 512^2 level of the shipped config): the sub-pixel kernel's two-plane chunk ring does not fit
            # LDS there; the nearest-x2 plane is materialised in 16 bits (a layout copy) and the plain 3x3 runs on it (9/4 of the MACs)
            up16 = self._planes((B, 2 * H, 2 * W, C), "upx2")
            for s16, d16 in zip(src16, up16):
                if s16 is not None:
                    d16.view(B, H, 2, W, 2, C).copy_(s16.view(B, H, 1, W, 1, C).expand(B, H, 2, W, 2, C))
            return self._conv(self._packed[("plain", id(up.conv))], up16, out)
        return ops.conv_igemm(None, pk.hi, pk.lo, out, prec=self.precision, mode=CONV_UP_SUBPIXEL, src16=src16,
                              bias=pk.bias, w_frag=pk.frag, chan_stats=self._cs_new(out, 4 * ops.gn_chan_nslab(H * W)))

    def _down(self, tag, row, dn, x):
        """Downsample.forward model.py:69-79: zero pad bottom/right by one, conv 3x3 stride 2."""
        B, H, W, C = x.shape
        if H % 2 or W % 2:
            raise StedmHipError("VQ Downsample needs even H, W")
        pk = self._packed[id(dn.conv)]
        prec = self.precision
        one = Precision(prec.mm_dtype, 1)
        hi = self._buf(f"s2d.hi.{B}x{H}x{W}x{C}", (B, H // 2, W // 2, 4 * C), torch.int16)
        lo = self._buf(f"s2d.lo.{B}x{H}x{W}x{C}", (B, H // 2, W // 2, 4 * C), torch.int16) if prec.npass == 3 else None
        ops.space_to_depth16(x, hi, lo, prec)
        out = self._buf(tag + ".out", (B, H // 2, W // 2, C))
        ws = self._ws(out.numel())
        if prec.npass == 1:
            return ops.conv_igemm(None, None, None, out, prec=one, mode=CONV_S2D, src16=(hi, None), bias=pk.bias, w_frag=pk.frag, chan_stats=self._cs_new(out),
                                  ws=ws, pad_br=True)
        ops.conv_igemm(None, None, None, out, prec=one, mode=CONV_S2D, src16=(lo, None), bias=None, w_frag=pk.frag, ws=ws, pad_br=True)
        ops.conv_igemm(None, None, None, out, prec=one, mode=CONV_S2D, src16=(hi, None), bias=None, w_frag=pk.extra, res=out, ws=ws, pad_br=True)
        return ops.conv_igemm(None, None, None, out, prec=one, mode=CONV_S2D, src16=(hi, None), bias=pk.bias, w_frag=pk.frag, res=out,
                              chan_stats=self._cs_new(out), ws=ws, pad_br=True)

    # ------------------------------------------------------------------------------------------------ encoder / decoder
    def _walk(self, name, h):
        """the rows of one half in execution order, then GroupNorm + SiLU + conv_out; NHWC in, NCHW out"""
        for tag, row, m in self._steps[name]:
            h = getattr(self, "_" + row.kind)(tag, row, m, h)
        net = getattr(self, name)
        n, co = net.norm_out, net.conv_out
        out = torch.empty((h.shape[0], co.out_channels, h.shape[1], h.shape[2]), dtype=torch.float32, device=h.device)
        return ops.conv_out(h, n.weight, n.bias, n.eps, n.num_groups, self._out_w[id(co)], co.bias, out, self._chan_stats(h))

    @torch.no_grad()
    def _encoder(self, x):
        """Encoder.forward model.py:433-459. x [B,3,H,W] NCHW -> [B,z,H/4,W/4] NCHW."""
        ci = self.encoder.conv_in
        B, _, H, W = x.shape
        h = self._buf("enc.in", (B, H, W, ci.out_channels))
        cs = self._cs_new(h, H // 2) if H % 2 == 0 else None
        if not ops.conv_in(x, None, ci.weight, ci.bias, h, chan_stats=cs) and cs is not None:
            del self._cs[h.data_ptr()]
        return self._walk("encoder", h)

    @torch.no_grad()
    def _decoder(self, z):
        """Decoder.forward model.py:528-568. z [B,zc,h,w] NCHW -> [B,out_ch,4h,4w] NCHW."""
        ci = self.decoder.conv_in
        B, _, H, W = z.shape
        h = self._buf("dec.in", (B, H, W, ci.out_channels))
        # z_channels (3 or 4) -> the coarsest level's width: zero-padded to 32 channels (layout shuffle) and run on the MFMA kernels like
        # every other conv
        zp = self._buf("dec.zpad", (B, H, W, 32))
        zp.zero_()
        zp[..., :z.shape[1]].copy_(z.permute(0, 2, 3, 1))
        self._conv(self._packed[id(ci)], self._norm16(None, 0, zp, kind="z16"), h)
        return self._walk("decoder", h)


class VQModelInterface(FirstStageEngine):
    """autoencoder.py:264-282 over VQModel (:14-110). Extra (non-reference) argument: `precision` (ops.Precision name; the parity mode
    is the one asserted against the oracle, bf16 / f16 are the single-product fast modes)."""

    def __init__(self, embed_dim, ddconfig=None, lossconfig=None, n_embed=None, ckpt_path=None, ignore_keys=(), image_key="image",
                 colorize_nlabels=None, monitor=None, batch_resize_range=None, scheduler_config=None, lr_g_factor=1.0, remap=None,
                 sane_index_shape=False, use_ema=False, precision: str = "parity"):
        super().__init__()
        if ddconfig is None or n_embed is None:
            raise TypeError("VQModelInterface needs ddconfig and n_embed (conf/diffusion/first_stage_config/vq-f4.yaml)")
        if use_ema or colorize_nlabels is not None or batch_resize_range is not None:
            raise NotImplementedError("use_ema / colorize_nlabels / batch_resize_range: training-side options of VQModel, unused by the frozen stage")
        self.embed_dim, self.n_embed, self.image_key = embed_dim, n_embed, image_key
        dd = dict(ddconfig)
        self._build_halves(dd, precision)
        self.loss = nn.Identity()                     # lossconfig: torch.nn.Identity (vq-f4.yaml:22-23)
        self.quantize = VectorQuantizer(n_embed, embed_dim, beta=0.25, remap=remap, sane_index_shape=sane_index_shape)
        self.quant_conv = nn.Conv2d(dd["z_channels"], embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, dd["z_channels"], 1)
        if monitor is not None:
            self.monitor = monitor
        self._freeze(ckpt_path, ignore_keys)

    # ------------------------------------------------------------------------------------------------ the reference's surface
    @torch.no_grad()
    def encode(self, x):
        """autoencoder.py:269-272: encoder + quant_conv, NO quantisation (the latents of the diffusion model are pre-quant)."""
        self._prepare()
        self._cs = {}
        h = self._encoder(x.float().contiguous())
        return ops.conv1x1_nchw(h, self.quant_conv.weight, self.quant_conv.bias)

    @torch.no_grad()
    def decode(self, h, force_not_quantize=False):
        """autoencoder.py:274-282: quantise (unless told not to), post_quant_conv, decoder."""
        self._prepare()
        self._cs = {}
        h = h.float().contiguous()
        if not force_not_quantize:
            quant, _, _ = self.quantize(h)
        else:
            quant = h
        quant = ops.conv1x1_nchw(quant, self.post_quant_conv.weight, self.post_quant_conv.bias)
        return self._decoder(quant)

    @torch.no_grad()
    def decode_code(self, code_b):
        """autoencoder.py:107-110 (through the interface's decode without re-quantising)."""
        quant_b = self.quantize.get_codebook_entry(code_b, tuple(code_b.shape) + (self.embed_dim,))
        return self.decode(quant_b, force_not_quantize=True)

    def forward(self, input, return_pred_indices=False):
        raise NotImplementedError("VQModel.forward (autoencoder training) is outside the frozen first stage")


CONV_OUT_MAX = 8      # output channels stedm_conv_out writes (the encoder's conv_out of a KL stage has 2 * z_channels)


class AutoencoderKL(FirstStageEngine):
    """autoencoder.py:285-342: the KL first stage (kl-f4, kl-f8, ...), frozen. The encoder's conv_out writes 2 * z_channels moments,
    `quant_conv` maps them to 2 * embed_dim and `encode` returns their DiagonalGaussianDistribution; `decode` is `post_quant_conv` and the
    decoder. Encoder, decoder and the glue convolutions run on the engine VQModelInterface uses; the posterior's sample is
    stedm_gauss_sample (stedm_amd/distributions.py). Extra (non-reference) argument: `precision`, as on VQModelInterface."""

    def __init__(self, ddconfig, lossconfig, embed_dim, ckpt_path=None, ignore_keys=(), image_key="image", colorize_nlabels=None, monitor=None,
                 precision: str = "parity"):
        super().__init__()
        dd = dict(ddconfig)
        if not dd.get("double_z", True):
            raise ValueError("AutoencoderKL needs ddconfig['double_z'] true: the encoder emits the mean and the log-variance "
                             "(the reference asserts it, autoencoder.py:301)")
        if 2 * dd["z_channels"] > CONV_OUT_MAX or 2 * embed_dim > 16:
            raise NotImplementedError(f"AutoencoderKL: the encoder's conv_out writes 2 * z_channels = {2 * dd['z_channels']} channels; "
                                      f"stedm_conv_out covers up to {CONV_OUT_MAX} (z_channels <= {CONV_OUT_MAX // 2}: kl-f4, kl-f8) and the glue "
                                      f"convolutions up to 16 (embed_dim <= 8)")
        if colorize_nlabels is not None:
            raise NotImplementedError("colorize_nlabels: a logging option of the autoencoder's own training, unused by the frozen stage")
        self.embed_dim, self.image_key = embed_dim, image_key
        self._build_halves(dd, precision)
        self.loss = nn.Identity()                     # whatever lossconfig names (LPIPSWithDiscriminator): a checkpoint's loss.* keys are dropped
        self.quant_conv = nn.Conv2d(2 * dd["z_channels"], 2 * embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, dd["z_channels"], 1)
        if monitor is not None:
            self.monitor = monitor
        self._freeze(ckpt_path, ignore_keys)

    @torch.no_grad()
    def encode(self, x):
        """autoencoder.py:324-328: encoder, quant_conv -> the posterior over the latents."""
        from .distributions import DiagonalGaussianDistribution
        self._prepare()
        self._cs = {}
        h = self._encoder(x.float().contiguous())
        return DiagonalGaussianDistribution(ops.conv1x1_nchw(h, self.quant_conv.weight, self.quant_conv.bias))

    @torch.no_grad()
    def decode(self, z, *args, **kwargs):
        """autoencoder.py:330-333: post_quant_conv, decoder."""
        self._prepare()
        self._cs = {}
        z = ops.conv1x1_nchw(z.float().contiguous(), self.post_quant_conv.weight, self.post_quant_conv.bias)
        return self._decoder(z)

    @torch.no_grad()
    def forward(self, input, sample_posterior=True):
        """autoencoder.py:335-342 -> (dec, posterior)."""
        posterior = self.encode(input)
        z = posterior.sample() if sample_posterior else posterior.mode()
        return self.decode(z), posterior


class IdentityFirstStage(nn.Module):
    """autoencoder.py:426-443: a diffusion model over the pixels themselves."""

    def __init__(self, *args, vq_interface=False, **kwargs):
        super().__init__()
        self.vq_interface = vq_interface

    def encode(self, x, *args, **kwargs):
        return x

    def decode(self, x, *args, **kwargs):
        return x

    def quantize(self, x, *args, **kwargs):
        return (x, None, [None, None, None]) if self.vq_interface else x

    def forward(self, x, *args, **kwargs):
        return x
