"""DDIM sampler with sequential-equivalent classifier-free guidance and std-rescale, HIP-backed.

Mirrors `ldm.models.diffusion.ddim.DDIMSampler` (reference ddim.py:11-210): same constructor,
`make_schedule`, `sample`, `ddim_sampling`, `p_sample_ddim` names / argument meaning / returns.
Host logic (schedule tables, the python loop) stays on the host as in the reference; every tensor
operation of the loop body runs in HIP kernels:
  * the two `apply_model` calls of ddim.py:177-178 -> one shared-encoder CFG pass (`apply_model_cfg`)
    when the model offers it, else two calls in the reference's order (cond, then uncond);
  * ddim.py:179-184 (CFG combine + (C,H)-std rescale, phi = 0.7) and :195-210 (x0 / direction / noise)
    -> one fused kernel (stedm_ddim_step);
  * masked sampling, ddim.py:143-146 (q_sample of x0 blended into img before the U-Net call) -> one kernel
    (stedm_ddim_mask_blend) whose noise is drawn in it from the device step index, so it is captured with the step;
  * with `use_graph=True` the whole step (timestep fill, U-Net, update, counter decrement) is captured
    once in a hipGraph and replayed per step, per-step scalars coming from a device table;
  * temperature / noise_dropout (ddim.py:206-208) and the step noise drawn from (noise_seed, sample id) -> stedm_ddim_step_ex, the same
    kernel with compile-time options; quantize_x0 (ddim.py:201-203) -> one more kernel after it (stedm_ddim_quantize_x0);
  * one guidance scale per sample (a sequence or 1-D tensor as unconditional_guidance_scale) -> stedm_ddim_step_rows, which reads the
    scales from a device array, so a captured step serves any scales (StepGraph.set_scales).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .schedule import DDIMTables, make_ddim_tables


def first_stage_codebook(model, C, option):
    """The first stage's codebook [n_e, C] fp32 on the model's device for the samplers' `option` (quantize_x0 / quantize_denoised):
    NotImplementedError without a VQ first stage, ValueError when its width is not the latents' channel count C - both before any
    device work."""
    emb = getattr(getattr(getattr(model, "first_stage_model", None), "quantize", None), "embedding", None)
    if emb is None:
        fs = getattr(model, "first_stage_model", None)
        raise NotImplementedError(f"{option} needs a VQ first stage (first_stage_model.quantize.embedding); this model's first stage is "
                                  f"{'absent' if fs is None else type(fs).__name__}, which has no codebook")
    w = emb.weight
    if w.dim() != 2 or int(w.shape[1]) != int(C):
        raise ValueError(f"{option}: codebook {tuple(w.shape)} has width {w.shape[-1]}, the latents have {C} channels")
    return w.detach().to(model.device).float().contiguous()


def guidance_rows(scale, batch_size):
    """unconditional_guidance_scale as the samplers take it -> None for one scale (a Python / numpy number or a 0-d tensor: today's path),
    else the per-sample scales as a list of `batch_size` finite floats (a sequence or a 1-D tensor). ValueError on a wrong length, a
    non-finite value or more than one dimension. Host work only."""
    if isinstance(scale, torch.Tensor):
        if scale.dim() == 0:
            return None
        vals = scale.detach().cpu().double().numpy()
    elif isinstance(scale, np.ndarray):
        if scale.ndim == 0:
            return None
        vals = scale.astype(np.float64)
    elif isinstance(scale, (list, tuple)):
        try:
            vals = np.asarray(scale, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"unconditional_guidance_scale {scale!r}: per-sample scales must be a flat sequence of numbers") from e
    else:
        return None
    if vals.ndim != 1 or vals.shape[0] != int(batch_size):
        raise ValueError(f"unconditional_guidance_scale of shape {tuple(vals.shape)}: per-sample scales must be 1-D of length batch_size = "
                         f"{int(batch_size)}")
    if not np.isfinite(vals).all():
        raise ValueError(f"unconditional_guidance_scale holds a non-finite value: {vals.tolist()}")
    return [float(v) for v in vals]


def refuse_guidance_rows(scale, who):
    """The samplers without per-sample guidance scales: NotImplementedError for anything guidance_rows would read as rows."""
    if (isinstance(scale, (torch.Tensor, np.ndarray)) and scale.ndim > 0) or isinstance(scale, (list, tuple)):
        raise NotImplementedError(f"{who} takes one unconditional_guidance_scale for the batch; per-sample scales are DDIMSampler's "
                                  "(stedm_ddim_step_rows)")


class _StepOpts:
    """What stedm_ddim_step_ex needs beyond stedm_ddim_step: iterations of the run, temperature, noise dropout, the in-kernel draw, the
    seed of the draw and of the keep bits, the first global sample id, the codebook of quantize_x0 (or None)."""

    def __init__(self, n_iters, temperature, noise_dropout, draw, seed, first_id, codebook):
        self.n_iters, self.temperature, self.noise_dropout, self.draw = n_iters, temperature, noise_dropout, draw
        self.seed, self.first_id, self.codebook = seed, first_id, codebook


class DDIMSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.use_graph = bool(kwargs.get("use_graph", False))
        self._graph_cache = {}

    def register_buffer(self, name, attr):
        """ddim.py:18-22 moves tensors to "cuda"; here: to the model's device."""
        if isinstance(attr, torch.Tensor) and attr.device != self.model.device:
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """ddim.py:24-53 — tables built on the host from the model's fp32 alphas_cumprod buffer."""
        acp = self.model.alphas_cumprod
        assert acp.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        tb: DDIMTables = make_ddim_tables(acp.detach().cpu().numpy(), ddim_num_steps, float(ddim_eta))
        self.tables = tb
        self.ddim_timesteps = tb.timesteps
        dev = self.model.device
        self.register_buffer('ddim_sigmas', torch.from_numpy(tb.sigmas))
        self.register_buffer('ddim_alphas', torch.from_numpy(tb.alphas))
        self.register_buffer('ddim_alphas_prev', torch.from_numpy(tb.alphas_prev))
        self.register_buffer('ddim_sqrt_one_minus_alphas', torch.from_numpy(tb.sqrt_one_minus_alphas))
        self._coefs = torch.from_numpy(tb.coef_table()).to(dev).contiguous()       # [n][4] device table
        self._ts_table = torch.from_numpy(tb.timesteps.astype(np.int64)).to(dev)    # [n] int64
        self._idx_all = torch.arange(tb.timesteps.shape[0], dtype=torch.int32, device=dev)
        self._eta = float(ddim_eta)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        """ddim.py:56-110.

        Masked sampling (ddim.py:143-146): with `mask` (and `x0`, required with it) every step starts with
        img = q_sample(x0, t) * mask + (1 - mask) * img — mask == 1 keeps x0, mask == 0 generates, soft values blend. x0 is
        [B, C, H, W] (a batch-1 x0 is refused: the reference's one batch-shaped noise draw shared by every sample cannot be reproduced by
        per-sample streams); mask is [B|1, 1|C, H, W]. Repo-specific keywords: `mask_noises` (one N(0,1) tensor per iteration in place
        of q_sample's draw; eager loop), else the draw is made in the kernel from `mask_seed` (default: one draw from torch's CPU
        generator per call) and the global sample id `sample_id0 + b` (ops.ddim_mask_blend).

        temperature / noise_dropout (ddim.py:206-208): noise = ((sigma_t z) temperature), then dropout with keep bits drawn in the kernel
        (include/stedm_hip.h, stedm_ddim_step_ex; torch's F.dropout stream cannot be reproduced, its rule and scale are kept). quantize_x0
        (ddim.py:202-203): pred_x0 snapped to the first stage's codebook every step (needs first_stage_model.quantize.embedding, width C).
        With eta == 0 the noise term is zero, so temperature and noise_dropout change nothing. `noise_seed` (repo-specific, the ancestral
        sampler's name): the step noise of eta > 0 is drawn in the kernel as row sample_id0 + b of ops.philox_normal(noise_seed, stream
        1 + iteration) - what predict_latents_sharded fed as `noises` - and the loop can be graphed; without it the step noise comes from
        torch.randn per step (or `noises`) and the dropout bits from a seed drawn once per call from torch's CPU generator.

        unconditional_guidance_scale may be a sequence or a 1-D tensor of batch_size finite scales, one per sample (repo-specific; a
        number or 0-d tensor is the reference's one scale and runs exactly as before). Sample b then equals a run of the whole batch at
        scale[b] (stedm_ddim_step_rows). Without unconditional_conditioning, or with every scale 1, the run is unguided: one forward per
        step, as in the reference. Otherwise every step runs the CFG pass on all rows: a row at scale 1 inside a mixed batch is legal and
        takes the unguided update, but still pays its share of the unconditional decoder rows (there is no ragged forward). eta > 0,
        noises / noise_seed and mask / x0 compose; quantize_x0 and, with eta != 0, temperature != 1 or noise_dropout != 0 are refused
        (NotImplementedError)."""
        if score_corrector is not None:
            raise NotImplementedError("score_corrector: unused by the reference drivers (ldm_diffusion.py:82,90), not implemented")
        if not 0.0 <= float(noise_dropout) < 1.0:
            raise ValueError(f"noise_dropout {noise_dropout} outside [0, 1)")
        self._check_rows(guidance_rows(unconditional_guidance_scale, batch_size), quantize_x0, eta, temperature, noise_dropout)
        codebook = self._codebook(shape[0]) if quantize_x0 else None
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        masking = {}
        if mask is not None:
            masking = self._mask_args(size, mask, x0, kwargs.get("mask_noises"), kwargs.get("mask_seed"), kwargs.get("sample_id0", 0))
        masking.setdefault("sample_id0", int(kwargs.get("sample_id0", 0)))
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, noises=kwargs.get("noises"),
                                  quantize_denoised=quantize_x0, temperature=temperature, noise_dropout=noise_dropout,
                                  noise_seed=kwargs.get("noise_seed"), _codebook=codebook, **masking)

    def _codebook(self, C):
        return first_stage_codebook(self.model, C, "quantize_x0")

    @staticmethod
    def _check_rows(rows, quantize_x0, eta, temperature, noise_dropout):
        """What per-sample guidance scales do not combine with (stedm_ddim_step_rows has none of stedm_ddim_step_ex's options)."""
        if rows is None:
            return
        if quantize_x0:
            raise NotImplementedError("per-sample guidance scales: quantize_x0 is not implemented (stedm_ddim_step_rows has no eps output)")
        if float(eta) != 0.0 and (float(temperature) != 1.0 or float(noise_dropout) != 0.0):
            raise NotImplementedError("per-sample guidance scales with eta != 0: temperature and noise_dropout are not implemented")

    def _step_opts(self, temperature, noise_dropout, codebook, noise_seed, draw_ok, sample_id0):
        """The options of stedm_ddim_step_ex for this run, or None for stedm_ddim_step (the path and bits of a plain call)."""
        if self._eta == 0.0:                         # sigma == 0: the noise term of ddim.py:206-208 is zero whatever its options
            temperature, noise_dropout, noise_seed = 1.0, 0.0, None
        draw = noise_seed is not None and draw_ok
        if temperature == 1.0 and noise_dropout == 0.0 and codebook is None and not draw:
            return None
        seed = noise_seed
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if noise_dropout > 0.0 else 0
        return _StepOpts(int(self.ddim_timesteps.shape[0]), float(temperature), float(noise_dropout), draw, int(seed), int(sample_id0),
                         codebook)

    def _mask_args(self, size, mask, x0, mask_noises, mask_seed, sample_id0):
        """Checks and device placement of the masked-sampling inputs (see `sample`)."""
        if x0 is None:
            raise ValueError("mask given without x0 (ddim.py:144 asserts x0 is not None)")
        B, C, H, W = size
        dev = self.model.device
        x0 = x0.to(dev).float().contiguous()
        mask = mask.to(dev).float().contiguous()
        if x0.dim() != 4 or tuple(x0.shape[1:]) != (C, H, W) or x0.shape[0] != B:
            raise ValueError(f"x0 {tuple(x0.shape)} must be [{B}, {C}, {H}, {W}] (a batch-1 x0 is not broadcast: per-sample noise streams "
                             "cannot reproduce the reference's one draw shared by the batch)")
        if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, C) or tuple(mask.shape[2:]) != (H, W):
            raise ValueError(f"mask {tuple(mask.shape)} must be [{B}|1, 1|{C}, {H}, {W}]")
        if mask_noises is not None:
            mask_noises = list(mask_noises)
            if len(mask_noises) != self.ddim_timesteps.shape[0]:
                raise ValueError(f"mask_noises holds {len(mask_noises)} tensors for {self.ddim_timesteps.shape[0]} iterations")
        elif mask_seed is None:
            mask_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        return {"mask": mask, "x0": x0, "mask_noises": mask_noises, "mask_seed": None if mask_seed is None else int(mask_seed),
                "sample_id0": int(sample_id0)}

    def _blend(self, img, mask, x0, t, step, noise=None, seed=0, first_id=0):
        """ddim.py:143-146 in place on img (one kernel; q_sample's noise given or drawn in it)."""
        m = self.model
        ops.ddim_mask_blend(img, x0, mask, t, m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, noise=noise, step_idx=step,
                            seed=0 if seed is None else seed, first_id=first_id)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, log_every_t=100,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, noises=None, mask=None, x0=None,
                      mask_noises=None, mask_seed=None, sample_id0=0, quantize_denoised=False, temperature=1., noise_dropout=0.,
                      noise_seed=None, _codebook=None, **kwargs):
        """ddim.py:113-162. `noises` (optional list, one N(0,1) tensor per iteration) replaces the global-RNG
        draw of ddim.py:206 so that runs are reproducible across devices and shard counts. mask / x0 / mask_noises / mask_seed /
        sample_id0: masked sampling, checked and placed by `sample` (the blend runs before the U-Net call; x_inter logs unblended img).
        quantize_denoised / temperature / noise_dropout / noise_seed: see `sample`."""
        device = self.model.device
        b = shape[0]
        rows = guidance_rows(unconditional_guidance_scale, b)
        self._check_rows(rows, quantize_denoised, self._eta, temperature, noise_dropout)
        if rows is not None and (unconditional_conditioning is None or all(v == 1.0 for v in rows)):
            rows, unconditional_guidance_scale = None, 1.0          # unguided: one forward per step (ddim.py:170-171)
        # the device array stedm_ddim_step_rows reads, made once
        scales = None if rows is None else torch.tensor(rows, dtype=torch.float32, device=device)
        if quantize_denoised and _codebook is None:
            _codebook = self._codebook(shape[1])
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float().clone()
        timesteps = self.ddim_timesteps
        total_steps = timesteps.shape[0]
        intermediates = {'x_inter': [img.clone()], 'pred_x0': [img.clone()]}
        cfg = rows is not None or not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        need_inter = lambda index: index % log_every_t == 0 or index == total_steps - 1

        blend = None if mask is None else (mask, x0, mask_seed, int(sample_id0))
        opts = self._step_opts(temperature, noise_dropout, _codebook if quantize_denoised else None, noise_seed, noises is None,
                               sample_id0)

        if self.use_graph and callback is None and img_callback is None and hasattr(self.model, "apply_model_cfg") \
                and mask_noises is None and (self._eta == 0.0 or (opts is not None and opts.draw)):
            out = self._sample_graph(img, cond, unconditional_conditioning, rows if rows is not None else unconditional_guidance_scale, cfg,
                                     total_steps, log_every_t, intermediates, blend, opts)
            ops.f16_guard_check("the DDIM sampling loop")       # fp16 modes: raise rather than return samples computed through an inf
            return out

        pred_x0 = torch.empty_like(img)
        for i, step in enumerate(np.flip(timesteps)):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:            # ddim.py:143-146
                mnz = None if mask_noises is None else mask_noises[i].to(device).float().contiguous()
                self._blend(img, mask, x0, ts, self._idx_all[index:index + 1], noise=mnz, seed=mask_seed, first_id=sample_id0)
            nz = None
            if noises is not None:
                nz = noises[i].to(device).float().contiguous()
            elif self._eta != 0.0 and not (opts is not None and opts.draw):
                nz = torch.randn(shape, device=device)     # ddim.py:206 (when sigma == 0 the draw cannot change x)
            img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning, _noise=nz, _out=(img, pred_x0),
                                              _uniform_t=True, _opts=opts, _scales=scales)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if need_inter(index):
                intermediates['x_inter'].append(img.clone())
                intermediates['pred_x0'].append(pred_x0.clone())
        ops.f16_guard_check("the DDIM sampling loop")
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, rescale_phi=0.7,
                      _noise: Optional[torch.Tensor] = None, _out=None, _uniform_t: bool = False, _opts=None, _scales=None):
        """ddim.py:164-210. Returns (x_prev, pred_x0). The step noise is `_noise` (None: no noise term); temperature, noise_dropout
        (keep bits from a seed drawn per call) and quantize_denoised as in `sample`. _opts: the loop's options (they take precedence).
        unconditional_guidance_scale: a number, or one scale per sample (a sequence or 1-D tensor of x.shape[0] values) - see `sample`.
        _scales: the loop's device tensor of per-sample scales, already checked (it takes precedence)."""
        if use_original_steps or score_corrector is not None or repeat_noise:
            raise NotImplementedError("use_original_steps / score_corrector / repeat_noise not implemented")
        scales = _scales
        rows = None if _scales is not None else guidance_rows(unconditional_guidance_scale, x.shape[0])
        if rows is not None:
            self._check_rows(rows, quantize_denoised, self._eta if _noise is not None else 0.0, temperature, noise_dropout)
            if unconditional_conditioning is None or all(v == 1.0 for v in rows):
                unconditional_guidance_scale = 1.0
            else:
                scales = torch.tensor(rows, dtype=torch.float32, device=x.device)
        if _opts is None and (quantize_denoised or temperature != 1. or noise_dropout != 0.):
            if not 0.0 <= float(noise_dropout) < 1.0:
                raise ValueError(f"noise_dropout {noise_dropout} outside [0, 1)")
            _opts = self._step_opts(temperature, noise_dropout, self._codebook(x.shape[1]) if quantize_denoised else None, None, False, 0)
        x = x.float().contiguous()
        e_u = None
        ours = hasattr(self.model, "apply_model_cfg")
        kw = {"uniform_t": True} if (ours and _uniform_t) else {}
        if scales is None and (unconditional_conditioning is None or unconditional_guidance_scale == 1.):
            e_c = self.model.apply_model(x, t, c, **kw)
        elif ours:
            e_c, e_u = self.model.apply_model_cfg(x, t, c, unconditional_conditioning, **kw)
        else:
            e_c = self.model.apply_model(x, t, c)                           # cond first, then uncond (ddim.py:177-178)
            e_u = self.model.apply_model(x, t, unconditional_conditioning)
        x_prev, pred_x0 = _out if _out is not None else (torch.empty_like(x), torch.empty_like(x))
        step = self._idx_all[index:index + 1]   # device-resident loop index (no H2D copy per step)
        self._update(x, e_c.contiguous(), None if e_u is None else e_u.contiguous(), x_prev, pred_x0, step,
                     scales if scales is not None else float(unconditional_guidance_scale), float(rescale_phi), _noise, _opts)
        return x_prev, pred_x0

    def _update(self, x, e_c, e_u, x_prev, pred_x0, step, scale, phi, noise=None, opts=None, noise_buf=None):
        """ddim.py:179-210 after the model call: stedm_ddim_step, or with options stedm_ddim_step_ex (+ stedm_ddim_quantize_x0); with
        `scale` a device tensor [B] (per-sample scales) stedm_ddim_step_rows."""
        if isinstance(scale, torch.Tensor):
            draw = opts is not None and opts.draw and self._eta != 0.0
            ops.ddim_step_rows(x, e_c, e_u, self._coefs, x_prev, scale, pred_x0=pred_x0, noise=noise if self._eta != 0.0 else None,
                               draw=draw, step_idx=step, n_iters=opts.n_iters if draw else 0, rescale_phi=phi,
                               seed=opts.seed if draw else 0, first_id=opts.first_id if draw else 0)
            return
        if opts is None:
            ops.ddim_step(x, e_c, e_u, self._coefs, x_prev, pred_x0=pred_x0, noise=noise, step_idx=step, cfg_scale=scale, rescale_phi=phi)
            return
        quant = opts.codebook is not None
        noisy = self._eta != 0.0 and (noise is not None or opts.draw)
        nbuf = None
        if quant and noisy:
            nbuf = noise_buf if noise_buf is not None else torch.empty_like(x)
        ops.ddim_step_ex(x, e_c, e_u, self._coefs, x_prev, pred_x0=pred_x0, noise=noise if self._eta != 0.0 else None,
                         draw=opts.draw and self._eta != 0.0, step_idx=step, n_iters=opts.n_iters, cfg_scale=scale, rescale_phi=phi,
                         temperature=opts.temperature, noise_dropout=opts.noise_dropout, seed=opts.seed, first_id=opts.first_id,
                         eps_out=e_c if quant else None, noise_out=nbuf)
        if quant:                                # ddim.py:202-203, then x_prev again from the quantized pred_x0 (ddim.py:205-209)
            ops.ddim_quantize_x0(pred_x0, e_c, self._coefs, opts.codebook, x_prev, noise=nbuf, step_idx=step)


    # ------------------------------------------------------------------------------------------------ graph replay
    def _sample_graph(self, img, cond, uncond, scale, cfg, total_steps, log_every_t, intermediates, blend=None, opts=None):
        """Taken for eta == 0 (sigma == 0: the noise term of ddim.py:206 is identically zero) and for eta > 0 with the noise drawn in the
        kernel from noise_seed (opts.draw)."""
        sg = StepGraph(self, img, cond, uncond if cfg else None, scale, blend=blend, opts=opts)

        def log(index):
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img.clone())
                intermediates['pred_x0'].append(sg.pred_x0.clone())

        sg.reset(total_steps - 1)
        sg.step_eager()   # packs weights and allocates every buffer before capture
        log(total_steps - 1)
        if total_steps > 1:
            with sg.stream_ctx():
                sg.capture()
                for i in range(1, total_steps):
                    sg.replay()
                    log(total_steps - i - 1)
            sg.join()
        return img, intermediates


class StepGraph:
    """One denoising step = {t fill from the device table, [masked sampling: blend of q_sample(x0, t) into `img`, noise drawn in the
    kernel from the device index], U-Net (shared-encoder CFG pass), fused DDIM/CFG update in place on `img` [with opts: stedm_ddim_step_ex,
    its noise drawn in the kernel from the device index, then stedm_ddim_quantize_x0 for quantize_x0], device index decrement},
    capturable once in a hipGraph and replayed for every step. blend: None or (mask, x0, seed, first sample id). scale: one number, or
    per-sample scales (a float32 tensor [B], a sequence): the update is then stedm_ddim_step_rows reading `scales`, a device tensor this
    object owns - set_scales() overwrites it in place, and the captured graph replays with the new values, no recapture."""

    def __init__(self, sampler: DDIMSampler, img: torch.Tensor, cond, uncond, scale: float, rescale_phi: float = 0.7, blend=None, opts=None):
        self.s = sampler
        self.img = img
        self.blend = blend
        self.opts = opts            # _StepOpts of stedm_ddim_step_ex (in-kernel noise, temperature, dropout, quantize_x0) or None
        dev = img.device
        b = img.shape[0]
        rows = guidance_rows(scale, b)
        self.scales = None if rows is None else torch.tensor(rows, dtype=torch.float32, device=dev)
        if rows is not None and opts is not None and (opts.codebook is not None or opts.temperature != 1.0 or opts.noise_dropout != 0.0):
            raise NotImplementedError("per-sample guidance scales: quantize_x0, temperature and noise_dropout are not implemented")
        self.cond, self.uncond, self.phi = cond, uncond, float(rescale_phi)
        self.scale = None if rows is not None else float(scale)
        self.cfg = uncond is not None and (rows is not None or scale != 1.0)
        self.step = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((b,), dtype=torch.int64, device=dev)
        self.pred_x0 = torch.empty_like(img)
        self.eps = torch.empty((2 * b if self.cfg else b,) + tuple(img.shape[1:]), dtype=torch.float32, device=dev)
        self.noise_buf = torch.empty_like(img) if (opts is not None and opts.codebook is not None and opts.draw) else None
        self.graph = None
        self.side = None

    def reset(self, index: int):
        self.step.fill_(int(index))

    def set_scales(self, values):
        """New per-sample guidance scales for a StepGraph built with per-sample scales: an in-place copy into the device tensor the
        captured update reads (no recapture). Every row keeps running through the CFG pass, a row set to 1 included."""
        if self.scales is None:
            raise ValueError("set_scales: this StepGraph was built with one scale for the batch (it is a launch argument of the captured "
                             "stedm_ddim_step); build it with per-sample scales")
        rows = guidance_rows(values, self.img.shape[0])
        if rows is None:
            raise ValueError(f"set_scales takes one scale per sample (a sequence or 1-D tensor), got {values!r}")
        self.scales.copy_(torch.tensor(rows, dtype=torch.float32), non_blocking=False)

    def step_eager(self):
        s, m = self.s, self.s.model
        ops.step_set_t(s._ts_table, self.step, self.t_buf)
        if self.blend is not None:
            mask, x0, seed, first_id = self.blend
            s._blend(self.img, mask, x0, self.t_buf, self.step, seed=seed, first_id=first_id)
        if self.cfg:
            e_c, e_u = m.apply_model_cfg(self.img, self.t_buf, self.cond, self.uncond, out=self.eps, uniform_t=True)
        else:
            e_c, e_u = m.apply_model(self.img, self.t_buf, self.cond, out=self.eps, uniform_t=True), None
        s._update(self.img, e_c, e_u, self.img, self.pred_x0, self.step, self.scales if self.scales is not None else self.scale, self.phi,
                  opts=self.opts, noise_buf=self.noise_buf)
        ops.step_advance(self.step, -1)

    def stream_ctx(self):
        if self.side is None:
            self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.side)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.side)

    def capture(self):
        """Must be called inside stream_ctx() after at least one step_eager()."""
        g = ops.Graph()
        with g:
            self.step_eager()
        self.graph = g

    def replay(self):
        self.graph.launch()
