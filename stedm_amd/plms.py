"""PLMS sampler (pseudo linear multistep), HIP-backed.

Mirrors `ldm.models.diffusion.plms.PLMSSampler` (reference plms.py:11-239): same constructor, `make_schedule` and `sample` surface,
returns (x, intermediates). The schedule is DDIM's with eta = 0 (plms.py:24-55 is ddim.py:24-53 line for line, and refuses eta != 0), so
the tables are `make_ddim_tables(acp, S, 0)` and the uniform stride's quirk holds (S = 128 gives 143 iterations). Iteration i (table
row index = n - 1 - i) evaluates the model at t = timesteps[index]; iteration 0 is a pseudo improved Euler step that evaluates it a
second time at (x_prev, t_next), the later ones are Adams-Bashforth steps of order min(i, 3) over the CFG-combined eps of the previous
iterations. n iterations cost n + 1 model evaluations. Every tensor operation of the loop runs in HIP kernels:
  * the model calls -> one shared-encoder CFG pass (`apply_model_cfg`) when the model offers it, else two `apply_model` calls (cond,
    then uncond). CFG is the plain e_u + s (e_c - e_u) of plms.py:178-192: DDIM's std rescale (ddim.py) does not apply here. The
    reference forms the CFG batch with torch.cat([unconditional_conditioning, c]), which fails on STEDM's dict conditioning; the
    arithmetic it intends (one batched call per sample, then chunk(2)) is what the shared-encoder pass computes;
  * CFG combine, the multistep combination, the eps history and the DDIM update -> one fused kernel per update (stedm_plms_step) over a
    device ring of the last four eps; the history slot and the order come from the device step index, so no host branch remains;
  * masked sampling (plms.py:147-150) -> DDIMSampler's blend kernel (stedm_ddim_mask_blend) with its checks, before the first model call
    of each iteration; its in-kernel noise is keyed by the same table index as DDIM's, so equal mask_seed and S draw equal noise;
  * with `use_graph=True` iteration 0 runs eagerly (it also packs the weights and allocates every buffer) and one later iteration
    {t from the table, [blend], CFG pass into a preallocated eps, stedm_plms_step, index - 1} is captured once in a hipGraph and replayed
    for the remaining n - 1 iterations.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .ddim import DDIMSampler, refuse_guidance_rows


class PLMSSampler(object):
    # DDIM's device placement, masked-sampling checks and blend, unchanged (the reference's masked loop is the same in both files)
    register_buffer = DDIMSampler.register_buffer
    _mask_args = DDIMSampler._mask_args
    _blend = DDIMSampler._blend

    def __init__(self, model, schedule="linear", **kwargs):
        """plms.py:12-16. use_graph=True: hipGraph replay of the iterations after the first (PLMSStepGraph)."""
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.use_graph = bool(kwargs.get("use_graph", False))

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        """plms.py:24-55: DDIM's tables (DDIMSampler.make_schedule); eta != 0 raises ValueError as in the reference."""
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        DDIMSampler.make_schedule(self, ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0., verbose=verbose)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        """plms.py:58-112 -> (x, intermediates). eta != 0 raises ValueError (as the reference); quantize_x0, score_corrector,
        noise_dropout and temperature != 1 raise NotImplementedError, as do per-step `noises` (PLMS draws nothing after x_T) — all before
        any device work. mask / x0 and the keywords mask_noises / mask_seed / sample_id0: as DDIMSampler.sample. callback(i) and
        img_callback(pred_x0, i) run after iteration i (eager loop). One unconditional_guidance_scale for the batch: per-sample scales
        (a sequence or 1-D tensor) raise NotImplementedError - DDIMSampler has them."""
        refuse_guidance_rows(unconditional_guidance_scale, "PLMSSampler")
        if eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        if quantize_x0 or score_corrector is not None or noise_dropout > 0. or temperature != 1. or kwargs.get("noises") is not None:
            raise NotImplementedError("PLMS sampling: quantize_x0 / score_corrector / noise_dropout / temperature / noises are not "
                                      "implemented (unused by the reference drivers)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        masking = {}
        if mask is not None:
            masking = self._mask_args(size, mask, x0, kwargs.get("mask_noises"), kwargs.get("mask_seed"), kwargs.get("sample_id0", 0))
        return self.plms_sampling(conditioning, size, x_T=x_T, callback=callback, img_callback=img_callback, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, **masking)

    def _eps(self, x, t, cond, uncond, out=None):
        """(e_c, e_u or None) at timesteps t (int64 [B], equal rows): get_model_output's model calls (plms.py:178-186)."""
        m = self.model
        if hasattr(m, "apply_model_cfg"):
            if uncond is None:
                return m.apply_model(x, t, cond, out=out, uniform_t=True), None
            return m.apply_model_cfg(x, t, cond, uncond, out=out, uniform_t=True)
        e_c = m.apply_model(x, t, cond)
        return e_c, (None if uncond is None else m.apply_model(x, t, uncond))

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, log_every_t=100, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, mask=None, x0=None, mask_noises=None, mask_seed=None, sample_id0=0):
        """plms.py:114-170 (ddim_use_original_steps=False, timesteps=None). x_inter logs the unblended img as the reference does."""
        refuse_guidance_rows(unconditional_guidance_scale, "PLMSSampler")
        device = self.model.device
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float().clone()
        total_steps = self.ddim_timesteps.shape[0]
        intermediates = {'x_inter': [img.clone()], 'pred_x0': [img.clone()]}
        cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        uncond = unconditional_conditioning if cfg else None
        scale = float(unconditional_guidance_scale)
        blend = None if mask is None else (mask, x0, mask_seed, int(sample_id0))

        def log(index, pred_x0):
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img.clone())
                intermediates['pred_x0'].append(pred_x0.clone())

        if self.use_graph and callback is None and img_callback is None and hasattr(self.model, "apply_model_cfg") and mask_noises is None:
            sg = PLMSStepGraph(self, img, cond, uncond, scale, blend=blend)
            sg.reset(total_steps - 1)
            sg.first_step()
            log(total_steps - 1, sg.pred_x0)
            if total_steps > 1:
                with sg.stream_ctx():
                    sg.capture()
                    for i in range(1, total_steps):
                        sg.replay()
                        log(total_steps - i - 1, sg.pred_x0)
                sg.join()
        else:
            self._sample_eager(img, cond, uncond, scale, blend, mask_noises, callback, img_callback, log)
        ops.f16_guard_check("the PLMS sampling loop")        # fp16 modes: raise rather than return samples computed through an inf
        return img, intermediates

    def _sample_eager(self, img, cond, uncond, scale, blend, mask_noises, callback, img_callback, log):
        dev = img.device
        b = img.shape[0]
        ts = self.ddim_timesteps
        n = ts.shape[0]
        ring = torch.empty((4,) + tuple(img.shape), dtype=torch.float32, device=dev)
        x_tmp = torch.empty_like(img)
        pred_x0 = torch.empty_like(img)
        f = lambda e: None if e is None else e.float().contiguous()
        for i in range(n):
            index = n - 1 - i
            step = self._idx_all[index:index + 1]
            t = torch.full((b,), int(ts[index]), device=dev, dtype=torch.long)
            if blend is not None:                   # plms.py:147-150
                mask, x0, seed, first_id = blend
                mnz = None if mask_noises is None else mask_noises[i].to(dev).float().contiguous()
                self._blend(img, mask, x0, t, step, noise=mnz, seed=seed, first_id=first_id)
            e_c, e_u = self._eps(img, t, cond, uncond)
            if i == 0:                              # pseudo improved Euler (plms.py:219-223); t_next = time_range[min(1, n - 1)]
                ops.plms_step(img, f(e_c), f(e_u), ring, self._coefs, step, n, ops.PLMS_EULER, scale, x_tmp=x_tmp)
                t_next = torch.full((b,), int(ts[max(index - 1, 0)]), device=dev, dtype=torch.long)
                e_c, e_u = self._eps(x_tmp, t_next, cond, uncond)
                ops.plms_step(img, f(e_c), f(e_u), ring, self._coefs, step, n, ops.PLMS_HEUN, scale, pred_x0=pred_x0)
            else:
                ops.plms_step(img, f(e_c), f(e_u), ring, self._coefs, step, n, ops.PLMS_MULTISTEP, scale, pred_x0=pred_x0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            log(index, pred_x0)


class PLMSStepGraph:
    """The PLMS loop on device state: a step counter (the table index), the eps ring, x_tmp, pred_x0 and a preallocated eps. Iteration 0
    (`first_step`, eager) = {t from the table, [blend], CFG pass, stedm_plms_step EULER, t_next, CFG pass at x_tmp, HEUN, index - 1};
    every later iteration (`step`) = {t from the table, [blend], CFG pass, stedm_plms_step MULTISTEP, index - 1}, capturable once in a
    hipGraph and replayed (the pattern of ddim.StepGraph). blend: None or (mask, x0, seed, first sample id)."""

    def __init__(self, sampler: PLMSSampler, img: torch.Tensor, cond, uncond, scale: float, blend=None):
        self.s = sampler
        self.img = img
        self.cond, self.uncond, self.scale = cond, uncond, float(scale)
        self.blend = blend
        dev = img.device
        b = img.shape[0]
        self.n = int(sampler.ddim_timesteps.shape[0])
        self.step_idx = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((b,), dtype=torch.int64, device=dev)
        self.ring = torch.empty((4,) + tuple(img.shape), dtype=torch.float32, device=dev)
        self.x_tmp = torch.empty_like(img)
        self.pred_x0 = torch.empty_like(img)
        self.eps = torch.empty((2 * b if uncond is not None else b,) + tuple(img.shape[1:]), dtype=torch.float32, device=dev)
        self.graph = None
        self.side = None

    def reset(self, index: int):
        self.step_idx.fill_(int(index))

    def _eval(self, x):
        m = self.s.model
        if self.uncond is not None:
            return m.apply_model_cfg(x, self.t_buf, self.cond, self.uncond, out=self.eps, uniform_t=True)
        return m.apply_model(x, self.t_buf, self.cond, out=self.eps, uniform_t=True), None

    def _set_t_and_blend(self):
        s = self.s
        ops.step_set_t(s._ts_table, self.step_idx, self.t_buf)
        if self.blend is not None:
            mask, x0, seed, first_id = self.blend
            s._blend(self.img, mask, x0, self.t_buf, self.step_idx, seed=seed, first_id=first_id)

    def first_step(self):
        """Iteration 0; the counter must hold n - 1."""
        s, n = self.s, self.n
        self._set_t_and_blend()
        e_c, e_u = self._eval(self.img)
        ops.plms_step(self.img, e_c, e_u, self.ring, s._coefs, self.step_idx, n, ops.PLMS_EULER, self.scale, x_tmp=self.x_tmp)
        j = max(n - 2, 0)
        ops.step_set_t(s._ts_table, s._idx_all[j:j + 1], self.t_buf)
        e_c, e_u = self._eval(self.x_tmp)
        ops.plms_step(self.img, e_c, e_u, self.ring, s._coefs, self.step_idx, n, ops.PLMS_HEUN, self.scale, pred_x0=self.pred_x0)
        ops.step_advance(self.step_idx, -1)

    def step(self):
        """One iteration i >= 1 (i = n - 1 - counter)."""
        s = self.s
        self._set_t_and_blend()
        e_c, e_u = self._eval(self.img)
        ops.plms_step(self.img, e_c, e_u, self.ring, s._coefs, self.step_idx, self.n, ops.PLMS_MULTISTEP, self.scale, pred_x0=self.pred_x0)
        ops.step_advance(self.step_idx, -1)

    def stream_ctx(self):
        if self.side is None:
            self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.side)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.side)

    def capture(self):
        """Must be called inside stream_ctx() after first_step()."""
        g = ops.Graph()
        with g:
            self.step()
        self.graph = g

    def replay(self):
        self.graph.launch()
