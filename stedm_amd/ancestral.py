"""Ancestral DDPM sampling (the reference's `sample_log(ddim=False)`), HIP-backed.

Mirrors `LatentDiffusion.sample` / `p_sample_loop` / `p_sample` / `p_mean_variance` (reference ddpm.py:1050-1250): the whole chain
t = timesteps - 1 ... 0 of the model's schedule, one model evaluation per step, returns (x, intermediates) with intermediates a list
(x_T, then x after every step i with i % log_every_t == 0 or i == timesteps - 1). Every tensor operation of the loop runs in HIP kernels:
  * the model call -> `apply_model(x, t, cond, out=eps, uniform_t=True)` (no guidance: the reference's ancestral path has none);
  * predict_start_from_noise, the clamp (clip_denoised), q_posterior's mean, the posterior noise sigma_t z and, with a mask, the blend
    with q_sample(x0, t) after the step (ddpm.py:1207-1209) -> one fused kernel (stedm_ddpm_step) from a device table [T][5]
    {sr, srm1, c1, c2, sigma} (schedule.ddpm_step_table); its noise is drawn in the kernel from (noise_seed, global sample id) on stream
    0x10000 + t, the blend's from (mask_seed, global sample id) on stream 0x8000 + t, so a sample does not depend on the shard;
  * with `use_graph=True` the first step runs eagerly (it also packs the weights and allocates every buffer) and one step {t from the
    device counter, model call into a preallocated eps, stedm_ddpm_step, counter - 1} is captured once in a hipGraph and replayed for the
    remaining timesteps - 1 steps (the pattern of ddim.StepGraph).
"""
from __future__ import annotations

import torch

from . import ops
from .ddim import DDIMSampler
from .schedule import ddpm_step_table


def _slice_cond(cond, batch_size):
    """ddpm.py:1225-1229: cond[:batch_size], also inside dicts of lists."""
    if cond is None:
        return None
    if isinstance(cond, dict):
        return {key: cond[key][:batch_size] if not isinstance(cond[key], list) else list(map(lambda x: x[:batch_size], cond[key]))
                for key in cond}
    return [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]


def step_table(model) -> torch.Tensor:
    """The device table [T][5] of stedm_ddpm_step from the model's fp32 buffers (built on the CPU: schedule.ddpm_step_table)."""
    tab = ddpm_step_table(*(getattr(model, n).detach().cpu() for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                                       "posterior_mean_coef1", "posterior_mean_coef2",
                                                                       "posterior_log_variance_clipped")))
    return torch.from_numpy(tab).to(model.device)


class AncestralSampler(object):
    """The ancestral loop over a model with the reference's DDPM surface: num_timesteps, clip_denoised, log_every_t, device, the fp32
    buffers sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1 / 2, posterior_log_variance_clipped,
    sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, and apply_model(x, t, cond)."""

    def __init__(self, model, use_graph=False):
        self.model = model
        self.use_graph = bool(use_graph)

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None, quantize_denoised=False,
               mask=None, x0=None, shape=None, **kwargs):
        """ddpm.py:1219-1235. Forwards x_T, timesteps, quantize_denoised, mask, x0 and shape to p_sample_loop, and the repo's keywords
        noises / noise_seed / sample_id0 / mask_noises / mask_seed (see p_sample_loop). Like the reference it ignores every other keyword
        - log_every_t (the loop logs by the model's log_every_t), verbose, ddim_steps, callbacks - except the options whose effect the
        reference silently drops, which raise NotImplementedError before any device work: eta != 0, temperature != 1,
        noise_dropout > 0, score_corrector, quantize_denoised=True, and unconditional_guidance_scale != 1 with
        unconditional_conditioning (the reference's ancestral chain has no guidance)."""
        scale = kwargs.get("unconditional_guidance_scale", 1.)
        if kwargs.get("unconditional_conditioning") is not None and scale != 1.:
            raise NotImplementedError("ancestral sampling has no classifier-free guidance in the reference (sample() drops "
                                      "unconditional_guidance_scale / unconditional_conditioning); use a DDIM / PLMS / DPM-Solver sampler")
        if kwargs.get("eta", 0.) != 0. or kwargs.get("temperature", 1.) != 1. or kwargs.get("noise_dropout", 0.) > 0. \
                or kwargs.get("score_corrector") is not None:
            raise NotImplementedError("ancestral sampling: eta / temperature / noise_dropout / score_corrector are dropped by the "
                                      "reference's sample(); refused rather than ignored")
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs the first stage's quantizer (taming); not built")
        if shape is None:
            shape = (batch_size, self.model.channels, self.model.image_size, self.model.image_size)
        cond = _slice_cond(cond, batch_size)
        extra = {k: kwargs[k] for k in ("noises", "noise_seed", "sample_id0", "mask_noises", "mask_seed") if k in kwargs}
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose, timesteps=timesteps,
                                  quantize_denoised=quantize_denoised, mask=mask, x0=x0, **extra)

    def _checks(self, shape, T, x_T, noises, mask, x0, mask_noises, mask_seed, sample_id0):
        size = tuple(int(s) for s in shape)
        if len(size) != 4:
            raise ValueError(f"shape must be (B, C, H, W), got {tuple(shape)}")
        if x_T is not None and tuple(x_T.shape) != size:
            raise ValueError(f"x_T {tuple(x_T.shape)} must have the shape {size}")
        if noises is not None:
            noises = list(noises)
            if len(noises) != T or any(tuple(n.shape) != size for n in noises):
                raise ValueError(f"noises must hold {T} tensors of shape {size}, one per step")
        masking = None
        if mask is not None:
            if mask_noises is not None:
                mask_noises = list(mask_noises)
                if len(mask_noises) != T or any(tuple(n.shape) != size for n in mask_noises):
                    raise ValueError(f"mask_noises must hold {T} tensors of shape {size}, one per step")
            masking = DDIMSampler._mask_args(self, size, mask, x0, None, 0 if mask_noises is not None else mask_seed, sample_id0)
            masking["mask_noises"] = mask_noises
        elif mask_noises is not None:
            raise ValueError("mask_noises given without a mask")
        return size, noises, masking

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None,
                      noises=None, noise_seed=None, sample_id0=0, mask_noises=None, mask_seed=None):
        """ddpm.py:1169-1217 -> img, or (img, intermediates). The blend with q_sample(x0, ts) runs after each step at the same ts, the
        t = 0 step included. Repo-specific keywords: `noises` (one N(0,1) tensor per step, step k at t = timesteps - 1 - k, in place of
        noise_like's draw; eager loop); else the step noise is drawn in the kernel from `noise_seed` (default: one draw from torch's CPU
        generator per call) and the global sample id `sample_id0 + b`. mask / x0 / mask_noises / mask_seed: as DDIMSampler.sample, one
        mask noise per step. callback(i) / img_callback(img, i) after the step at t = i (eager loop). verbose is ignored (no progress
        bar)."""
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised needs the first stage's quantizer (taming); not built")
        m = self.model
        if not log_every_t:
            log_every_t = m.log_every_t
        T = m.num_timesteps if timesteps is None else int(timesteps)
        if start_T is not None:
            T = min(T, int(start_T))
        if not 1 <= T <= m.num_timesteps:
            raise ValueError(f"timesteps {T} outside [1, {m.num_timesteps}]")
        size, noises, masking = self._checks(shape, T, x_T, noises, mask, x0, mask_noises, mask_seed, sample_id0)
        if noises is None and noise_seed is None:
            noise_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        dev = m.device
        b = size[0]
        img = torch.randn(size, device=dev) if x_T is None else x_T.to(dev).float().clone()
        intermediates = [img.clone()]
        st = AncestralStepGraph(m, img, cond, step_table(m), bool(m.clip_denoised), 0 if noise_seed is None else int(noise_seed),
                                int(sample_id0), masking)

        def log(i):
            if i % log_every_t == 0 or i == T - 1:
                intermediates.append(img.clone())

        if self.use_graph and callback is None and img_callback is None and noises is None and hasattr(m, "apply_model_cfg") \
                and (masking is None or masking["mask_noises"] is None):
            st.step_idx.fill_(T - 1)
            st.step()                   # packs the weights and allocates every buffer before the capture
            log(T - 1)
            if T > 1:
                with st.stream_ctx():
                    st.capture()
                    for i in range(T - 2, -1, -1):
                        st.replay()
                        log(i)
                st.join()
        else:
            idx = torch.arange(T, dtype=torch.int32, device=dev)
            for k, i in enumerate(range(T - 1, -1, -1)):
                t = torch.full((b,), i, device=dev, dtype=torch.long)
                nz = None if noises is None else noises[k].to(dev).float().contiguous()
                mnz = None
                if masking is not None and masking["mask_noises"] is not None:
                    mnz = masking["mask_noises"][k].to(dev).float().contiguous()
                st.update(st.eval(img, t), idx[i:i + 1], noise=nz, mask_noise=mnz)
                log(i)
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(img, i)
        ops.f16_guard_check("the ancestral sampling loop")      # fp16 modes: raise rather than return samples computed through an inf
        if return_intermediates:
            return img, intermediates
        return img


class AncestralStepGraph:
    """The loop's device state: the step table, the step counter (= t), the t buffer, a preallocated eps; `step` = {t from the counter,
    model call, stedm_ddpm_step, counter - 1}, capturable once in a hipGraph and replayed (the pattern of ddim.StepGraph)."""

    def __init__(self, model, img, cond, table, clip, seed, first_id, masking):
        self.m, self.img, self.cond, self.table, self.clip = model, img, cond, table, clip
        self.seed, self.first_id, self.masking = seed, first_id, masking
        dev = img.device
        self.step_idx = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((img.shape[0],), dtype=torch.int64, device=dev)
        self.ts_table = torch.arange(model.num_timesteps, dtype=torch.int64, device=dev)
        self.eps = torch.empty_like(img)
        self.graph = None
        self.side = None

    def eval(self, x, t):
        m = self.m
        if hasattr(m, "apply_model_cfg"):
            return m.apply_model(x, t, self.cond, out=self.eps, uniform_t=True)
        return m.apply_model(x, t, self.cond).float().contiguous()

    def update(self, eps, step_idx, noise=None, mask_noise=None):
        mk = self.masking
        if mk is None:
            ops.ddpm_step(self.img, eps, self.table, step_idx, self.clip, noise=noise, seed=self.seed, first_id=self.first_id)
        else:
            m = self.m
            ops.ddpm_step(self.img, eps, self.table, step_idx, self.clip, noise=noise, seed=self.seed, first_id=self.first_id,
                          mask=mk["mask"], x0=mk["x0"], mask_noise=mask_noise, mask_seed=mk["mask_seed"] or 0,
                          sqrt_ac=m.sqrt_alphas_cumprod, sqrt_1mac=m.sqrt_one_minus_alphas_cumprod)

    def step(self):
        ops.step_set_t(self.ts_table, self.step_idx, self.t_buf)
        self.update(self.eval(self.img, self.t_buf), self.step_idx)
        ops.step_advance(self.step_idx, -1)

    def stream_ctx(self):
        if self.side is None:
            self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.side)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.side)

    def capture(self):
        """Must be called inside stream_ctx() after one eager step()."""
        g = ops.Graph()
        with g:
            self.step()
        self.graph = g

    def replay(self):
        self.graph.launch()
