"""Ancestral DDPM sampling (the reference's `sample_log(ddim=False)`), HIP-backed.

Mirrors `LatentDiffusion.sample` / `p_sample_loop` / `p_sample` / `p_mean_variance` (reference ddpm.py:1050-1250): the whole chain
t = timesteps - 1 ... 0 of the model's schedule, one model evaluation per step, returns (x, intermediates) with intermediates a list
(x_T, then x after every step i with i % log_every_t == 0 or i == timesteps - 1). Every tensor operation of the loop runs in HIP kernels:
  * the model call -> `apply_model(x, t, cond, out=eps, uniform_t=True)` (no guidance: the reference's ancestral path has none);
  * predict_start_from_noise, the clamp (clip_denoised), q_posterior's mean, the posterior noise sigma_t z and, with a mask, the blend
    with q_sample(x0, t) after the step (ddpm.py:1207-1209) -> one fused kernel (stedm_ddpm_step_ex) from a device table [T][5]
    {sr, srm1, c1, c2, sigma} (schedule.ddpm_step_table); its noise is drawn in the kernel from (noise_seed, global sample id) on stream
    0x10000 + t, the blend's from (mask_seed, global sample id) on stream 0x8000 + t, so a sample does not depend on the shard;
  * with `use_graph=True` the first step runs eagerly (it also packs the weights and allocates every buffer) and one step {t from the
    device counter, model call into a preallocated eps, stedm_ddpm_step_ex, counter - 1} is captured once in a hipGraph and replayed for the
    remaining timesteps - 1 steps (the pattern of ddim.StepGraph);
  * quantize_denoised (ddpm.py:1071-1072), and `progressive_denoising` (ddpm.py:1112-1166) with its temperature (a number or a
    per-timestep list), noise_dropout and x0-prediction log, and the single steps `p_sample` / `p_mean_variance` (:1050-1110) at a
    per-sample t -> the same kernel's options (the temperature as a device table indexed by t, the keep bits of the dropout drawn in the
    kernel from (noise_seed, global sample id, t)), eager and graphed alike.
"""
from __future__ import annotations

import numbers

import torch

from . import ops
from .ddim import DDIMSampler, first_stage_codebook, refuse_guidance_rows
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
    """The device table [T][5] of stedm_ddpm_step_ex from the model's fp32 buffers (built on the CPU: schedule.ddpm_step_table)."""
    tab = ddpm_step_table(*(getattr(model, n).detach().cpu() for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                                       "posterior_mean_coef1", "posterior_mean_coef2",
                                                                       "posterior_log_variance_clipped")))
    return torch.from_numpy(tab).to(model.device)


class _ExOpts:
    """The options of stedm_ddpm_step_ex a run sets: the temperature table (device fp32 [T] indexed by t, or None for 1), the
    noise dropout and the codebook of quantize_denoised (or None)."""

    def __init__(self, temperature, noise_dropout, codebook):
        self.temperature, self.noise_dropout, self.codebook = temperature, float(noise_dropout), codebook


def _check_dropout(noise_dropout):
    if not 0.0 <= float(noise_dropout) < 1.0:
        raise ValueError(f"noise_dropout {noise_dropout} outside [0, 1)")
    return float(noise_dropout)


def _draw_seed():
    """The repo's default seed: one draw from torch's CPU generator per call."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


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
        noise_dropout > 0, score_corrector, and unconditional_guidance_scale != 1 with unconditional_conditioning (the reference's
        ancestral chain has no guidance; temperature and noise_dropout are progressive_denoising's). quantize_denoised needs a VQ first
        stage (p_sample_loop)."""
        scale = kwargs.get("unconditional_guidance_scale", 1.)
        refuse_guidance_rows(scale, "the ancestral sampler")
        if kwargs.get("unconditional_conditioning") is not None and scale != 1.:
            raise NotImplementedError("ancestral sampling has no classifier-free guidance in the reference (sample() drops "
                                      "unconditional_guidance_scale / unconditional_conditioning); use a DDIM / PLMS / DPM-Solver sampler")
        if kwargs.get("eta", 0.) != 0. or kwargs.get("temperature", 1.) != 1. or kwargs.get("noise_dropout", 0.) > 0. \
                or kwargs.get("score_corrector") is not None:
            raise NotImplementedError("ancestral sampling: eta / temperature / noise_dropout / score_corrector are dropped by the "
                                      "reference's sample(); refused rather than ignored")
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

    def _codebook(self, shape):
        """first_stage_codebook for quantize_denoised at the latents' shape (B, C, H, W); raises before any device work."""
        size = tuple(shape)
        if len(size) != 4:
            raise ValueError(f"shape must be (B, C, H, W), got {size}")
        return first_stage_codebook(self.model, size[1], "quantize_denoised")

    def _temperature_table(self, temperature, T):
        """progressive_denoising's temperature (ddpm.py:1142-1143, 1155) as host floats indexed by t over the whole schedule: a number
        (the reference takes floats only; any real number is accepted here) fills [0, T); a list is indexed by t and must hold at least T
        entries. Timesteps the run does not visit keep 1. None: every entry is 1 (no table needed)."""
        if isinstance(temperature, numbers.Real):
            vals = [float(temperature)] * T
        else:
            vals = [float(v) for v in temperature]
            if len(vals) < T:
                raise ValueError(f"temperature holds {len(vals)} entries, the run indexes it by t up to {T - 1}")
            vals = vals[:T]
        if all(v == 1.0 for v in vals):
            return None
        return vals + [1.0] * (self.model.num_timesteps - T)

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None,
                      noises=None, noise_seed=None, sample_id0=0, mask_noises=None, mask_seed=None):
        """ddpm.py:1169-1217 -> img, or (img, intermediates). The blend with q_sample(x0, ts) runs after each step at the same ts, the
        t = 0 step included. quantize_denoised: the predicted x0 of every step is snapped to the first stage's codebook (needs
        first_stage_model.quantize.embedding of the latents' width). Repo-specific keywords: `noises` (one N(0,1) tensor per step, step k
        at t = timesteps - 1 - k, in place of noise_like's draw; eager loop); else the step noise is drawn in the kernel from `noise_seed`
        (default: one draw from torch's CPU generator per call) and the global sample id `sample_id0 + b`. mask / x0 / mask_noises /
        mask_seed: as DDIMSampler.sample, one mask noise per step. callback(i) / img_callback(img, i) after the step at t = i (eager
        loop). verbose is ignored (no progress bar)."""
        codebook = self._codebook(shape) if quantize_denoised else None
        m = self.model
        if not log_every_t:
            log_every_t = m.log_every_t
        T = m.num_timesteps if timesteps is None else int(timesteps)
        if start_T is not None:
            T = min(T, int(start_T))
        if not 1 <= T <= m.num_timesteps:
            raise ValueError(f"timesteps {T} outside [1, {m.num_timesteps}]")
        opts = None if codebook is None else _ExOpts(None, 0.0, codebook)
        img, intermediates = self._loop(cond, shape, T, x_T, log_every_t, noises, noise_seed, sample_id0, mask, x0, mask_noises, mask_seed,
                                        callback, img_callback, opts, log_x0=False)
        if return_intermediates:
            return img, intermediates
        return img

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False, img_callback=None, mask=None,
                              x0=None, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, batch_size=None,
                              x_T=None, start_T=None, log_every_t=None, noises=None, noise_seed=None, sample_id0=0, mask_noises=None,
                              mask_seed=None):
        """ddpm.py:1112-1166 -> (img, intermediates). With batch_size, shape is (C, H, W); without, (B, C, H, W). The chain runs
        t = timesteps - 1 ... 0 with timesteps = min(num_timesteps, start_T); every step is p_sample(clip_denoised=model.clip_denoised,
        quantize_denoised, temperature[t], noise_dropout), then the mask blend (t = 0 included). intermediates is the list of the
        PREDICTED x0 (after clamp and quantisation) of the steps with t % log_every_t == 0 or t == timesteps - 1; it does not hold x_T
        (not p_sample_loop's list). temperature: a number for every step, or a list indexed by t with at least `timesteps` entries. The
        reference tests type(temperature) == float, so an int fails there with "'int' object is not subscriptable"; any real number is
        accepted here. noise_dropout p in [0, 1): F.dropout's rule and scale with keep bits drawn in the kernel from (noise_seed,
        sample_id0 + b, t) (include/stedm_hip.h, stedm_ddpm_step_ex; torch's stream cannot be reproduced). score_corrector, and a model
        with shorten_cond_schedule (the reference asserts non-hybrid conditioning there), raise NotImplementedError. Repo keywords, the
        graphed form's conditions, callbacks and verbose: as p_sample_loop."""
        if score_corrector is not None:
            raise NotImplementedError("score_corrector: unused by the reference drivers, not implemented")
        m = self.model
        if getattr(m, "shorten_cond_schedule", False):
            raise NotImplementedError("shorten_cond_schedule: the reference asserts non-hybrid conditioning there (ddpm.py:1147-1150); "
                                      "STEDM's conditioning is hybrid")
        noise_dropout = _check_dropout(noise_dropout)
        if not log_every_t:
            log_every_t = m.log_every_t
        T = m.num_timesteps
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        if start_T is not None:
            T = min(T, int(start_T))
        if T < 1:
            raise ValueError(f"start_T {start_T} leaves no step to run")
        temps = self._temperature_table(temperature, T)
        codebook = self._codebook(shape) if quantize_denoised else None
        cond = _slice_cond(cond, batch_size)
        opts = _ExOpts(temps, noise_dropout, codebook)
        return self._loop(cond, shape, T, x_T, log_every_t, noises, noise_seed, sample_id0, mask, x0, mask_noises, mask_seed, callback,
                          img_callback, opts, log_x0=True)

    def _loop(self, cond, shape, T, x_T, log_every_t, noises, noise_seed, sample_id0, mask, x0, mask_noises, mask_seed, callback,
              img_callback, opts, log_x0):
        """The chain t = T - 1 ... 0 shared by p_sample_loop (logs x_T, then img) and progressive_denoising (log_x0: logs the predicted
        x0). opts: _ExOpts with the temperature still as host floats, or None for the plain step."""
        m = self.model
        size, noises, masking = self._checks(shape, T, x_T, noises, mask, x0, mask_noises, mask_seed, sample_id0)
        if noise_seed is None and (noises is None or (opts is not None and opts.noise_dropout > 0.0)):
            noise_seed = _draw_seed()
        dev = m.device
        b = size[0]
        img = torch.randn(size, device=dev) if x_T is None else x_T.to(dev).float().clone()
        if opts is not None and opts.temperature is not None:
            opts.temperature = torch.tensor(opts.temperature, dtype=torch.float32).to(dev)
        st = AncestralStepGraph(m, img, cond, step_table(m), bool(m.clip_denoised), 0 if noise_seed is None else int(noise_seed),
                                int(sample_id0), masking, opts=opts)
        intermediates = [] if log_x0 else [img.clone()]

        def log(i):
            if i % log_every_t == 0 or i == T - 1:
                intermediates.append((st.x0_pred if log_x0 else img).clone())

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
        return img, intermediates

    # ------------------------------------------------------------------------------------------------ single steps
    def _single_step_refusals(self, repeat_noise, return_codebook_ids, score_corrector):
        if repeat_noise:
            raise NotImplementedError("repeat_noise: one draw shared by the batch contradicts per-sample noise streams; not implemented")
        if return_codebook_ids:
            raise NotImplementedError("return_codebook_ids: the reference dropped its support (ddpm.py:1091-1092)")
        if score_corrector is not None:
            raise NotImplementedError("score_corrector: unused by the reference drivers, not implemented")

    def _step_inputs(self, x, c, t, quantize_denoised):
        """Argument checks, then the device work every single step needs: x and t on the device, the model call, the step table."""
        if x.dim() != 4:
            raise ValueError(f"x must be [B, C, H, W], got {tuple(x.shape)}")
        if t.dim() != 1 or t.shape[0] != x.shape[0] or t.is_floating_point():
            raise ValueError(f"t must be an integer tensor [B] = [{x.shape[0]}], got {t.dtype} {tuple(t.shape)}")
        codebook = self._codebook(x.shape) if quantize_denoised else None
        m = self.model
        dev = m.device
        x = x.to(dev).float().contiguous()
        t = t.to(dev).to(torch.int64).contiguous()
        eps = m.apply_model(x, t, c).float().contiguous()
        return x, t, eps, cached_step_table(m), codebook

    @torch.no_grad()
    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False, return_x0=False,
                        score_corrector=None, corrector_kwargs=None):
        """ddpm.py:1050-1079 -> (model_mean, posterior_variance, posterior_log_variance[, x_recon]) at the per-sample timesteps t (int64
        [B]); the two variances are the [B, 1, 1, 1] gathers of the reference's extract_into_tensor. One kernel (stedm_ddpm_step_ex
        without the sample) computes the mean and x_recon; x is left alone."""
        self._single_step_refusals(False, return_codebook_ids, score_corrector)
        x, t, eps, table, codebook = self._step_inputs(x, c, t, quantize_denoised)
        m = self.model
        mean = torch.empty_like(x)
        x_recon = torch.empty_like(x) if (return_x0 or codebook is not None) else None
        ops.ddpm_step_ex(x, eps, table, t=t, clip_denoised=bool(clip_denoised), codebook=codebook, x0_out=x_recon, mean_out=mean)
        ext = lambda a: a.to(x.device)[t].reshape(x.shape[0], 1, 1, 1)
        out = (mean, ext(m.posterior_variance), ext(m.posterior_log_variance_clipped))
        return out + (x_recon,) if return_x0 else out

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_codebook_ids=False, quantize_denoised=False,
                 return_x0=False, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, _noise=None,
                 noise_seed=None, sample_id0=0):
        """ddpm.py:1081-1110 -> x_prev, or (x_prev, x0) with return_x0, at the per-sample timesteps t (int64 [B]); x is left alone. The
        noise is `_noise` when given; otherwise it is drawn in the kernel from `noise_seed` (default: one draw from torch's CPU generator
        per call) and the global sample id sample_id0 + b on stream 0x10000 + t[b], as the loops draw it. noise_dropout's keep bits come
        from the same seed. repeat_noise, return_codebook_ids and score_corrector raise NotImplementedError."""
        self._single_step_refusals(repeat_noise, return_codebook_ids, score_corrector)
        noise_dropout = _check_dropout(noise_dropout)
        if _noise is not None and tuple(_noise.shape) != tuple(x.shape):
            raise ValueError(f"_noise {tuple(_noise.shape)} must have x's shape {tuple(x.shape)}")
        x, t, eps, table, codebook = self._step_inputs(x, c, t, quantize_denoised)
        if noise_seed is None and (_noise is None or noise_dropout > 0.0):
            noise_seed = _draw_seed()
        temps = None if float(temperature) == 1.0 else torch.full((table.shape[0],), float(temperature), dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        x_recon = torch.empty_like(x) if (return_x0 or codebook is not None) else None
        ops.ddpm_step_ex(x, eps, table, t=t, clip_denoised=bool(clip_denoised), noise=None if _noise is None else
                         _noise.to(x.device).float().contiguous(), temperature=temps, noise_dropout=noise_dropout, codebook=codebook,
                         seed=0 if noise_seed is None else int(noise_seed), first_id=int(sample_id0), x_out=out, x0_out=x_recon)
        return (out, x_recon) if return_x0 else out

    def _affine(self, name, a, b, t, c1, c2):
        """c1[t] a + c2[t] b per sample through the step kernel: with the table row {0, -1, c1, c2, 0} and `a` in the eps slot the
        predicted x0 is 0 b - (-1) a = a exactly, and the posterior mean c1 a + c2 b (c2 None: 0)."""
        m = self.model
        dev = m.device
        a = a.to(dev).float().contiguous()
        b = a if b is None else b.to(dev).float().contiguous()
        if a.dim() != 4 or a.shape != b.shape:
            raise ValueError(f"{name}: the operands must be [B, C, H, W] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        t = t.to(dev).to(torch.int64).contiguous()
        c1 = c1.detach().to(dev).float()
        tab = torch.zeros((c1.shape[0], 5), dtype=torch.float32, device=dev)
        tab[:, 1] = -1.0
        tab[:, 2] = c1
        if c2 is not None:
            tab[:, 3] = c2.detach().to(dev).float()
        out = torch.empty_like(a)
        ops.ddpm_step_ex(b, a, tab, t=t, clip_denoised=False, mean_out=out)
        return out, t

    def _extract(self, a, t, x):
        """extract_into_tensor (util.py:96-99): a[t] as [B, 1, 1, 1]"""
        return a.to(t.device)[t].reshape(x.shape[0], 1, 1, 1)

    @torch.no_grad()
    def q_posterior(self, x_start, x_t, t):
        """ddpm.py:225-232 -> (posterior_mean, posterior_variance, posterior_log_variance_clipped), the variances [B, 1, 1, 1]."""
        m = self.model
        mean, t = self._affine("q_posterior", x_start, x_t, t, m.posterior_mean_coef1, m.posterior_mean_coef2)
        return mean, self._extract(m.posterior_variance, t, mean), self._extract(m.posterior_log_variance_clipped, t, mean)

    @torch.no_grad()
    def q_mean_variance(self, x_start, t):
        """ddpm.py:207-217 -> (mean, variance, log_variance) of q(x_t | x_0), the variances [B, 1, 1, 1]."""
        m = self.model
        mean, t = self._affine("q_mean_variance", x_start, None, t, m.sqrt_alphas_cumprod, None)
        return mean, self._extract(1.0 - m.alphas_cumprod, t, mean), self._extract(m.log_one_minus_alphas_cumprod, t, mean)

    @torch.no_grad()
    def predict_start_from_noise(self, x_t, t, noise):
        """ddpm.py:219-223: sqrt_recip_alphas_cumprod[t] x_t - sqrt_recipm1_alphas_cumprod[t] noise (the step kernel's x0, no clamp)."""
        m = self.model
        dev = m.device
        x_t = x_t.to(dev).float().contiguous()
        noise = noise.to(dev).float().contiguous()
        out = torch.empty_like(x_t)
        ops.ddpm_step_ex(x_t, noise, cached_step_table(m), t=t.to(dev).to(torch.int64).contiguous(), clip_denoised=False, x0_out=out)
        return out


def cached_step_table(model) -> torch.Tensor:
    """step_table(model), built once per (buffer storage, version, device): a scripted loop of single steps does not rebuild it."""
    lv = model.posterior_log_variance_clipped
    key = (lv.data_ptr(), lv._version, str(model.device))
    hit = model.__dict__.get("_ddpm_step_table")
    if hit is None or hit[0] != key:
        hit = (key, step_table(model))
        model.__dict__["_ddpm_step_table"] = hit
    return hit[1]


class AncestralStepGraph:
    """The loop's device state: the step table, the step counter (= t), the t buffer, a preallocated eps; `step` = {t from the counter,
    model call, stedm_ddpm_step_ex (with opts: the predicted x0 left in x0_pred), counter - 1}, capturable once in a hipGraph and
    replayed (the pattern of ddim.StepGraph). opts: _ExOpts (temperature table on the device) or None for the plain step."""

    def __init__(self, model, img, cond, table, clip, seed, first_id, masking, opts=None):
        self.m, self.img, self.cond, self.table, self.clip = model, img, cond, table, clip
        self.seed, self.first_id, self.masking, self.opts = seed, first_id, masking, opts
        dev = img.device
        self.step_idx = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((img.shape[0],), dtype=torch.int64, device=dev)
        self.ts_table = torch.arange(model.num_timesteps, dtype=torch.int64, device=dev)
        self.eps = torch.empty_like(img)
        self.x0_pred = None if opts is None else torch.empty_like(img)
        self.graph = None
        self.side = None

    def eval(self, x, t):
        m = self.m
        if hasattr(m, "apply_model_cfg"):
            return m.apply_model(x, t, self.cond, out=self.eps, uniform_t=True)
        return m.apply_model(x, t, self.cond).float().contiguous()

    def update(self, eps, step_idx, noise=None, mask_noise=None):
        mk, o = self.masking, self.opts
        kw = {}
        if mk is not None:
            m = self.m
            kw = dict(mask=mk["mask"], x0=mk["x0"], mask_noise=mask_noise, mask_seed=mk["mask_seed"] or 0,
                      sqrt_ac=m.sqrt_alphas_cumprod, sqrt_1mac=m.sqrt_one_minus_alphas_cumprod)
        if o is not None:
            kw.update(temperature=o.temperature, noise_dropout=o.noise_dropout, codebook=o.codebook, x0_out=self.x0_pred)
        ops.ddpm_step_ex(self.img, eps, self.table, step_idx=step_idx, clip_denoised=self.clip, noise=noise, seed=self.seed,
                         first_id=self.first_id, x_out=self.img, **kw)

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
