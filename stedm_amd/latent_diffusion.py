"""Model surface that `modules/ldm_diffusion.py::LDM_Diffusion` drives (SURVEY.md §8b seam 2), HIP-backed.

  DiffusionWrapper   ddpm.py:1398-1424  (hybrid conditioning: cat([x]+c_concat,1), cat(c_crossattn,1))
  LatentDiffusion    ddpm.py:424-…     subset on the hot path: register_schedule :120-172, q_sample :277-280,
                                        apply_model :894-995 (live lines), p_losses :1015-1048 (forward value),
                                        sample_log :1237-1250, get_learned_conditioning :554-565, the DDPM sampling surface
                                        q_mean_variance / predict_start_from_noise / q_posterior :207-232, p_mean_variance / p_sample /
                                        progressive_denoising / p_sample_loop / sample :1050-1235 (stedm_amd/ancestral.py)
Training seam (what `LDM_Diffusion.training_step` drives, modules/ldm_diffusion.py:63-73): `training_step(batch, batch_idx)` ->
`shared_step` -> `get_input` + `forward(x, c)` (t ~ U{0..T-1}) -> `p_losses`, and the `on_train_batch_start/end` hooks
(ddpm.py:345-371, 479-494, 868-882). In training mode with autograd enabled `p_losses` returns a loss tensor whose `backward()`
runs the hand-scheduled HIP backward (an autograd.Function bridge), so `loss.backward(); optimizer.step()` — Lightning's automatic
optimisation on one device, or a plain torch loop with torch.optim.AdamW — works unchanged; `training_step_hip` is the fused fast path
(HIP AdamW + EMA, gradient accumulation, bucketed all-reduce) that `stedm_amd.ldm_module.LDM_Diffusion` uses.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import StedmHipError
from .ancestral import AncestralSampler
from .ddim import DDIMSampler, guidance_rows
from .dpm_solver import DPMSolverSampler
from .plms import PLMSSampler
from .schedule import POSTERIOR_BUFFERS, NoiseSchedule, PosteriorSchedule, lvlb_weights
from .tiling import TilePlan, fold_blend_cpu, image_to_uint8_cpu, unfold_tiles_cpu
from .unet import UNetModel

SAMPLERS = ("ddim", "dpm_solver", "plms")          # sample_log / predict_latents(sampler=...)
DPM_OPTIONS = ("order", "method", "skip_type", "predict_x0", "solver_type", "lower_order_final", "denoise_to_zero", "thresholding", "max_val",
               "t_start", "t_end")                  # predict_latents(sampler="dpm_solver", dpm_solver={...}): DPMSolverSampler.sample keywords
ANCESTRAL = "ddpm"                                  # the reference's 1000-step ancestral chain: sample_log(ddim=False) / sampler="ddpm"
ALL_SAMPLERS = SAMPLERS + (ANCESTRAL,)


def instantiate_from_config(config):
    """ldm/util.py:78-93 restricted to targets this package provides (reference target strings are mapped)."""
    import importlib
    if "target" not in config:
        raise KeyError("Expected key `target` to instantiate.")
    alias = {
        "ldm.modules.diffusionmodules.openaimodel.UNetModel": "stedm_amd.unet.UNetModel",
        "ldm.modules.encoders.modules.SpatialRescaler": "stedm_amd.style.SpatialRescaler",
    }
    target = alias.get(config["target"], config["target"])
    module, cls = target.rsplit(".", 1)
    return getattr(importlib.import_module(module), cls)(**config.get("params", dict()))


def instantiate_first_stage(config):
    """ddpm.py:530-535 (`instantiate_first_stage`): the reference targets `ldm.models.autoencoder.VQModelInterface`, `.AutoencoderKL` and
    `.IdentityFirstStage` map to the HIP stages of stedm_amd.vq; any other target must be importable as it stands."""
    cfg = dict(config)
    target = cfg.get("target")
    if target is None:
        raise KeyError("Expected key `target` to instantiate.")
    module, _, name = target.rpartition(".")
    if module in ("ldm.models.autoencoder", "stedm_amd.vq") and name in ("VQModelInterface", "AutoencoderKL", "IdentityFirstStage"):
        try:
            from . import vq
        except ImportError as e:
            raise NotImplementedError(f"first_stage_config target {target!r}: the HIP first stage is not available ({e}); pass a module "
                                      "as first_stage_config or leave it None for sampling up to the latents") from e
        return getattr(vq, name)(**cfg.get("params", dict())).eval()
    return instantiate_from_config(cfg).eval()


class DiffusionWrapper(nn.Module):
    """ddpm.py:1398-1424."""

    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = diff_model_config if isinstance(diff_model_config, nn.Module) else instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        assert self.conditioning_key in [None, 'concat', 'crossattn', 'hybrid', 'adm']
        if self.conditioning_key != 'hybrid':
            raise NotImplementedError("only conditioning_key='hybrid' is used by STEDM (conf/diffusion/ldm_based.yaml:12)")

    @torch.no_grad()
    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, out=None, uniform_t=False):
        cc = c_crossattn[0] if len(c_crossattn) == 1 else torch.cat(c_crossattn, 1)
        xc = c_concat[0] if len(c_concat) == 1 else torch.cat(c_concat, 1)
        return self.diffusion_model.forward_parts(x, xc, t, cc, out=out, uniform_t=uniform_t)   # cat folded into the first conv

    def _same_tensor(self, a, b) -> bool:
        """Content equality of two conditioning tensors, decided once per (storage, version) pair (no per-step sync). An entry
        keeps both tensors alive, so a freed tensor's address cannot reappear under a stale verdict."""
        if a is b or (a.shape == b.shape and a.data_ptr() == b.data_ptr()):
            return True
        if a.shape != b.shape:
            return False
        key = (a.data_ptr(), a._version, b.data_ptr(), b._version, tuple(a.shape))
        cache = self.__dict__.setdefault("_eq_cache", {})
        if key not in cache:
            if len(cache) > 64:
                cache.clear()
            cache[key] = (bool(torch.equal(a, b)), a, b)
        return cache[key][0]

    @torch.no_grad()
    def forward_cfg(self, x, t, cond: dict, uncond: dict, out=None, uniform_t=False):
        """cond/uncond evaluations of ddim.py:177-178 in one shared-encoder pass. Requires equal c_concat (the
        reference's unconditional batch keeps the segmentation, ldm_diffusion.py:86); otherwise two passes."""
        cc_c, cc_u = cond["c_concat"], uncond["c_concat"]
        same = len(cc_c) == len(cc_u) and all(self._same_tensor(a, b) for a, b in zip(cc_c, cc_u))
        if not same:
            B = x.shape[0]
            if out is None:
                out = torch.empty((2 * B, self.diffusion_model.out_channels) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
            self.forward(x, t, **cond, out=out[:B], uniform_t=uniform_t)
            self.forward(x, t, **uncond, out=out[B:], uniform_t=uniform_t)
            return out[:B], out[B:]
        xc = cc_c[0] if len(cc_c) == 1 else torch.cat(cc_c, 1)
        ca = cond["c_crossattn"]; cu = uncond["c_crossattn"]
        ca = ca[0] if len(ca) == 1 else torch.cat(ca, 1)
        cu = cu[0] if len(cu) == 1 else torch.cat(cu, 1)
        return self.diffusion_model.forward_cfg(x, xc, t, ca, cu, out=out, uniform_t=uniform_t)


class _HipTrainingLoss(torch.autograd.Function):
    """`loss = p_losses(...)` with a grad_fn: forward runs the HIP U-Net forward (tape kept by the trainer) and the loss kernel of the
    model's objective (a learned logvar's gradient lands in its slot of the trainer's gradient arena),
    backward runs the hand-scheduled HIP backward and ACCUMULATES into every parameter's `.grad` (autograd's contract: several
    `loss.backward()` between two `zero_grad()` sum up — Lightning's accumulate_grad_batches relies on it). c_concat / c_crossattn
    receive their gradients as ordinary autograd inputs, so a conditioning module that runs under autograd upstream (e.g. a
    torchvision embedder) trains through this node. One forward may be outstanding at a time (the tape lives in the trainer)."""

    @staticmethod
    def forward(ctx, anchor, c_concat, c_crossattn, ld, x_start, t, noise, cond_input):
        tr = ld._trainer_or_default()
        with torch.no_grad():
            x_noisy = ld.q_sample(x_start, t, noise)
            pred = tr.forward(x_noisy, c_concat.float().contiguous(), t, c_crossattn.float().contiguous())
            dpred = tr._buf(f"dpred.{tuple(pred.shape)}", tuple(pred.shape))
            obj = ld._objective()
            loss = tr.loss(pred, noise, t, obj, dpred)
        tr._fwd_token = getattr(tr, "_fwd_token", 0) + 1
        ctx.ld, ctx.token, ctx.dpred, ctx.nx, ctx.cond_input = ld, tr._fwd_token, dpred, x_noisy.shape[1], cond_input
        ctx.obj = obj
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        ld = ctx.ld
        tr = ld._trainer
        if tr._fwd_token != ctx.token:
            raise RuntimeError("p_losses: a newer training forward replaced this one's tape; call backward() before the next forward")
        with torch.no_grad():
            had = tr.internal_grads()
            dx, dctx = tr.backward(ctx.dpred * g)
            if ctx.obj.learned:
                tr._logvar_slot(ctx.obj).mul_(g)          # written by the forward's loss kernel for an upstream gradient of 1
            cs = ld.cond_stage_model
            if ld._cond_stage_in_optimizer() and ctx.cond_input is not None and hasattr(cs, "backward"):
                cs.backward(ctx.cond_input, dx[:, ctx.nx:].contiguous())
            ld._style_encoder_backward(dctx)
            tr.publish_grads(1.0, accumulate=had)
            tr._ema_pending = True
        dcc = dx[:, ctx.nx:].contiguous() if ctx.needs_input_grad[1] else None
        return torch.zeros_like(g), dcc, (dctx if ctx.needs_input_grad[2] else None), None, None, None, None, None


class LatentDiffusion(nn.Module):
    """Hot-path subset of ddpm.py::LatentDiffusion / DDPM with the attribute names its callers read."""

    def __init__(self, unet_config, timesteps=1000, beta_schedule="linear", linear_start=1e-4, linear_end=2e-2,
                 loss_type="l2", image_size=256, channels=3, conditioning_key=None, parameterization="eps",
                 cond_stage_config=None, first_stage_config=None, cond_stage_trainable=False, first_stage_key="image",
                 cond_stage_key="image", log_every_t=100, scale_factor=1.0, use_graph=False, use_ema=True, scale_by_std=False,
                 l_simple_weight=1.0, original_elbo_weight=0.0, learn_logvar=False, logvar_init=0., clip_denoised=True, v_posterior=0.,
                 scheduler_config=None, **ignored):
        super().__init__()
        if parameterization != "eps":
            raise NotImplementedError(f"parameterization {parameterization!r}: every sampler and the training step are built for eps-prediction")
        if loss_type not in ("l1", "l2"):
            raise NotImplementedError(f"unknown loss type {loss_type!r} (ddpm.py:282-295 knows 'l1' and 'l2')")
        self.parameterization = parameterization
        self.image_size = image_size
        self.channels = channels
        self.first_stage_key = first_stage_key
        self.cond_stage_key = cond_stage_key
        self.cond_stage_trainable = cond_stage_trainable
        self.log_every_t = log_every_t
        self.clip_denoised = bool(clip_denoised)      # ddpm.py:63, 83: the ancestral chain's clamp of the predicted x0
        if v_posterior != 0.:
            raise NotImplementedError("v_posterior != 0: no reference config sets it (ddpm.py:69 defaults to 0)")
        self.v_posterior = 0.
        self.loss_type = loss_type
        self.l_simple_weight = float(l_simple_weight)              # ddpm.py:101-102, 1040-1045
        self.original_elbo_weight = float(original_elbo_weight)
        self.scale_by_std = scale_by_std
        self.scale_factor = scale_factor
        self.learn_logvar = bool(learn_logvar)
        self.use_ema = use_ema          # ddpm.py:58,91-94: LitEma over `model`; the shadows live in the trainer (stedm_amd/train.py)
        # ddpm.py:95-97, 1364-1386: a {target, params} config of one of ldm/lr_scheduler.py's classes becomes the fused optimizer's
        # per-step LambdaLR (stedm_amd/lr_scheduler.py; configure_trainer hands its `schedule` over). Built here or refused, never dropped
        self.use_scheduler = scheduler_config is not None
        self.scheduler_config = scheduler_config
        self.lr_scheduler = None
        if self.use_scheduler:
            from .lr_scheduler import instantiate_from_config as instantiate_scheduler
            self.lr_scheduler = instantiate_scheduler(scheduler_config)
        self.restarted_from_ckpt = False
        self.use_graph = use_graph
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.cond_stage_model = None
        if cond_stage_config is not None:
            self.cond_stage_model = cond_stage_config if isinstance(cond_stage_config, nn.Module) else instantiate_from_config(cond_stage_config)
        if first_stage_config is None or isinstance(first_stage_config, nn.Module):
            self.first_stage_model = first_stage_config
        else:
            # a {target, params} config (what conf/diffusion/first_stage_config/vq-f4.yaml holds): built here or refused — never
            # silently dropped (a dropped first stage would make get_input hand all-zero latents to the training step)
            self.first_stage_model = instantiate_first_stage(first_stage_config)
        self.register_schedule(beta_schedule=beta_schedule, timesteps=timesteps, linear_start=linear_start, linear_end=linear_end)
        self.register_buffer("logvar", torch.full(fill_value=float(logvar_init), size=(self.num_timesteps,)))      # ddpm.py:115-117
        if self.learn_logvar:
            self.logvar = nn.Parameter(self.logvar, requires_grad=True)        # same state-dict key

    # ------------------------------------------------------------------------------------------ schedule
    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        """ddpm.py:120-172 (the buffers the hot path reads). The ancestral sampler's buffers (POSTERIOR_BUFFERS: posterior mean
        coefficients and log variance, sqrt_recip(m1)_alphas_cumprod, log_one_minus_alphas_cumprod) are registered non-persistent: the
        state dict keeps its layout, and a checkpoint's copies of them load as unexpected keys as before."""
        assert given_betas is None
        ns = NoiseSchedule.make(timesteps, linear_start, linear_end, beta_schedule)
        self.num_timesteps = ns.num_timesteps
        self.linear_start, self.linear_end = linear_start, linear_end
        for name in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
            self.register_buffer(name, torch.from_numpy(getattr(ns, name).copy()))
        ps = PosteriorSchedule.make(timesteps, linear_start, linear_end, beta_schedule, v_posterior=getattr(self, "v_posterior", 0.))
        for name in POSTERIOR_BUFFERS:
            self.register_buffer(name, torch.from_numpy(getattr(ps, name).copy()), persistent=False)
        # the weight of p_losses' variational-bound term (ddpm.py:162-172), non-persistent there too
        self.register_buffer("lvlb_weights", torch.from_numpy(lvlb_weights(timesteps, linear_start, linear_end, beta_schedule,
                                                                            v_posterior=getattr(self, "v_posterior", 0.))), persistent=False)

    @property
    def device(self):
        return self.betas.device

    # ------------------------------------------------------------------------------------------ conditioning
    def get_learned_conditioning(self, c):
        """ddpm.py:554-565 with a module cond stage (SpatialRescaler has `encode`)."""
        if hasattr(self.cond_stage_model, 'encode') and callable(self.cond_stage_model.encode):
            return self.cond_stage_model.encode(c)
        return self.cond_stage_model(c)

    # ------------------------------------------------------------------------------------------ denoiser
    @staticmethod
    def _as_cond_dict(cond, key='c_crossattn'):
        if isinstance(cond, dict):
            return cond
        if not isinstance(cond, list):
            cond = [cond]
        return {key: cond}

    @torch.no_grad()
    def apply_model(self, x_noisy, t, cond, return_ids=False, out=None, uniform_t=False):
        """ddpm.py:894-903 + 989-995. uniform_t: all entries of t are equal (the DDIM loop, ddim.py:141)."""
        self._refuse_tiled_unet()
        return self.model(x_noisy, t, **self._as_cond_dict(cond), out=out, uniform_t=uniform_t)

    @torch.no_grad()
    def apply_model_cfg(self, x_noisy, t, cond, uncond, out=None, uniform_t=False):
        """(e_t, e_t_uncond) of ddim.py:177-178 in one pass (see UNetModel.forward_cfg)."""
        self._refuse_tiled_unet()
        return self.model.forward_cfg(x_noisy, t, self._as_cond_dict(cond), self._as_cond_dict(uncond), out=out, uniform_t=uniform_t)

    def _refuse_tiled_unet(self):
        """ddpm.py:905-906: with `split_input_params` set the reference tiles the U-Net call too and asserts a single conditioning entry;
        STEDM's hybrid conditioning has two, and a tiled U-Net is not built."""
        if getattr(self, "split_input_params", None) is not None:
            raise NotImplementedError("apply_model with split_input_params set: the reference's tiled U-Net call asserts len(cond) == 1 "
                                      "(ddpm.py:906) and hybrid conditioning has two entries; to tile the first stage only, pass split= to "
                                      "decode_first_stage / encode_first_stage instead of setting the attribute")

    # ------------------------------------------------------------------------------------------ training-side forward values
    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None):
        """ddpm.py:277-280 (+ extract_into_tensor util.py:96-99): one elementwise HIP kernel, per-sample scalars gathered from the
        fp32 schedule buffers by t."""
        noise = torch.randn_like(x_start) if noise is None else noise
        return ops.q_sample(x_start.float().contiguous(), noise.float().contiguous(), t.to(torch.int64).contiguous(),
                            self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)

    def p_losses(self, x_start, cond, t, noise=None, cond_input=None):
        """ddpm.py:1015-1048 on the HIP loss kernels: the whole objective (loss_type l1 / l2, logvar, l_simple_weight,
        original_elbo_weight) through stedm_diffusion_loss, its plain point (l1, logvar == 0, weights 1 and 0: loss == loss_simple) through
        stedm_l1_loss. In training mode with autograd enabled the returned loss carries a grad_fn (`_HipTrainingLoss`):
        `loss.backward()` runs the HIP backward, as autograd does for the reference in training_step (ddpm.py:345-358). Otherwise:
        the forward value only."""
        prefix = 'train' if self.training else 'val'
        if self.training and torch.is_grad_enabled():
            if t.is_floating_point():
                raise TypeError("the training step takes integer timesteps (floating ones are DPM-Solver's inference path); got " + str(t.dtype))
            noise = torch.randn_like(x_start) if noise is None else noise
            cd = self._as_cond_dict(cond)
            cc, ca = cd["c_concat"], cd["c_crossattn"]
            xc = cc[0] if len(cc) == 1 else torch.cat(cc, 1)
            ctx = ca[0] if len(ca) == 1 else torch.cat(ca, 1)
            if cond_input is None:
                cond_input = self.__dict__.get("_last_cond_input")      # left by get_input: the raw layout the cond stage saw
            tr = self._trainer_or_default()
            if self._cond_stage_in_optimizer() and cond_input is None:
                raise ValueError("the cond stage is in the optimizer (cond_stage_trainable): its gradient needs the raw layout given to the "
                                 "cond stage — call get_input first or pass cond_input")
            loss = _HipTrainingLoss.apply(self._grad_anchor(x_start.device), xc, ctx, self, x_start.float().contiguous(),
                                          t.to(torch.int64).contiguous(), noise, cond_input)
            return loss, self._loss_dict(prefix, loss.detach(), tr.last_loss_terms)
        with torch.no_grad():
            noise = torch.randn_like(x_start) if noise is None else noise
            x_noisy = self.q_sample(x_start, t, noise)
            model_output = self.apply_model(x_noisy, t, cond)
            obj = self._objective()
            if obj.plain:
                loss = ops.l1_loss(model_output.contiguous(), noise.float().contiguous(), None,
                                   torch.empty((1024,), dtype=torch.float64, device=x_noisy.device),
                                   torch.empty((1,), dtype=torch.float32, device=x_noisy.device))[0]
                return loss, self._loss_dict(prefix, loss, None)
            terms = ops.diffusion_loss(model_output.contiguous(), noise.float().contiguous(), t.to(torch.int64).contiguous(), obj.logvar.detach(),
                                       obj.lvlb, obj.kind, obj.l_simple_weight, obj.elbo_weight)
        return terms[0], self._loss_dict(prefix, terms[0], terms)

    def _objective(self):
        """The objective as the trainer takes it (stedm_amd/train.py: Objective). Whether it is the plain point is decided once per
        (logvar storage, version): a non-learned logvar that holds a nonzero (logvar_init, a loaded checkpoint) leaves it."""
        from .train import Objective
        lv = self.logvar
        key = (self.loss_type, self.l_simple_weight, self.original_elbo_weight, self.learn_logvar, lv.data_ptr(), lv._version,
               self.lvlb_weights.data_ptr())
        hit = self.__dict__.get("_objective_cache")
        if hit is None or hit[0] != key:
            plain = (self.loss_type == 'l1' and self.l_simple_weight == 1.0 and self.original_elbo_weight == 0.0 and not self.learn_logvar
                     and not bool(lv.detach().any()))
            hit = (key, Objective(self.loss_type, self.l_simple_weight, self.original_elbo_weight, lv, self.lvlb_weights, self.learn_logvar, plain))
            self.__dict__["_objective_cache"] = hit
        return hit[1]

    def _loss_dict(self, prefix: str, loss, terms) -> dict:
        """p_losses' loss_dict (ddpm.py:1020-1046) from the loss kernel's {loss, loss_simple, loss_gamma, loss_vlb} (device values, no
        host sync); terms None: the plain objective, whose loss is loss_simple."""
        if terms is None:
            return {f"{prefix}/loss_simple": loss, f"{prefix}/loss": loss}
        terms = terms.detach().clone()            # (the trainer's buffer is overwritten by the next step)
        d = {f"{prefix}/loss_simple": terms[1]}
        if self.learn_logvar:
            d[f"{prefix}/loss_gamma"] = terms[2]
            d["logvar"] = self.logvar.data.mean()
        d[f"{prefix}/loss_vlb"] = terms[3]
        d[f"{prefix}/loss"] = terms[0]
        return d

    def _cond_stage_in_optimizer(self) -> bool:
        """whether the trainer's extra parameters include the cond stage's (a learned logvar is one too, and needs no cond_input)"""
        tr = self.__dict__.get("_trainer")
        lv = self.logvar if self.learn_logvar else None
        style = {id(p) for p in self._style_encoder_params()}
        return tr is not None and any(p is not lv and id(p) not in style for p in tr.extra_params)

    def _style_encoder_params(self) -> list:
        """parameters of a trainable style encoder (S_ZSS_DM(train_style_encoder=True)); none here"""
        return []

    def _style_encoder_backward(self, dctx) -> None:
        """hands dL/dc_crossattn to a trainable style encoder (S_ZSS_DM(train_style_encoder=True)); nothing here"""
        return None

    def _grad_anchor(self, device) -> torch.Tensor:
        """a scalar that requires grad, so that the bridge node is part of the autograd graph (not a Parameter: it must stay out of
        the state dict and of `parameters()`)"""
        a = self.__dict__.get("_anchor")
        if a is None or a.device != device:
            a = torch.zeros((), device=device, requires_grad=True)
            self.__dict__["_anchor"] = a
        return a

    # ------------------------------------------------------------------------------------------ the reference's training seam
    def get_input(self, batch, k, return_first_stage_outputs=False, force_c_encode=False, cond_key=None, return_original_cond=False, bs=None,
                  posterior_seed=None, sample_id0=0):
        """ddpm.py:656-706 for the paths the STEDM configs take: batch tensors NHWC (DDPM.get_input, ddpm.py:332-338) -> latents of
        the first stage (encode_first_stage, per-sample loop of ddpm.py:866 batched) and the conditioning: the raw cond input while
        `cond_stage_trainable` (the caller encodes it: forward / S_ZSS_DM.get_input), its encoding otherwise. -> [z, c].
        posterior_seed / sample_id0: a KL first stage samples its posterior for sample b from (posterior_seed, global sample id
        sample_id0 + b) (get_first_stage_encoding); None draws one seed per call from torch's CPU generator. Ignored by a VQ stage."""
        with torch.no_grad():
            x = batch[k]
            if x.dim() == 3:
                x = x[..., None]
            if bs is not None:
                x = x[:bs]
            x = x.permute(0, 3, 1, 2).float().contiguous().to(self.device)
            z = self.get_first_stage_encoding(self.encode_first_stage(x), seed=posterior_seed, sample_id0=sample_id0).detach()
            c = xc = None
            if self.model.conditioning_key is not None:
                cond_key = self.cond_stage_key if cond_key is None else cond_key
                if cond_key in ('caption', 'coordinates_bbox', 'class_label'):
                    raise NotImplementedError(f"cond_key {cond_key!r}: text / box / class conditioning is unused by STEDM")
                if cond_key != self.first_stage_key:
                    xc = batch[cond_key]
                    if xc.dim() == 3:
                        xc = xc[..., None]
                    xc = xc.permute(0, 3, 1, 2).float().contiguous().to(self.device)
                else:
                    xc = x
                if bs is not None:
                    xc = xc[:bs]
                c = self.get_learned_conditioning(xc) if (not self.cond_stage_trainable or force_c_encode) else xc
        out = [z, c]
        if return_first_stage_outputs:
            out.extend([x, self.decode_first_stage(z)])
        if return_original_cond:
            out.append(xc)
        return out

    def encode_first_stage(self, x, split=None, tile_batch=None):
        """ddpm.py:828-866. split (a dict with the reference's `split_input_params` keys) or, when it is None, the attribute
        `split_input_params` set by the caller selects the patch-distributed path while its `patch_distributed_vq` is true: overlapping
        crops of ks / stride IMAGE pixels are encoded `tile_batch` crops at a time and blended (_tiled_first_stage). Neither: one call."""
        if self.first_stage_model is None:
            raise StedmHipError("no first stage: latents cannot be produced from images (pass first_stage_config)")
        params = self._split_params(split)
        if params is None:
            return self.first_stage_model.encode(x)
        from .vq import AutoencoderKL
        if isinstance(self.first_stage_model, AutoencoderKL):
            # ddpm.py:849-856 stacks the crops' `encode` outputs, which are distributions there: the reference's tiled encode cannot run on a KL stage
            raise NotImplementedError("encode_first_stage: the patch-distributed (tiled) encode is not available for an AutoencoderKL first stage "
                                      "(its encode returns a distribution per crop, which the reference's fold cannot blend); tiled decode works")
        if split is None:
            self.split_input_params['original_image_size'] = x.shape[-2:]       # ddpm.py:835
        return self._tiled_first_stage(x, params, True, tile_batch)

    # ------------------------------------------------------------------------------------------ patch-distributed first stage
    def _split_params(self, split):
        """the dict that drives the tiled path, or None for the one-call path (ddpm.py:718-719, 830-831)"""
        params = split if split is not None else getattr(self, "split_input_params", None)
        if params is None or not params["patch_distributed_vq"]:
            return None
        return params

    @torch.no_grad()
    def _tiled_first_stage(self, x, params, encode: bool, tile_batch=None, out_u8: bool = False):
        """ddpm.py:720-755 / 832-861: unfold -> first stage over the crops -> weighted fold / normalisation, with the crops run as batches of
        `tile_batch` crops x B samples (the reference runs one call per crop). tile_batch None: TilePlan.default_tile_batch, which keeps one
        call within tiling.CALL_LATENT_PIXELS (16 latents of 128 x 128: half of what the VQ-f4 decoder's 32-bit plane offsets admit). The plan refuses unusable settings before any device work.
        Works with any first stage exposing `.encode` / `.decode` on NCHW fp32. GPU tensors run the HIP kernels (ops.unfold_tiles,
        ops.fold_blend); other tensors the same plan in torch (tiling.unfold_tiles_cpu, fold_blend_cpu)."""
        x = x.float().contiguous()
        B, _, h, w = x.shape
        plan = TilePlan.from_split(params, h, w, encode)
        nb = plan.default_tile_batch(B) if tile_batch is None else int(tile_batch)
        if nb < 1:
            raise ValueError(f"tile_batch must be at least 1, got {tile_batch}")
        fs = self.first_stage_model
        run = fs.encode if encode else fs.decode
        gpu = x.is_cuda
        th, tw = plan.tile
        # a stage whose arithmetic depends on the batch of a call (VQModelInterface: split-K by launch size) is asked for its batch-invariant
        # mode, so that the result does not depend on tile_batch
        switch = isinstance(getattr(fs, "batch_invariant", None), bool) and not fs.batch_invariant
        if switch:
            fs.batch_invariant = True
        try:
            stack = self._run_crops(x, plan, run, nb, gpu, params)
        finally:
            if switch:
                fs.batch_invariant = False
        if gpu:
            w_tile, w_tie = plan.weights(x.device)
            out, out8 = ops.fold_blend(stack, w_tile, w_tie, plan.out_stride, (plan.Ly, plan.Lx), want_f32=not out_u8, want_u8=out_u8)
            return out8 if out_u8 else out
        out = fold_blend_cpu(stack, plan)
        return image_to_uint8_cpu(out) if out_u8 else out

    @staticmethod
    def _run_crops(x, plan, run, nb, gpu, params):
        """the first stage over the crops of x, nb crops per call -> the tile stack [L, B, C, th, tw]"""
        B = x.shape[0]
        th, tw = plan.tile
        stack = None
        for l0 in range(0, plan.L, nb):
            nl = min(nb, plan.L - l0)
            crops = ops.unfold_tiles(x, plan.ks, plan.stride, l0, nl) if gpu else unfold_tiles_cpu(x, plan, l0, nl)
            o = run(crops.view((nl * B,) + tuple(crops.shape[2:])))
            if o.dim() != 4 or o.shape[0] != nl * B or tuple(o.shape[2:]) != (th, tw):
                raise StedmHipError(f"tiled first stage: crops of {plan.ks} gave {tuple(o.shape)}, the plan (vqf = {params['vqf']}) expects "
                                    f"[{nl * B}, C, {th}, {tw}]")
            if stack is None:
                stack = torch.empty((plan.L, B, o.shape[1], th, tw), dtype=torch.float32, device=x.device)
            stack[l0:l0 + nl].copy_(o.view(nl, B, o.shape[1], th, tw))
        return stack

    def get_first_stage_encoding(self, encoder_posterior, noise=None, seed=None, sample_id0=0):
        """ddpm.py:545-552. A tensor (the VQ interface returns the latent itself): scale_factor * it. The KL stage's
        DiagonalGaussianDistribution: scale_factor * its sample, the scale folded into the sampling kernel; noise / seed / sample_id0 as
        DiagonalGaussianDistribution.sample takes them (given noise, or the per-sample stream of (seed, sample_id0 + b), the seed drawn from
        torch's CPU generator when neither is given)."""
        from .distributions import DiagonalGaussianDistribution
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            return encoder_posterior.sample(noise=noise, seed=seed, sample_id0=sample_id0, scale=self.scale_factor)
        if not isinstance(encoder_posterior, torch.Tensor):
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * encoder_posterior

    def forward(self, x, c, *args, **kwargs):
        """ddpm.py:873-882: t ~ U{0..T-1} per sample, encode the conditioning when the cond stage is trainable, p_losses."""
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=self.device).long()
        if self.model.conditioning_key is not None:
            assert c is not None
            if self.cond_stage_trainable:
                self.__dict__["_last_cond_input"] = c
                c = self.get_learned_conditioning(c)
        return self.p_losses(x, c, t, *args, **kwargs)

    def shared_step(self, batch, **kwargs):
        """ddpm.py:868-871."""
        x, c = self.get_input(batch, self.first_stage_key)[:2]
        return self(x, c)

    def training_step(self, batch, batch_idx):
        """ddpm.py:345-358: returns the loss tensor Lightning's automatic optimisation (or any `loss.backward()`) consumes."""
        loss, loss_dict = self.shared_step(batch)
        return loss

    @torch.no_grad()
    def on_train_batch_start(self, batch, batch_idx, dataloader_idx=-1):
        """ddpm.py:479-494 (rank-0-only std-rescale of the latents on the very first batch; inactive in the reference configs:
        `scale_by_std` is not set in conf/diffusion/ldm_based.yaml)."""
        if not (self.scale_by_std and batch_idx == 0 and not self.restarted_from_ckpt and not self.__dict__.get("_std_rescaled")):
            return
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
            return
        assert self.scale_factor == 1., 'rather not use custom rescaling and std-rescaling simultaneously'
        x = batch[self.first_stage_key].permute(0, 3, 1, 2).float().contiguous().to(self.device)
        z = self.get_first_stage_encoding(self.encode_first_stage(x)).detach()
        self.scale_factor = 1. / z.flatten().std()
        self.__dict__["_std_rescaled"] = True

    @torch.no_grad()
    def on_train_batch_end(self, *args, **kwargs):
        """ddpm.py:369-371: `self.model_ema(self.model)` after every micro-batch. The fused path (training_step_hip) has run it
        already; after a bridged `loss.backward()` it runs here, as one EMA-only kernel launch."""
        tr = self.__dict__.get("_trainer")
        if self.use_ema and tr is not None and getattr(tr, "_ema_pending", False):
            tr.ema_step()
            tr._ema_pending = False

    @torch.no_grad()
    def attach_optimizer(self, optimizer):
        """For a caller that keeps `torch.optim.AdamW` (the reference's configure_optimizers, modules/ldm_diffusion.py:224-234) on
        several ranks: DistributedDataParallel's reducer hooks never fire for the HIP backward (it is not an autograd graph over the
        parameters), so the gradient average over the ranks is done here, in a pre-step hook of the optimizer — the bucketed RCCL
        all-reduce of the published arena, once per optimizer step (what DDP's no_sync does for the accumulation window)."""
        def pre_step(opt, args, kwargs):
            tr = self.__dict__.get("_trainer")
            if tr is not None and getattr(tr, "_pub_arena", None) is not None:
                from .parallel import all_reduce_buckets
                world = all_reduce_buckets(tr._pub_arena, 256 * (1 << 20) // 4)
                if world > 1:
                    tr._pub_arena.mul_(1.0 / world)
        optimizer.register_step_pre_hook(pre_step)
        return optimizer

    def _trainer_or_default(self):
        tr = self.__dict__.get("_trainer")
        return tr if tr is not None else self.configure_trainer()

    @contextmanager
    def ema_scope(self, context=None):
        """ddpm.py:174-188: run the body with the EMA weights in the U-Net, restore the training weights afterwards."""
        tr = self.__dict__.get("_trainer")
        named = tr.ema_named() if (self.use_ema and tr is not None) else None
        unet = self.model.diffusion_model
        if named:
            with torch.no_grad():
                saved = {n: p.detach().clone() for n, p in unet.named_parameters() if n in named}
                for n, p in unet.named_parameters():
                    if n in named:
                        p.copy_(named[n])
            unet.invalidate()
        try:
            yield None
        finally:
            if named:
                with torch.no_grad():
                    for n, p in unet.named_parameters():
                        if n in saved:
                            p.copy_(saved[n])
                unet.invalidate()

    # ------------------------------------------------------------------------------------------ training step (fused fast path)
    def configure_trainer(self, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                          ema_decay: Optional[float] = 0.9999, accumulate_grad_batches: int = 1, gradient_clip_val: Optional[float] = None,
                          gradient_clip_algorithm: str = "norm"):
        """AdamW over the U-Net's parameters (modules/ldm_diffusion.py:224-234 builds `torch.optim.AdamW(self._model.model.parameters()
        ...)`) + the EMA shadow of ddpm.py:369-371 / ema.py:25-44, as one fused kernel (stedm_amd/train.py).
        gradient_clip_val / gradient_clip_algorithm: Lightning's `Trainer` arguments of the same names (which it refuses under manual
        optimisation): the total gradient norm over the optimizer's parameters is clipped on the device before AdamW ("norm"; "value" is
        not built and raises). None or 0 (Lightning's "no clipping"): off. With a `scheduler_config` the learning rate follows its schedule,
        one scheduler step per optimizer step (ddpm.py:1374-1385: LambdaLR at interval "step").
        accumulate_grad_batches: `Trainer(accumulate_grad_batches=4)` of train_diff.py:76. A checkpoint loaded before this call
        (load_reference_state_dict) hands its EMA shadows / update counter and its AdamW state over to the new trainer."""
        from .train import UNetTrainer
        # the reference's parameter list: model.model (the U-Net) + cond_stage_model when cond_stage_trainable (true in
        # conf/diffusion/ldm_based.yaml:13 at configure time); the aggregation block is NOT in it (`hasattr(self.model, "embedder")` is
        # False, ldm_diffusion.py:230) — the style encoder is not trained by the reference as wired
        extra = []
        if self.cond_stage_trainable and self.cond_stage_model is not None and hasattr(self.cond_stage_model, "backward"):
            extra = [p for p in self.cond_stage_model.parameters() if p.requires_grad]
        if self.learn_logvar:
            # ddpm.py:1370-1372 / ldm_diffusion.py:228-229: appended after the cond stage's; no EMA shadow (LitEma covers `model` only). Its
            # gradient is written by the loss kernel into its slot of the arena's tail: it accumulates and all-reduces with that bucket
            extra.append(self.logvar)
        # a trainable style encoder (opt-in): after logvar, the position ldm_diffusion.py:230-231 gives `model.embedder`'s parameters; no EMA
        # shadow either. Its gradients accumulate and all-reduce with the arena's tail, like the cond stage's
        extra.extend(self._style_encoder_params())
        algorithm = str(gradient_clip_algorithm or "norm").lower()
        if algorithm != "norm":
            if algorithm == "value":
                raise NotImplementedError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: the fused step clips the total gradient norm "
                                          "(\"norm\"); clipping by value is not built")
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: \"norm\" or \"value\"")
        max_norm = None if gradient_clip_val is None or float(gradient_clip_val) == 0.0 else float(gradient_clip_val)
        if max_norm is not None and not max_norm > 0:
            raise ValueError(f"gradient_clip_val {gradient_clip_val!r}: a positive norm (None or 0: no clipping)")
        tr = UNetTrainer(self.model.diffusion_model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         ema_decay=ema_decay if self.use_ema else None, accumulate_grad_batches=accumulate_grad_batches, extra_params=extra,
                         max_grad_norm=max_norm, lr_lambda=self.lr_scheduler.schedule if self.lr_scheduler is not None else None)
        self.__dict__["_trainer"] = tr
        if self.__dict__.get("_ema_loaded"):
            tr.load_ema({n[len("diffusion_model."):]: v for n, v in self._ema_loaded.items()}, self._ema_num_updates)
        if self.__dict__.get("_opt_loaded") is not None:
            tr.load_optimizer_state_dict(self._opt_loaded)
        return tr

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """total gradient norm of the last optimizer step (0-d device tensor; reading it is the caller's sync). None without
        gradient_clip_val, or before the first optimizer step."""
        tr = self.__dict__.get("_trainer")
        return None if tr is None else tr.last_grad_norm

    def current_lr(self) -> float:
        """the learning rate the next optimizer step runs with (the base rate without a scheduler_config)"""
        return self._trainer_or_default().current_lr()

    @torch.no_grad()
    def p_losses_backward(self, x_start, cond, t, noise=None, cond_input=None):
        """p_losses (ddpm.py:1015-1048) followed by the backward pass autograd runs for the reference in training_step
        (ddpm.py:345-358): eps-parameterisation, the model's objective. Fills `.grad` of the U-Net's parameters (and of a learned logvar) and returns
        (loss, loss_dict, dL/dx_noisy over [x | c_concat], dL/dc_crossattn). With `cond_input` (the raw layout fed to the cond stage) the
        SpatialRescaler's channel-mapper gradient is filled too, and a trainable style encoder (S_ZSS_DM(train_style_encoder=True)) receives
        dL/dc_crossattn."""
        tr = self._trainer_or_default()
        noise = torch.randn_like(x_start) if noise is None else noise
        x_noisy = self.q_sample(x_start, t, noise)
        xc, ctx = self._split_cond(cond)
        if self._cond_stage_in_optimizer() and cond_input is None:
            raise ValueError("the cond stage is in the optimizer (cond_stage_trainable): pass cond_input (the raw layout given to the cond stage) so "
                             "that its gradient can be computed")
        loss, dx, dctx = tr.loss_and_backward(x_noisy, xc, t, ctx, noise, objective=self._objective())
        if cond_input is not None and hasattr(self.cond_stage_model, "backward"):
            # cond_stage_trainable (s_zss_dm.py:46-48): the layout conditioner's channel mapper receives the c_concat slice of dL/dx
            self.cond_stage_model.backward(cond_input, dx[:, x_noisy.shape[1]:].contiguous())
        self._style_encoder_backward(dctx)
        return loss, self._loss_dict("train", loss, tr.last_loss_terms), dx, dctx

    def _split_cond(self, cond):
        cd = self._as_cond_dict(cond)
        cc, ca = cd["c_concat"], cd["c_crossattn"]
        return (cc[0] if len(cc) == 1 else torch.cat(cc, 1)), (ca[0] if len(ca) == 1 else torch.cat(ca, 1))

    @torch.no_grad()
    def training_step_hip(self, x_start, cond, t=None, noise=None, cond_input=None, group=None, graph=False):
        """One micro-batch on the fused path (latents + conditioning as `get_input` returns them): t ~ U{0..T-1} (ddpm.py:878),
        p_losses + backward; every `accumulate_grad_batches`-th call averages the accumulated gradients over the ranks (bucketed
        all-reduce when torch.distributed is initialised — what DDP does for train_diff.py:75) and runs AdamW; LitEma's update runs
        after every micro-batch (ddpm.py:369-371). Returns the loss (device tensor). graph=True: the U-Net's part of the step (forward, loss,
        backward, AdamW + EMA) is captured once and replayed as one hipGraph launch (UNetTrainer.train_step_graphed) when the step is
        shape-static and self-contained — one rank, no accumulation, no trainable cond stage, no learned logvar (any other objective is
        captured with the step); the eager step runs otherwise."""
        tr = self._trainer_or_default()
        obj = self._objective()
        if t is None:
            t = torch.randint(0, self.num_timesteps, (x_start.shape[0],), device=x_start.device).long()
        noise = torch.randn_like(x_start) if noise is None else noise
        if cond_input is None:
            cond_input = self.__dict__.get("_last_cond_input")
        if self._cond_stage_in_optimizer() and cond_input is None:
            raise ValueError("the cond stage is in the optimizer (cond_stage_trainable): pass cond_input (the raw layout given to the cond stage) so "
                             "that its gradient can be computed")
        x_noisy = self.q_sample(x_start, t, noise)
        xc, ctx = self._split_cond(cond)
        after = None
        if cond_input is not None and hasattr(self.cond_stage_model, "backward"):
            nx = x_noisy.shape[1]
            after = lambda dx, dctx: self.cond_stage_model.backward(cond_input, dx[:, nx:].contiguous())
        if self._style_encoder_params():
            cond_after = after

            def after(dx, dctx):
                if cond_after is not None:
                    cond_after(dx, dctx)
                self._style_encoder_backward(dctx)
        if graph and after is None and not tr.extra_params and tr.accumulate_grad_batches == 1 and x_noisy.is_cuda:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
                return tr.train_step_graphed(x_noisy, xc, t, ctx, noise, objective=obj)
        return tr.train_step(x_noisy, xc, t, ctx, noise, group=group, after_backward=after, objective=obj)

    # ------------------------------------------------------------------------------------------ checkpoints (reference key layout)
    @staticmethod
    def _ema_name(param_name: str) -> str:
        """LitEma registers its shadow of `model.<name>` as a buffer named `<name>` without dots (ema.py:17-21)."""
        return param_name.replace('.', '')

    @torch.no_grad()
    def load_reference_state_dict(self, ckpt: dict, use_ema: bool = False):
        """Load a checkpoint written by the reference: a Lightning checkpoint ({"state_dict": ...}) of `LDM_Diffusion`, whose keys carry
        the `_model.` prefix (modules/ldm_diffusion.py:38), or a bare `LatentDiffusion.state_dict()`. U-Net, cond stage and
        aggregation block load by name (same parameter names and OIHW shapes); `model_ema.*` (ema.py) goes to the trainer's EMA
        shadows, or — with use_ema, like `ema_scope` (ddpm.py:174-188) — into the U-Net itself. `first_stage_model.*` is loaded only
        when a first stage was supplied. Returns (missing, unexpected) key lists like `load_state_dict(strict=False)`."""
        sd = ckpt.get("state_dict", ckpt)
        if isinstance(ckpt.get("optimizer_states"), (list, tuple)) and ckpt["optimizer_states"]:
            self.__dict__["_opt_loaded"] = ckpt["optimizer_states"][0]       # Lightning keeps torch's AdamW.state_dict() there
        self.restarted_from_ckpt = True
        sd = {(k[len("_model."):] if k.startswith("_model.") else k): v for k, v in sd.items()}
        ema = {k[len("model_ema."):]: v for k, v in sd.items() if k.startswith("model_ema.")}
        rest = {k: v for k, v in sd.items() if not k.startswith("model_ema.")
                and (self.first_stage_model is not None or not k.startswith("first_stage_model."))}
        res = self.load_state_dict(rest, strict=False)
        missing, unexpected = list(res.missing_keys), list(res.unexpected_keys)
        named = dict(self.model.named_parameters())
        if use_ema and ema:
            for name, p in named.items():
                key = self._ema_name(name)
                if key in ema:
                    p.copy_(ema[key].to(p.device, p.dtype))
            self.model.diffusion_model.invalidate()
        self.__dict__["_ema_loaded"] = {name: ema[self._ema_name(name)] for name in named if self._ema_name(name) in ema}
        self.__dict__["_ema_num_updates"] = int(ema["num_updates"]) if "num_updates" in ema else 0
        tr = self.__dict__.get("_trainer")
        if tr is not None:      # a trainer built before the checkpoint arrived; configure_trainer() hands both over otherwise
            if self._ema_loaded:
                tr.load_ema({n[len("diffusion_model."):]: v for n, v in self._ema_loaded.items()}, self._ema_num_updates)
            if self.__dict__.get("_opt_loaded") is not None:
                tr.load_optimizer_state_dict(self._opt_loaded)
        return missing, unexpected

    def reference_state_dict(self, prefix: str = "_model.") -> dict:
        """State dict in the reference's key layout (see load_reference_state_dict), including `model_ema.*` when a trainer holds
        EMA shadows."""
        out = {prefix + k: v for k, v in self.state_dict().items()}
        tr = self.__dict__.get("_trainer")
        if tr is not None and tr.ema_named() is not None:
            out[prefix + "model_ema.decay"] = torch.tensor(tr.ema_decay, dtype=torch.float32)
            out[prefix + "model_ema.num_updates"] = torch.tensor(tr.ema_updates, dtype=torch.int)
            for name, v in tr.ema_named().items():
                out[prefix + "model_ema." + self._ema_name("diffusion_model." + name)] = v
        return out

    def reference_checkpoint(self, prefix: str = "_model.") -> dict:
        """{"state_dict", "optimizer_states"} as Lightning's ModelCheckpoint writes them for the reference (train_diff.py:64-66):
        parameters + `model_ema.*` in the reference's key layout, AdamW state in torch.optim.AdamW.state_dict() layout. Feeding it
        back through load_reference_state_dict + configure_trainer continues the run (EMA history, moments, bias-correction step)."""
        ck = {"state_dict": self.reference_state_dict(prefix)}
        tr = self.__dict__.get("_trainer")
        if tr is not None and tr._opt is not None:
            ck["optimizer_states"] = [tr.optimizer_state_dict()]
        return ck

    # ------------------------------------------------------------------------------------------ sampling
    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None, quantize_denoised=False,
               mask=None, x0=None, shape=None, **kwargs):
        """ddpm.py:1219-1235: the ancestral chain (stedm_amd/ancestral.py, AncestralSampler.sample). Keywords the reference swallows are
        ignored (log_every_t, verbose, ddim_steps, callbacks), except those whose effect it drops, which raise: eta != 0, temperature,
        noise_dropout (both are progressive_denoising's), score_corrector, and guidance (unconditional_guidance_scale != 1 with
        unconditional_conditioning). quantize_denoised snaps every step's predicted x0 to the VQ first stage's codebook.
        Repo keywords: noises, noise_seed, sample_id0, mask_noises, mask_seed (AncestralSampler.p_sample_loop)."""
        return AncestralSampler(self, use_graph=self.use_graph).sample(cond, batch_size=batch_size, return_intermediates=return_intermediates,
                                                                       x_T=x_T, verbose=verbose, timesteps=timesteps,
                                                                       quantize_denoised=quantize_denoised, mask=mask, x0=x0, shape=shape,
                                                                       **kwargs)

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None, **kwargs):
        """ddpm.py:1169-1217 on the HIP path (AncestralSampler.p_sample_loop; kwargs: its repo keywords)."""
        return AncestralSampler(self, use_graph=self.use_graph).p_sample_loop(
            cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose, callback=callback, timesteps=timesteps,
            quantize_denoised=quantize_denoised, mask=mask, x0=x0, img_callback=img_callback, start_T=start_T, log_every_t=log_every_t,
            **kwargs)

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False, img_callback=None, mask=None,
                              x0=None, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, batch_size=None,
                              x_T=None, start_T=None, log_every_t=None, **kwargs):
        """ddpm.py:1112-1166 on the HIP path (AncestralSampler.progressive_denoising; kwargs: its repo keywords) -> (img, the list of the
        logged steps' predicted x0). The one place where the ancestral chain honours temperature (a number or a per-timestep list) and
        noise_dropout."""
        return AncestralSampler(self, use_graph=self.use_graph).progressive_denoising(
            cond, shape, verbose=verbose, callback=callback, quantize_denoised=quantize_denoised, img_callback=img_callback, mask=mask,
            x0=x0, temperature=temperature, noise_dropout=noise_dropout, score_corrector=score_corrector,
            corrector_kwargs=corrector_kwargs, batch_size=batch_size, x_T=x_T, start_T=start_T, log_every_t=log_every_t, **kwargs)

    @torch.no_grad()
    def p_mean_variance(self, x, c, t, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False, return_x0=False,
                        score_corrector=None, corrector_kwargs=None):
        """ddpm.py:1050-1079 (AncestralSampler.p_mean_variance): t int64 [B], may differ per sample."""
        return AncestralSampler(self).p_mean_variance(x, c, t, clip_denoised, return_codebook_ids=return_codebook_ids,
                                                      quantize_denoised=quantize_denoised, return_x0=return_x0,
                                                      score_corrector=score_corrector, corrector_kwargs=corrector_kwargs)

    @torch.no_grad()
    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_codebook_ids=False, quantize_denoised=False,
                 return_x0=False, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, _noise=None,
                 noise_seed=None, sample_id0=0):
        """ddpm.py:1081-1110 (AncestralSampler.p_sample): one ancestral step at the per-sample timesteps t -> x_prev or (x_prev, x0).
        Repo keywords: _noise (the step's N(0, 1) draw), else noise_seed / sample_id0 (the in-kernel draw)."""
        return AncestralSampler(self).p_sample(x, c, t, clip_denoised=clip_denoised, repeat_noise=repeat_noise,
                                               return_codebook_ids=return_codebook_ids, quantize_denoised=quantize_denoised,
                                               return_x0=return_x0, temperature=temperature, noise_dropout=noise_dropout,
                                               score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, _noise=_noise,
                                               noise_seed=noise_seed, sample_id0=sample_id0)

    def q_posterior(self, x_start, x_t, t):
        """ddpm.py:225-232 -> (posterior_mean, posterior_variance, posterior_log_variance_clipped)."""
        return AncestralSampler(self).q_posterior(x_start, x_t, t)

    def predict_start_from_noise(self, x_t, t, noise):
        """ddpm.py:219-223."""
        return AncestralSampler(self).predict_start_from_noise(x_t, t, noise)

    def q_mean_variance(self, x_start, t):
        """ddpm.py:207-217 -> (mean, variance, log_variance)."""
        return AncestralSampler(self).q_mean_variance(x_start, t)

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, sampler="ddim", **kwargs):
        """ddpm.py:1237-1250. sampler: "ddim" (the reference's) or "dpm_solver" (DPMSolverSampler, the reference's
        ldm/models/diffusion/dpm_solver: DPM-Solver++(2M), ddim_steps model evaluations; the keywords order, method, skip_type,
        predict_x0, solver_type, lower_order_final, denoise_to_zero, thresholding, max_val, t_start and t_end select the rest of the
        reference's DPM_Solver.sample, e.g. order=3 for DPM-Solver++(3M) or method="singlestep" for DPM-Solver-fast) or "plms" (PLMSSampler, the reference's
        plms.py: DDIM's schedule, n iterations cost n + 1 model evaluations, mask / x0 as DDIM; returns (x, intermediates)).
        ddim=False (or sampler="ddpm"): the reference's ancestral chain, self.sample(cond, batch_size, return_intermediates=True,
        **kwargs); ddim_steps is ignored and intermediates is a list."""
        if sampler not in ALL_SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r}; choose from {ALL_SAMPLERS}")
        if not ddim or sampler == ANCESTRAL:
            if sampler not in ("ddim", ANCESTRAL):
                raise ValueError(f"ddim=False runs the ancestral chain; sampler={sampler!r} contradicts it")
            return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)
        if sampler == "dpm_solver":
            sampler = DPMSolverSampler(self, device=self.device, use_graph=self.use_graph)
        elif sampler == "plms":
            sampler = PLMSSampler(self, use_graph=self.use_graph)
        else:
            sampler = DDIMSampler(self, use_graph=self.use_graph)
        shape = (self.channels, self.image_size, self.image_size)
        return sampler.sample(ddim_steps, batch_size, shape, cond, verbose=False, **kwargs)

    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False, split=None, tile_batch=None, out_u8=False, **kw):
        """ddpm.py:708-766 (predict_cids / force_not_quantize are accepted and ignored, as before). split / the attribute
        `split_input_params` with `patch_distributed_vq` true: the patch-distributed path over crops of ks / stride LATENT pixels
        (_tiled_first_stage; see encode_first_stage). out_u8: return predict_step's uint8 image [B,H,W,C] (images_for_saving's conversion)
        instead of the fp32 one; on the tiled path it comes out of the blend kernel's registers, no fp32 image is written."""
        if self.first_stage_model is None:
            raise NotImplementedError("decode_first_stage: this LatentDiffusion was built without a first stage; pass first_stage_config "
                                      "(built as stedm_amd.vq.VQModelInterface / AutoencoderKL) or a first_stage module")
        params = self._split_params(split)
        if params is not None:
            return self._tiled_first_stage(1. / self.scale_factor * z, params, False, tile_batch, out_u8=out_u8)
        dec = self.first_stage_model.decode(z / self.scale_factor)
        if out_u8:
            dec = dec.float().contiguous()
            return ops.image_to_uint8(dec) if dec.is_cuda else image_to_uint8_cpu(dec)
        return dec


class S_ZSS_DM(LatentDiffusion):
    """networks/s_zss_dm.py:11-60 — LatentDiffusion + style aggregation block; `get_input` emits the hybrid conditioning
    dict {"c_concat": [layout], "c_crossattn": [style]}.

    `encoder` names the torchvision embedder of the mean/max/linear aggregators in the reference ("swin_v2_t", third-party,
    SURVEY.md §8c): the Swin-V2 family is built on the HIP kernels (stedm_amd/swin.py); any other embedder can be supplied as a module
    through `embedder=`. `style_agg: svit` and `style_sampling: none` need no embedder.

    train_style_encoder (default False: the reference as wired, whose optimizer never sees the aggregation block): with `style_agg: svit`
    the set-ViT is trained with the U-Net — `get_input` in training mode keeps its forward, the training step hands it dL/dc_crossattn
    (sViT.backward) and its parameters follow `logvar` in the optimizer. Any other aggregation block raises: only the sViT has a backward.
    style_lsa_bwd ("f32" | "mfma16", default "f32"): the form of the set-ViT's attention backward (sViT(lsa_bwd=...)); ignored without
    train_style_encoder."""

    def __init__(self, encoder, sampling_cfg, agg_cfg, cfg, *args, embedder: Optional[nn.Module] = None, train_style_encoder: bool = False,
                 style_lsa_bwd: str = "f32", **kwargs):
        super().__init__(*args, **kwargs)
        self.train_style_encoder = bool(train_style_encoder)
        from . import style as st
        self._sampling_cfg = sampling_cfg
        self._agg_cfg = agg_cfg
        self._cfg = cfg
        self.embed_key = "style_imgs"
        name = lambda c: c["name"] if isinstance(c, dict) else c.name
        get = lambda c, k: c[k] if isinstance(c, dict) else getattr(c, k)
        if name(sampling_cfg) == "none":
            self._agg_block = st.Agg_None(sampling_cfg, embedder)
        elif name(agg_cfg) == "svit":
            a = dict(agg_cfg) if isinstance(agg_cfg, dict) else {k: getattr(agg_cfg, k) for k in
                                                               ("patch_size", "dim", "depth", "heads", "mlp_dim", "pool", "channels",
                                                                "dropout", "emb_dropout", "t_dim")}
            a.pop("name", None)
            data = cfg["data"] if isinstance(cfg, dict) else cfg.data
            img = data["patch_size"] if isinstance(data, dict) else data.patch_size
            ns = get(sampling_cfg, "num_patches") if name(sampling_cfg) == "mp" else 1
            self._agg_block = st.sViT(image_size=img, num_classes=512, ns=ns, lsa_bwd=style_lsa_bwd if self.train_style_encoder else "f32", **a)
        else:
            if embedder is None:
                # s_zss_dm.py:19-20: `torchvision.models.get_model(encoder)` with its head replaced by Linear(768, 512). The HIP-backed
                # Swin-V2 (stedm_amd/swin.py) keeps torchvision's state-dict names, so a torchvision checkpoint loads into it; its arithmetic
                # is torchvision's published algorithm (third-party: parity unpinned). Other encoders: pass `embedder=`.
                from .swin import get_model
                embedder = get_model(encoder)
                embedder.head = torch.nn.Linear(768, 512)
            cls = {"linear": st.Agg_Linear, "max": st.Agg_Max, "mean": st.Agg_Mean}.get(name(agg_cfg))
            if cls is None:
                raise Exception("Unkown aggregation function!")
            self._agg_block = cls(sampling_cfg, embedder)
        self.register_module("agg_block", self._agg_block)
        if self.train_style_encoder and not isinstance(self._agg_block, st.sViT):
            raise NotImplementedError(f"train_style_encoder: only the set-ViT (style_agg: svit) has a backward; got {type(self._agg_block).__name__}")
        if self.train_style_encoder:
            self._agg_block.repack_on_raw_writes = True      # the fused optimizer writes its parameters through raw pointers

    def _style_encoder_params(self) -> list:
        return list(self._agg_block.parameters()) if self.train_style_encoder else []

    def _style_encoder_backward(self, dctx) -> None:
        if self.train_style_encoder and dctx is not None:
            self._agg_block.backward(dctx.contiguous())

    def get_input(self, batch, k, cond_key=None, bs=None, predict_only: Optional[bool] = None, **kwargs):
        """s_zss_dm.py:45-60 over LatentDiffusion.get_input (ddpm.py:656-706). batch tensors are NHWC (LDM_Diffusion.prepare_batch,
        ldm_diffusion.py:51-60). Returns [z, {"c_concat": [c], "c_crossattn": [style]}].

        predict_only=True: z is a zero placeholder of the latent shape and the VQ encode is skipped — predict_step uses len(z) alone
        (ldm_diffusion.py:79-90), so the reference's two VQ encodes there are wasted work. Default (None): encode when a first stage
        exists (the reference's literal behaviour); without one, the placeholder in eval mode and an error in training mode (the
        latents are the training target: never silently zeros). posterior_seed / sample_id0 (keywords of LatentDiffusion.get_input: the
        KL first stage's per-sample posterior draw) pass through with the other keywords."""
        skip_encode = predict_only is True or (predict_only is None and self.first_stage_model is None and not self.training)
        dev = self.device
        if skip_encode or self.first_stage_model is None:
            if not skip_encode:
                raise StedmHipError("S_ZSS_DM.get_input in training mode needs the first stage (the latents are the training target): pass "
                                    "first_stage_config; the zero placeholder exists for predict_step only")
            x = batch[k] if bs is None else batch[k][:bs]
            z = torch.zeros((x.shape[0], self.channels, self.image_size, self.image_size), device=dev)
            xc = batch[cond_key or self.cond_stage_key]
            xc = (xc if bs is None else xc[:bs]).permute(0, 3, 1, 2).float().contiguous().to(dev)
            outputs = [z, xc]
        else:
            self.cond_stage_trainable = True
            outputs = LatentDiffusion.get_input(self, batch, k, cond_key=cond_key, bs=bs, **kwargs)
            self.cond_stage_trainable = False
        self.cond_stage_trainable = False
        z, c = outputs[0], outputs[1]
        self.__dict__["_last_cond_input"] = c                # raw layout: the channel mapper's gradient needs it (cond_stage_trainable)
        with torch.no_grad():
            c = self.get_learned_conditioning(c)
            style_imgs = batch[self.embed_key]
            if bs is not None:
                style_imgs = style_imgs[:bs]
            keep = self.train_style_encoder and self.training
            if keep:
                self._agg_block.keep_for_backward = True
            try:
                style_features = self._agg_block(style_imgs.to(dev))
            finally:
                if keep:
                    self._agg_block.keep_for_backward = False
        noutputs = [z, {"c_concat": [c], "c_crossattn": [style_features]}]
        noutputs.extend(outputs[2:])
        return noutputs


@torch.no_grad()
def prepare_batch(batch, device=None) -> dict:
    """LDM_Diffusion.prepare_batch (modules/ldm_diffusion.py:51-60): the DataModule's tuple (image [B,3,H,W], one-hot segmentation
    [B,K,H,W], _, style images [B,n,3,H,W], ...) -> the NHWC dict `get_input` reads. The class merge of the segmentation (channel 1 =
    sum of the classes >= 1) and its NHWC layout come from one HIP kernel; image and style stack are views, as in the reference."""
    dev = device or batch[1].device
    seg = ops.seg_merge(batch[1].to(dev).float().contiguous())
    return {"image": batch[0].permute(0, 2, 3, 1), "segmentation": seg, "style_imgs": batch[3].permute(0, 1, 3, 4, 2)}


@torch.no_grad()
def predict_latents(model: S_ZSS_DM, ldm_batch: dict, ddim_steps: int, eta: float = 0.0, cfg_scale: float = 1.0,
                    style_sampling: str = "nearby", x_T: Optional[torch.Tensor] = None, dedup_uncond: bool = True, noises=None,
                    mask: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None, mask_seed: Optional[int] = None, sample_id0: int = 0,
                    sampler: str = "ddim", noise_seed: Optional[int] = None, dpm_solver: Optional[dict] = None):
    """Lightning-free restatement of LDM_Diffusion.predict_step (modules/ldm_diffusion.py:76-91) up to the sampled latents:
    conditional get_input, unconditional batch {image: 0, segmentation: same, style_imgs: -2}, DDIM + CFG.

    dedup_uncond: the unconditional style input is the same constant (-2) image stack for every sample (ldm_diffusion.py:86) and the
    style encoder works per sample, so its output is one vector: it is computed for ONE sample and broadcast instead of running the
    encoder over the whole constant batch; the layout conditioning of the unconditional batch is the conditional one (same
    segmentation). False: the reference's literal second get_input.

    Masked sampling (DDIMSampler.sample's mask / x0, ddim.py:143-146): mask == 1 keeps the real tile, mask == 0 lets the model generate,
    soft values blend. x0 defaults to the latent of the batch's own image (get_input with the first-stage encode: the `z` the reference
    computes and discards). mask is at latent resolution ([B|1, 1|C, h, w]) or at image resolution ([B, 1, H, W] or [B, H, W], H = f h):
    an image mask is min-pooled by the first stage's factor f, so a latent pixel is kept only where its whole f x f footprint is kept.
    mask_seed / sample_id0: the per-sample stream of the blend's noise (DDIMSampler.sample). The returned latent is the model's output:
    its kept region is close to x0, not pasted from it.

    sampler: "ddim" (default) or "dpm_solver" (DPM-Solver++(2M), stedm_amd/dpm_solver.py): ddim_steps is then the number of model
    evaluations; it draws no noise after x_T, and eta != 0, noises and mask are refused. "plms" (PLMS, stedm_amd/plms.py): DDIM's
    schedule and masked sampling, ddim_steps as for DDIM (n iterations, n + 1 model evaluations); it draws no noise after x_T (and the
    blend's), and eta != 0 (ValueError, as the reference) and noises are refused. "ddpm" (the ancestral chain of sample_log(ddim=False),
    stedm_amd/ancestral.py): model.num_timesteps unguided steps, ddim_steps ignored; cfg_scale != 1 with style_sampling != "none" raises
    (the reference's ancestral path has no guidance), as does eta != 0. Its step noise is drawn from (noise_seed, sample_id0 + b);
    `noises` (optional) holds one N(0,1) tensor per step.

    noise_seed with sampler="ddim" and eta != 0: every step's noise is drawn in the DDIM kernel as row sample_id0 + b of
    ops.philox_normal(noise_seed, stream 1 + iteration) (DDIMSampler.sample), so the loop can be graphed; given `noises` take precedence.
    Without it (or with eta == 0) the DDIM noise is torch's, as before.

    dpm_solver (sampler="dpm_solver" only, ValueError otherwise): a dict of DPMSolverSampler.sample's solver options (DPM_OPTIONS:
    order, method, skip_type, predict_x0, solver_type, lower_order_final, denoise_to_zero, thresholding, max_val, t_start, t_end);
    None or {} keeps DPM-Solver++(2M).

    cfg_scale may be a sequence or 1-D tensor with one guidance scale per sample of the batch (sampler="ddim" only; NotImplementedError
    otherwise): sample b is then guided at cfg_scale[b] in one batched run (DDIMSampler.sample, stedm_ddim_step_rows). A wrong length
    raises ValueError before any device work; every scale 1 is the unguided run."""
    if sampler not in ALL_SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}; choose from {ALL_SAMPLERS}")
    rows = None
    if isinstance(cfg_scale, (list, tuple)) or (isinstance(cfg_scale, (torch.Tensor, np.ndarray)) and cfg_scale.ndim > 0):
        rows = guidance_rows(cfg_scale, len(ldm_batch["image"]))
    if rows is not None:
        if sampler != "ddim":
            raise NotImplementedError(f"sampler={sampler!r} takes one cfg_scale for the batch; per-sample scales are sampler='ddim' (DDIMSampler)")
        cfg_scale = 1.0 if all(v == 1.0 for v in rows) else rows
    if dpm_solver is not None:
        if sampler != "dpm_solver":
            raise ValueError(f"dpm_solver options are for sampler='dpm_solver', got sampler={sampler!r}")
        bad = sorted(set(dpm_solver) - set(DPM_OPTIONS))
        if bad:
            raise ValueError(f"unknown dpm_solver option(s) {bad}; choose from {DPM_OPTIONS}")
    if sampler == ANCESTRAL and cfg_scale != 1 and style_sampling != "none":
        raise NotImplementedError("sampler='ddpm': the reference's ancestral chain has no classifier-free guidance (cfg_scale must be 1)")
    if sampler == ANCESTRAL and eta != 0.0:
        raise NotImplementedError("sampler='ddpm': eta is a DDIM option")
    if sampler == "dpm_solver" and (eta != 0.0 or noises is not None or mask is not None):
        raise NotImplementedError("sampler='dpm_solver': eta != 0, per-step noises and masked sampling are DDIM options")
    if sampler == "plms" and eta != 0.0:
        raise ValueError("sampler='plms': ddim_eta must be 0 for PLMS")
    if sampler == "plms" and noises is not None:
        raise NotImplementedError("sampler='plms': PLMS draws no per-step noise")
    masked = mask is not None
    z, c_0 = model.get_input(ldm_batch, "image", predict_only=not (masked and x0 is None))
    kw = {} if x_T is None else {"x_T": x_T}
    if noises is not None:          # one N(0,1) tensor per DDIM iteration in place of the global-RNG draw of ddim.py:206 (eta > 0)
        kw["noises"] = noises
    if masked:
        kw.update(mask=latent_mask(model, mask, len(z)), x0=z if x0 is None else x0, mask_seed=mask_seed, sample_id0=int(sample_id0))
    if sampler == ANCESTRAL:
        kw.update(noise_seed=noise_seed, sample_id0=int(sample_id0))
        out, _ = model.sample_log(c_0, batch_size=len(z), ddim=False, ddim_steps=ddim_steps, **kw)
        return out
    if sampler != "ddim":
        kw["sampler"] = sampler
        kw.update(dpm_solver or {})
    elif eta != 0.0 and noise_seed is not None:
        kw.update(noise_seed=int(noise_seed), sample_id0=int(sample_id0))
    if (not isinstance(cfg_scale, list) and cfg_scale == 1) or style_sampling == "none":
        out, _ = model.sample_log(c_0, batch_size=len(z), ddim=True, ddim_steps=ddim_steps, eta=eta, log_every_t=1000, **kw)
    else:
        if dedup_uncond:
            sty = ldm_batch["style_imgs"]
            one = torch.full((1,) + tuple(sty.shape[1:]), -2.0, dtype=torch.float32, device=model.device)
            unc_style = model._agg_block(one).expand(len(z), -1).contiguous()
            c_uncond = {"c_concat": c_0["c_concat"], "c_crossattn": [unc_style]}
        else:
            unc_batch = {"image": torch.zeros_like(ldm_batch["image"]), "segmentation": ldm_batch["segmentation"],
                         "style_imgs": torch.zeros_like(ldm_batch["style_imgs"]) - 2}
            z, c_uncond = model.get_input(unc_batch, "image", predict_only=True)
        out, _ = model.sample_log(c_0, batch_size=len(z), ddim=True, ddim_steps=ddim_steps, eta=eta, log_every_t=1000,
                                  unconditional_conditioning=c_uncond, unconditional_guidance_scale=cfg_scale, **kw)
    return out


def latent_mask(model: LatentDiffusion, mask: torch.Tensor, batch: int) -> torch.Tensor:
    """A sampling mask at latent resolution: latent masks ([B|1, 1|C, h, w]) pass; image masks ([B, 1, H, W] or [B, H, W] with H = f h,
    W = f w, f the first stage's downsampling factor) are min-pooled over f x f blocks (a latent pixel is kept only if its whole footprint
    is kept; soft values take the block's minimum)."""
    h = w = int(model.image_size)
    m = mask.to(model.device).float()
    if m.dim() == 3:
        m = m[:, None]
    if m.dim() != 4:
        raise ValueError(f"mask {tuple(mask.shape)}: expected [B|1, 1|C, {h}, {w}] or an image mask [B, 1, H, W] / [B, H, W]")
    if tuple(m.shape[2:]) == (h, w):
        return m.contiguous()
    H, W = int(m.shape[2]), int(m.shape[3])
    f = H // h
    enc = getattr(model.first_stage_model, "encoder", None)
    want = 2 ** (enc.num_resolutions - 1) if enc is not None and hasattr(enc, "num_resolutions") else None
    if f < 2 or H != f * h or W != f * w or m.shape[1] != 1 or (want is not None and f != want) or m.shape[0] not in (1, batch):
        raise ValueError(f"mask {tuple(mask.shape)} is neither a latent mask [B|1, 1|C, {h}, {w}] nor an image mask [B, 1, f*{h}, f*{w}]"
                         + ("" if want is None else f" with the first stage's factor f = {want}"))
    return m.reshape(m.shape[0], 1, h, f, w, f).amin(dim=(3, 5)).contiguous()


@torch.no_grad()
def predict_latents_sharded(model: S_ZSS_DM, shard_batch: dict, global_batch: int, ddim_steps: int, eta: float = 0.0, cfg_scale: float = 1.0,
                            seed: int = 0, rank: Optional[int] = None, world: Optional[int] = None, group=None, gather: bool = True,
                            mask: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None, **kw):
    """predict_step on one rank of a data-parallel prediction run (predict_diff.py:86: Trainer.predict under DDP hands every rank its shard of
    the dataset; modules/ldm_diffusion.py:76-107). `shard_batch` holds this rank's samples — the contiguous slice
    parallel.shard_range(global_batch, rank, world) of the global batch. Latents are independent, so nothing is exchanged inside the loop;
    the initial noise x_T (ddim.py:122) and, for eta > 0, every step's noise (ddim.py:206) come from per-SAMPLE streams keyed by the global
    sample id (parallel.per_sample_normal), so sample i is the same for every world size, which the reference's batch-shaped global-RNG
    draw cannot give. (On the GPU the step noise of eta > 0 is drawn inside the DDIM kernel from the same key and stream, 1 + iteration.) gather: all-gather the shards (RCCL over xGMI with backend "nccl") -> [global_batch, C, H, W] on every rank.

    mask / x0 (masked sampling, see predict_latents): given for the global batch (their rows lo:hi are taken), for the shard, or (mask
    only) as one row for every sample. The blend's noise is keyed by (seed, global sample id), like x_T.

    sampler="dpm_solver" (through **kw): DPM-Solver draws nothing after x_T, so the per-sample x_T alone makes the shards invariant.
    sampler="plms" likewise, its masked blend keyed by the global sample id as DDIM's. sampler="ddpm": every step's noise is drawn in
    the kernel from (seed, global sample id), so the ancestral chain is shard-invariant too.

    cfg_scale: one number, or per-sample scales (predict_latents) given for the global batch (rows lo:hi are taken) or for the shard."""
    import torch.distributed as dist
    from . import parallel as par
    if rank is None or world is None:
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(group), dist.get_world_size(group)) if on else (0, 1)
    lo, hi = par.shard_range(int(global_batch), rank, world)
    ids = list(range(lo, hi))
    n = len(shard_batch["image"])
    if n != hi - lo:
        raise ValueError(f"rank {rank} of {world}: the shard holds {n} samples, shard_range({global_batch}) gives {hi - lo}")
    if (isinstance(cfg_scale, (torch.Tensor, np.ndarray)) and cfg_scale.ndim == 1) or isinstance(cfg_scale, (list, tuple)):
        if len(cfg_scale) == int(global_batch) and len(cfg_scale) != n:
            cfg_scale = cfg_scale[lo:hi]
        elif len(cfg_scale) != n:
            raise ValueError(f"cfg_scale holds {len(cfg_scale)} scales: expected {int(global_batch)} (the global batch) or {n} (this shard)")
    shape = (model.channels, model.image_size, model.image_size)
    dev = model.device
    on_gpu = torch.device(dev).type == "cuda"
    # (GPU: drawn on the device from the per-sample Philox key - one launch per tensor; the numpy streams remain for CPU tensors)
    draw = (lambda st: par.per_sample_normal_device(seed, lo, hi - lo, shape, st, dev)) if on_gpu else \
           (lambda st: par.per_sample_normal(seed, ids, shape, stream=st).to(dev))
    x_T = draw(0)
    noises = None
    if eta != 0.0 and kw.get("sampler", "ddim") == "ddim" and on_gpu:
        kw.update(noise_seed=int(seed), sample_id0=lo)      # drawn in the DDIM kernel: the same rows draw(1 + i) gives, bit for bit
    elif eta != 0.0 and kw.get("sampler", "ddim") == "ddim":
        from .schedule import make_ddim_timesteps
        n_iter = int(make_ddim_timesteps(int(ddim_steps), model.num_timesteps).shape[0])      # (S = 6 -> 7 iterations: ddim.py's uniform stride)
        noises = [draw(1 + i) for i in range(n_iter)]
    if mask is not None:
        rows = lambda a: a[lo:hi] if (a.shape[0] == int(global_batch) and a.shape[0] != n) else a
        kw.update(mask=rows(mask), x0=None if x0 is None else rows(x0), mask_seed=int(seed), sample_id0=lo)
    if kw.get("sampler") == ANCESTRAL:
        kw.update(noise_seed=int(seed), sample_id0=lo)
    from ._lib import StedmHipError
    err: Optional[StedmHipError] = None
    lat = None
    try:
        lat = predict_latents(model, shard_batch, ddim_steps, eta=eta, cfg_scale=cfg_scale, x_T=x_T, noises=noises, **kw)
    except StedmHipError as e:       # (the fp16 range guard raises at the end of the loop: ddim.py's f16_guard_check)
        if not (gather and world > 1):
            raise
        err = e
    if gather and world > 1:
        # a rank that raised must not leave the others waiting in the all-gather: agree on the outcome first (one 4-byte all-reduce)
        flag = torch.tensor([1 if err is not None else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
        if int(flag.item()):
            if err is not None:
                raise err
            raise StedmHipError(f"rank {rank} of {world}: another rank's sampling loop raised (fp16 operand overflow there); no latents gathered")
        lat = par.all_gather_samples(lat, int(global_batch), group)
    return lat


@torch.no_grad()
def images_for_saving(decoded: torch.Tensor, segmentation_nhwc: Optional[torch.Tensor] = None):
    """The array work of predict_step after decode_first_stage (modules/ldm_diffusion.py:93-99): decoded [B,3,H,W] fp32 -> uint8
    [B,H,W,3] (clip to [-1,1], scale, truncate), segmentation [B,H,W,ncls] -> uint8 class map. Returned on the device; PNG
    encoding stays with the caller."""
    img = None if decoded is None else ops.image_to_uint8(decoded.float().contiguous())       # None: the caller has the uint8 image already
    seg = None if segmentation_nhwc is None else ops.argmax_u8(segmentation_nhwc.float().contiguous())
    return img, seg
