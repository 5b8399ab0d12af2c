"""DPM-Solver++(2M) sampler, HIP-backed.

Mirrors `ldm.models.diffusion.dpm_solver.sampler.DPMSolverSampler` (reference sampler.py:12-95): same constructor and `sample`
surface, the same solver — multistep DPM-Solver++ of order 2 (predict_x0=True, solver_type 'dpm_solver', thresholding off),
skip_type 'time_uniform', lower_order_final=True (sampler.py:82-93) — and exactly S model evaluations for S steps.

Step i evaluates the model at t_i and moves x from t_i to t_{i+1} (i = 0 .. S-1, the shape of the reference's loop,
dpm_solver.py:1053-1083). The host builds every per-step scalar once (`dpm_tables`, the reference's fp32 arithmetic restated with torch
CPU ops in its order); every tensor operation of a step runs in HIP kernels:
  * the model call at the fractional model time t_input = (t - 1/N) * 1000 (dpm_solver.py:246-253) -> the U-Net with float32
    timesteps (stedm_time_embed_f32), one shared-encoder CFG pass (`apply_model_cfg`) when the model offers it;
  * CFG combine, data prediction and the multistep update -> one fused kernel (stedm_dpm_step);
  * with `use_graph=True` the whole step (model time from the device table, U-Net, update, step counter) is captured once in a
    hipGraph and replayed for the remaining steps.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import torch

from . import ops

MODEL_TYPES = {"eps": "noise"}      # sampler.py:7-10 ('v' is not a parameterization of the STEDM configs)


@dataclass
class DPMTables:
    """Host tables of one S-step run. t_cont: fp32 [S+1] continuous times, 1 -> 1/N (get_time_steps 'time_uniform'); t_input: fp32 [S]
    model times of the S evaluations; coefs: fp32 [S, ops.DPM_NCOEF] rows {alpha_i, sigma_i, r, A, inv_r0, 0.5 A} of stedm_dpm_step;
    orders: the solver order of every step."""
    t_cont: torch.Tensor
    t_input: torch.Tensor
    coefs: torch.Tensor
    orders: List[int]


class _VPSchedule:
    """NoiseScheduleVP('discrete', alphas_cumprod=...) (dpm_solver.py:7-132) on fp32 CPU tensors: log(alpha_t) is the piecewise-linear
    interpolation of 0.5 log(alphas_cumprod) over the keypoints t_n = (n + 1) / N, extended linearly beyond the ends."""

    def __init__(self, alphas_cumprod):
        ac = torch.as_tensor(alphas_cumprod).detach().to("cpu", torch.float32)
        self.log_alpha = 0.5 * torch.log(ac)
        self.N = int(ac.shape[0])
        self.t_keys = torch.linspace(0., 1., self.N + 1)[1:]

    def log_mean_coeff(self, t: torch.Tensor) -> torch.Tensor:
        # segment j holds t: the last keypoint strictly below t, clamped to the first / last segment (the reference's sort-based search
        # places t ahead of an equal keypoint); then y_j + (t - x_j) (y_{j+1} - y_j) / (x_{j+1} - x_j), in that order
        xp, yp = self.t_keys, self.log_alpha
        j = (xp[None, :] < t[:, None]).sum(1) - 1
        j = j.clamp(0, self.N - 2)
        x0, x1, y0, y1 = xp[j], xp[j + 1], yp[j], yp[j + 1]
        return y0 + (t - x0) * (y1 - y0) / (x1 - x0)

    def alpha(self, t):
        return torch.exp(self.log_mean_coeff(t))

    def std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.log_mean_coeff(t)))

    def lam(self, t):
        lmc = self.log_mean_coeff(t)
        return lmc - 0.5 * torch.log(1. - torch.exp(2. * lmc))


def dpm_tables(alphas_cumprod, S: int, lower_order_final: bool = True) -> DPMTables:
    """Every per-step scalar of DPM_Solver.sample(steps=S, skip_type='time_uniform', method='multistep', order=2, lower_order_final)
    for a discrete-time model with these alphas_cumprod. Each scalar is one-element fp32 torch arithmetic in the reference's order:
    first-order rows (step 0; the last step when S < 15) follow dpm_solver_first_update (A = alpha_t expm1(-h)), second-order rows
    multistep_dpm_solver_second_update (A = alpha_t (exp(-h) - 1), inv_r0 = 1 / (h_0 / h))."""
    S = int(S)
    if S < 2:
        raise ValueError(f"DPM-Solver++(2M) needs S >= 2 steps (the reference asserts steps >= order), got {S}")
    ns = _VPSchedule(alphas_cumprod)
    t_cont = torch.linspace(1., 1. / ns.N, S + 1)
    t_input = ((t_cont[:S] - 1. / ns.N) * 1000.).contiguous()
    rows, orders = [], []
    one = lambda i: t_cont[i:i + 1]
    for i in range(S):
        s, t = one(i), one(i + 1)
        order = 1 if i == 0 or (lower_order_final and S < 15 and i == S - 1) else 2
        alpha_s, sigma_s = ns.alpha(s), ns.std(s)
        sigma_t, alpha_t = ns.std(t), torch.exp(ns.log_mean_coeff(t))
        if order == 1:
            h = ns.lam(t) - ns.lam(s)
            A = alpha_t * torch.expm1(-h)
            inv_r0 = torch.zeros_like(A)
            half_A = torch.zeros_like(A)
        else:
            l1, l0, lt = ns.lam(one(i - 1)), ns.lam(s), ns.lam(t)
            h_0 = l0 - l1
            h = lt - l0
            inv_r0 = 1. / (h_0 / h)
            A = alpha_t * (torch.exp(-h) - 1.)
            half_A = 0.5 * A
        rows.append(torch.cat([alpha_s, sigma_s, sigma_t / sigma_s, A, inv_r0, half_A]))
        orders.append(order)
    return DPMTables(t_cont=t_cont, t_input=t_input, coefs=torch.stack(rows).contiguous(), orders=orders)


class DPMSolverSampler(object):
    def __init__(self, model, device=torch.device("cuda"), **kwargs):
        """sampler.py:13-18. The run happens where the model lives (its tensors and the HIP kernels); `device` is kept for the
        reference's signature. use_graph=True: hipGraph replay of the step (DPMStepGraph)."""
        super().__init__()
        self.model = model
        self.device = device
        self.use_graph = bool(kwargs.get("use_graph", False))
        self.alphas_cumprod = model.alphas_cumprod.detach().clone().to(torch.float32)

    def make_schedule(self, S, tables=None):
        """The host tables of an S-step run (dpm_tables) and their device copies: the model times and the coefficient rows."""
        tb = dpm_tables(self.alphas_cumprod, S) if tables is None else tables
        dev = self.model.device
        self.tables = tb
        self._coefs = tb.coefs.to(dev)
        self._t_table = tb.t_input.to(dev)
        return tb

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        """sampler.py:24-95 -> (x, None). The reference accepts mask / x0 / eta / quantize_x0 / score_corrector / noise_dropout /
        temperature and ignores them; here they raise NotImplementedError, and S < 2 raises ValueError, before any device work.
        callback(i) and img_callback(pred_x0, i) are called after step i (eager loop; the reference calls neither)."""
        if mask is not None or x0 is not None or eta != 0. or quantize_x0 or score_corrector is not None or noise_dropout > 0. \
                or temperature != 1.:
            raise NotImplementedError("DPM-Solver++(2M) sampling: mask / x0 / eta / quantize_x0 / score_corrector / noise_dropout / "
                                      "temperature are not implemented (the reference's DPMSolverSampler ignores them)")
        ptype = getattr(self.model, "parameterization", "eps")
        if ptype not in MODEL_TYPES:
            raise NotImplementedError(f"DPM-Solver sampling for parameterization {ptype!r}: only 'eps' is built")
        tb = dpm_tables(self.alphas_cumprod, S)
        C, H, W = shape
        size = (batch_size, C, H, W)
        dev = self.model.device
        self.make_schedule(S, tb)
        img = torch.randn(size, device=dev) if x_T is None else x_T.to(dev).float().clone()
        cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        uncond = unconditional_conditioning if cfg else None
        scale = float(unconditional_guidance_scale)
        if self.use_graph and callback is None and img_callback is None and hasattr(self.model, "apply_model_cfg"):
            sg = DPMStepGraph(self, img, conditioning, uncond, scale)
            sg.reset(0)
            sg.step_eager()             # packs weights and allocates every buffer before capture
            if int(S) > 1:
                with sg.stream_ctx():
                    sg.capture()
                    for _ in range(1, int(S)):
                        sg.replay()
                sg.join()
        else:
            self._sample_eager(img, conditioning, uncond, scale, int(S), callback, img_callback)
        ops.f16_guard_check("the DPM-Solver sampling loop")    # fp16 modes: raise rather than return samples computed through an inf
        return img, None

    def _eps(self, x, t, cond, uncond, out=None):
        """(e_c, e_u or None) at model time t (float32 [B]); model_wrapper's classifier-free branch (dpm_solver.py:305-321)."""
        m = self.model
        if hasattr(m, "apply_model_cfg"):
            if uncond is None:
                return m.apply_model(x, t, cond, out=out, uniform_t=True), None
            return m.apply_model_cfg(x, t, cond, uncond, out=out, uniform_t=True)
        e_c = m.apply_model(x, t, cond)
        return e_c, (None if uncond is None else m.apply_model(x, t, uncond))

    def _sample_eager(self, img, cond, uncond, scale, S, callback, img_callback):
        dev = img.device
        B = img.shape[0]
        x0_prev = torch.empty_like(img)
        pred_x0 = torch.empty_like(img) if img_callback else None
        steps = torch.arange(S, dtype=torch.int32, device=dev)
        for i in range(S):
            t = torch.full((B,), float(self.tables.t_input[i]), dtype=torch.float32, device=dev)
            e_c, e_u = self._eps(img, t, cond, uncond)
            ops.dpm_step(img, e_c.float().contiguous(), None if e_u is None else e_u.float().contiguous(), x0_prev, self._coefs,
                         step_idx=steps[i:i + 1], cfg_scale=scale, pred_x0=pred_x0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)


class DPMStepGraph:
    """One DPM-Solver step = {model time from the device table (stedm_step_set_t_f32), U-Net (shared-encoder CFG pass) into a
    preallocated eps, fused update in place on `img` and x0_prev (stedm_dpm_step), step index + 1}, capturable once in a hipGraph and
    replayed for every later step (the pattern of ddim.StepGraph)."""

    def __init__(self, sampler: DPMSolverSampler, img: torch.Tensor, cond, uncond, scale: float):
        self.s = sampler
        self.img = img
        self.cond, self.uncond, self.scale = cond, uncond, float(scale)
        dev = img.device
        b = img.shape[0]
        self.step = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.t_buf = torch.empty((b,), dtype=torch.float32, device=dev)
        self.x0_prev = torch.empty_like(img)
        self.eps = torch.empty((2 * b if uncond is not None else b,) + tuple(img.shape[1:]), dtype=torch.float32, device=dev)
        self.graph = None
        self.side = None

    def reset(self, index: int):
        self.step.fill_(int(index))

    def step_eager(self):
        s = self.s
        ops.step_set_t(s._t_table, self.step, self.t_buf)
        e_c, e_u = s._eps(self.img, self.t_buf, self.cond, self.uncond, out=self.eps)
        ops.dpm_step(self.img, e_c, e_u, self.x0_prev, s._coefs, step_idx=self.step, cfg_scale=self.scale)
        ops.step_advance(self.step, 1)

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
