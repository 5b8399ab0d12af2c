"""The posterior of the KL first stage: `ldm.modules.distributions.distributions.DiagonalGaussianDistribution` (distributions.py:24-62) with
the reference's attributes and methods. `sample` on GPU tensors is one HIP kernel (stedm_gauss_sample: clamp, exp, noise and — for
LatentDiffusion.get_first_stage_encoding — the scale factor in one pass, the noise given or drawn in the kernel from the per-sample
Philox streams); `kl` and `nll` are on no path LatentDiffusion takes and stay plain torch expressions over the device tensors."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops


class DiagonalGaussianDistribution(object):
    """distributions.py:24-62. `parameters` [B, 2C, H, W]: the mean and the log-variance stacked along the channels."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean).to(device=self.parameters.device)

    def sample(self, noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, sample_id0: int = 0, scale: float = 1.0):
        """mean + std * noise (distributions.py:35-37), times `scale` (get_first_stage_encoding's scale_factor, ddpm.py:552; 1 here).
        GPU tensors: the kernel. noise [B, C, H, W] is used when given; otherwise sample b is drawn in the kernel from
        (seed, global sample id sample_id0 + b) — row sample_id0 + b of ops.philox_normal(seed, stream STREAM_POSTERIOR) — so a sample's
        latent does not depend on the batch or shard it is encoded in; without a seed one is drawn per call from torch's CPU generator
        (torch.manual_seed reproduces the run), as the samplers do. CPU tensors: `noise` or torch.randn in torch; a seed is refused there,
        since the host cannot reproduce the device's bits."""
        p = self.parameters
        if not p.is_cuda:
            if seed is not None:
                raise ValueError("DiagonalGaussianDistribution.sample(seed=...) draws in the HIP kernel; CPU tensors take `noise` (or torch's "
                                 "generator), which would give other bits than the device's")
            n = torch.randn(self.mean.shape).to(device=p.device) if noise is None else noise
            x = self.mean + self.std * n
            return x if scale == 1.0 else scale * x
        m = p.detach().float().contiguous()
        if self.deterministic:                        # std is 0: the kernel's mode flag, scale * mean with no noise read or drawn
            return ops.gauss_sample(m, scale=float(scale), mode=True)
        if noise is not None:
            return ops.gauss_sample(m, noise.detach().float().contiguous(), scale=float(scale))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        return ops.gauss_sample(m, None, scale=float(scale), seed=int(seed), first_id=int(sample_id0))

    def kl(self, other=None):
        """distributions.py:39-51."""
        if self.deterministic:
            return torch.Tensor([0.])
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar + other.logvar,
                               dim=[1, 2, 3])

    def nll(self, sample, dims=[1, 2, 3]):
        """distributions.py:53-59."""
        if self.deterministic:
            return torch.Tensor([0.])
        logtwopi = float(np.log(2.0 * np.pi))
        return 0.5 * torch.sum(logtwopi + self.logvar + torch.pow(sample - self.mean, 2) / self.var, dim=dims)

    def mode(self):
        """distributions.py:61-62."""
        return self.mean
