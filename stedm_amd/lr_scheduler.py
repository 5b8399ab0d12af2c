"""Learning-rate multipliers of the reference's `scheduler_config` (ldm/lr_scheduler.py; ddpm.py:1364-1386 wraps one in
`LambdaLR(opt, lr_lambda=scheduler.schedule)` at interval "step"): f(n) for the n-th scheduler step, n = 0 for the first optimizer
step. `UNetTrainer(lr_lambda=scheduler.schedule)` runs optimizer step s with lr * f(s - 1).

Three shapes, all computed in double:
  LambdaWarmUpCosineScheduler    one linear warm-up from lr_start to lr_max over warm_up_steps, then half a cosine down to lr_min at
                                 max_decay_steps, constant afterwards
  LambdaWarmUpCosineScheduler2   the same per cycle, cycles of cycle_lengths[i] steps; a step ON a cycle's last boundary still belongs
                                 to that cycle (n <= cumulative length), and counts from that cycle's start
  LambdaLinearScheduler          per cycle: linear warm-up, then a straight line from f_max (extrapolated back to the cycle's start)
                                 to f_min at the cycle's end: f_min + (f_max - f_min) * (length - n) / length
"""
from __future__ import annotations

import math
from typing import Sequence

__all__ = ["LambdaWarmUpCosineScheduler", "LambdaWarmUpCosineScheduler2", "LambdaLinearScheduler", "SCHEDULER_TARGETS", "instantiate_from_config"]


def _warm_up(start: float, peak: float, steps, n) -> float:
    return (peak - start) / steps * n + start


def _half_cosine(low: float, high: float, t: float) -> float:
    return low + 0.5 * (high - low) * (1 + math.cos(min(t, 1.0) * math.pi))


class LambdaWarmUpCosineScheduler:
    """use with a base learning rate of 1.0 when lr_max is the rate itself (the multiplier is returned as it stands)"""

    def __init__(self, warm_up_steps, lr_min, lr_max, lr_start, max_decay_steps, verbosity_interval=0):
        self.lr_warm_up_steps = warm_up_steps
        self.lr_start, self.lr_min, self.lr_max = lr_start, lr_min, lr_max
        self.lr_max_decay_steps = max_decay_steps
        self.verbosity_interval = verbosity_interval
        self.last_lr = 0.

    def schedule(self, n, **kwargs) -> float:
        if self.verbosity_interval > 0 and n % self.verbosity_interval == 0:
            print(f"current step: {n}, recent lr-multiplier: {self.last_lr}")
        if n < self.lr_warm_up_steps:
            lr = _warm_up(self.lr_start, self.lr_max, self.lr_warm_up_steps, n)
        else:
            lr = _half_cosine(self.lr_min, self.lr_max, (n - self.lr_warm_up_steps) / (self.lr_max_decay_steps - self.lr_warm_up_steps))
        self.last_lr = lr
        return lr

    def __call__(self, n, **kwargs) -> float:
        return self.schedule(n, **kwargs)


class LambdaWarmUpCosineScheduler2:
    """repeated cycles, every argument a list with one entry per cycle"""

    def __init__(self, warm_up_steps: Sequence, f_min: Sequence, f_max: Sequence, f_start: Sequence, cycle_lengths: Sequence, verbosity_interval=0):
        if not (len(warm_up_steps) == len(f_min) == len(f_max) == len(f_start) == len(cycle_lengths)):
            raise ValueError("warm_up_steps, f_min, f_max, f_start and cycle_lengths need one entry per cycle each")
        self.lr_warm_up_steps = list(warm_up_steps)
        self.f_start, self.f_min, self.f_max = list(f_start), list(f_min), list(f_max)
        self.cycle_lengths = list(cycle_lengths)
        self.cum_cycles = [0]
        for length in self.cycle_lengths:
            self.cum_cycles.append(self.cum_cycles[-1] + length)
        self.verbosity_interval = verbosity_interval
        self.last_f = 0.

    def find_in_interval(self, n) -> int:
        for cycle, end in enumerate(self.cum_cycles[1:]):
            if n <= end:
                return cycle
        raise ValueError(f"step {n} lies past the last cycle (the cycles cover {self.cum_cycles[-1]} steps): make the last cycle as long as the run")

    def _locate(self, n):
        cycle = self.find_in_interval(n)
        n = n - self.cum_cycles[cycle]
        if self.verbosity_interval > 0 and n % self.verbosity_interval == 0:
            print(f"current step: {n}, recent lr-multiplier: {self.last_f}, current cycle {cycle}")
        return cycle, n

    def _decay(self, cycle: int, n) -> float:
        warm, length = self.lr_warm_up_steps[cycle], self.cycle_lengths[cycle]
        return _half_cosine(self.f_min[cycle], self.f_max[cycle], (n - warm) / (length - warm))

    def schedule(self, n, **kwargs) -> float:
        cycle, n = self._locate(n)
        if n < self.lr_warm_up_steps[cycle]:
            f = _warm_up(self.f_start[cycle], self.f_max[cycle], self.lr_warm_up_steps[cycle], n)
        else:
            f = self._decay(cycle, n)
        self.last_f = f
        return f

    def __call__(self, n, **kwargs) -> float:
        return self.schedule(n, **kwargs)


class LambdaLinearScheduler(LambdaWarmUpCosineScheduler2):
    def _decay(self, cycle: int, n) -> float:
        length = self.cycle_lengths[cycle]
        return self.f_min[cycle] + (self.f_max[cycle] - self.f_min[cycle]) * (length - n) / length


SCHEDULER_TARGETS = {f"{mod}.{cls.__name__}": cls for cls in (LambdaWarmUpCosineScheduler, LambdaWarmUpCosineScheduler2, LambdaLinearScheduler)
                     for mod in ("ldm.lr_scheduler", "stedm_amd.lr_scheduler")}


def instantiate_from_config(config):
    """`scheduler_config` {target, params} -> one of the three schedulers; a config without `target`, or with any other target, raises (a
    config entry is instantiated or refused, never dropped)."""
    if not hasattr(config, "get") or config.get("target") is None:
        raise KeyError("scheduler_config: expected key `target` to instantiate.")
    cls = SCHEDULER_TARGETS.get(config["target"])
    if cls is None:
        raise NotImplementedError(f"scheduler_config target {config['target']!r}: the learning-rate schedulers provided are "
                                  f"{sorted(t for t in SCHEDULER_TARGETS if t.startswith('ldm.'))}")
    return cls(**dict(config.get("params") or {}))
