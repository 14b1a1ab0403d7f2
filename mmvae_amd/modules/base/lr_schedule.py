"""Learning-rate schedules (host-side scalars), in the style of annealing_fn.py.  Not in the reference, whose
`configure_optimizers` fixes lr = 5e-3 (cmmvae/models/cmmvae_model.py:299-318).

A schedule is a function of the number of training steps the model has taken: before step `t` the model sets every
optimiser's `param_groups[0]["lr"]` to `base_lr * factor(t)` and, after the step, calls `step()`.  On the engine path
the learning rate is a device word the captured programs read (HipAdam.hyper_dev), so a schedule costs one small write
per step.  `step_count` is a plain attribute: set it when resuming a run.
"""
import math


class LRScheduleFn:
    """The constant schedule: factor 1 at every step."""

    def __init__(self):
        self.step_count = 0

    def factor(self, t: int) -> float:
        """Multiplier of the base learning rate for training step `t` (0-based)."""
        return 1.0

    def step(self) -> None:
        """Once per training step, after it."""
        self.step_count += 1


class WarmupCosineLRFn(LRScheduleFn):
    """Linear warm-up over the first `warmup_steps` steps -- (t + 1) / warmup_steps, so step 0 already moves -- then half
    a cosine from 1 down to `min_factor`, reached at `total_steps` and kept from there on."""

    def __init__(self, warmup_steps: int, total_steps: int, min_factor: float = 0.0):
        super().__init__()
        # (values that arrive from YAML as strings -- `1e4` is one to PyYAML -- become numbers, as for KLAnnealingFn)
        self.warmup_steps = int(float(warmup_steps))
        self.total_steps = int(float(total_steps))
        self.min_factor = float(min_factor)

    def factor(self, t: int) -> float:
        if t < self.warmup_steps:
            return (t + 1) / self.warmup_steps
        if t >= self.total_steps:
            return self.min_factor
        progress = (t - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps)
        return self.min_factor + (1.0 - self.min_factor) * 0.5 * (1.0 + math.cos(math.pi * progress))


class StepDecayLRFn(LRScheduleFn):
    """`gamma ** (t // step_size)`: the factor drops by `gamma` every `step_size` steps."""

    def __init__(self, step_size: int, gamma: float):
        super().__init__()
        self.step_size = int(float(step_size))
        self.gamma = float(gamma)

    def factor(self, t: int) -> float:
        return self.gamma ** (t // self.step_size)
