"""Learning-rate schedule of the large-batch recipe: linear warm-up, then polynomial decay.

Host-side and stateless -- the rate is a pure function of the global step, so resuming a run needs
nothing in the checkpoint beyond the step it restarts at.
"""
from __future__ import annotations


class WarmupPolyLR:
    """``lr_at(step)`` for ``step = 0, 1, ...`` (the step about to run):

    * warm-up, ``step < warmup_steps``: ``base_lr * (step + 1) / warmup_steps`` -- linear from
      ``base_lr / warmup_steps`` up to ``base_lr`` at the last warm-up step;
    * decay: ``end_lr + (base_lr - end_lr) * (1 - t) ** power`` with
      ``t = (step - warmup_steps) / (total_steps - warmup_steps)`` clamped to [0, 1], so the first
      decay step still runs at ``base_lr`` and every step from ``total_steps`` on at ``end_lr``.

    ``set(step)`` writes the rate into every param group.  Call it BEFORE the forward of the step:
    an optimizer whose update runs per bucket inside backward is armed with the hyperparameters it
    has at forward time, and changing ``lr`` between backward and ``step()`` is a contract
    violation that raises.
    """

    def __init__(self, optimizer, base_lr: float, warmup_steps: int, total_steps: int, power: float = 2.0,
                 end_lr: float = 0.0):
        if warmup_steps < 0 or total_steps < 1 or warmup_steps > total_steps:
            raise ValueError(f"need 0 <= warmup_steps <= total_steps and total_steps >= 1, got "
                             f"{warmup_steps}, {total_steps}")
        self.optimizer = optimizer
        self.base_lr, self.end_lr = float(base_lr), float(end_lr)
        self.warmup_steps, self.total_steps = int(warmup_steps), int(total_steps)
        self.power = float(power)

    def lr_at(self, step: int) -> float:
        if step < self.warmup_steps:
            return self.base_lr * (max(step, 0) + 1) / self.warmup_steps
        span = self.total_steps - self.warmup_steps
        t = 1.0 if span <= 0 else min(max((step - self.warmup_steps) / span, 0.0), 1.0)
        return self.end_lr + (self.base_lr - self.end_lr) * (1.0 - t) ** self.power

    def set(self, step: int) -> float:
        lr = self.lr_at(step)
        if self.optimizer is not None:
            for group in self.optimizer.param_groups:
                group["lr"] = lr
        return lr
