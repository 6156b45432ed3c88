"""Learning-rate schedule and global-norm clipping shared by the two optimisation paths.

ONE formula (stated in ``include/morec_hip.h`` at ``morec_lr_schedule``): ``morec_step_decide_ex`` evaluates it on the device from the
applied-step count of the step block (``--fused_step``); ``lr_multiplier`` below is its host form, which the autograd paths hand to
``torch.optim.lr_scheduler.LambdaLR``.  ``t`` is the 0-based index of the optimizer step (= steps applied before it), as LambdaLR counts.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

KINDS = {"constant": 0, "linear": 1, "cosine": 2}


def lr_multiplier(t: int, kind: str, warmup_steps: int, total_steps: int, min_ratio: float) -> float:
    if t < warmup_steps:
        return t / warmup_steps
    if kind == "constant":
        return 1.0
    q = min(1.0, (t - warmup_steps) / max(1, total_steps - warmup_steps))
    shape = 0.5 * (1.0 + math.cos(math.pi * q)) if kind == "cosine" else 1.0 - q
    return min_ratio + (1.0 - min_ratio) * shape


@dataclass(frozen=True)
class LrSchedule:
    kind: str = "constant"
    warmup_steps: int = 0
    total_steps: int = 0
    min_ratio: float = 0.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"lr schedule kind {self.kind!r}: one of {sorted(KINDS)}")
        if self.warmup_steps < 0 or not 0.0 <= self.min_ratio <= 1.0:
            raise ValueError(f"lr schedule: warmup_steps {self.warmup_steps} (>= 0), min_ratio {self.min_ratio} (in [0, 1])")
        if self.kind != "constant" and self.total_steps < self.warmup_steps:
            raise ValueError(f"lr schedule: total_steps {self.total_steps} < warmup_steps {self.warmup_steps}")

    def multiplier(self, t: int) -> float:
        return lr_multiplier(int(t), self.kind, self.warmup_steps, self.total_steps, self.min_ratio)

    def c_struct(self):
        from . import _lib
        return _lib.LrSchedule(KINDS[self.kind], int(self.warmup_steps), int(self.total_steps), float(self.min_ratio))

    @staticmethod
    def coerce(x):
        """None | LrSchedule | dict(kind=, warmup_steps=, total_steps=, min_ratio=) -> LrSchedule or None."""
        if x is None or isinstance(x, LrSchedule):
            return x
        return LrSchedule(**dict(x))


def schedule_from_args(args, total_steps: int):
    """The schedule the command line asks for, or None when it asks for none (constant, no warmup: every multiplier is 1)."""
    kind = getattr(args, "lr_schedule", "constant")
    warm = int(getattr(args, "warmup_steps", 0))
    if kind == "constant" and warm == 0:
        return None
    return LrSchedule(kind, warm, int(total_steps), float(getattr(args, "min_lr_ratio", 0.0)))


def make_lambda_lr(optimizer, schedule):
    """``LambdaLR`` over every parameter group with the one multiplier (None: no scheduler)."""
    if schedule is None:
        return None
    from torch.optim.lr_scheduler import LambdaLR
    return LambdaLR(optimizer, lr_lambda=schedule.multiplier)


class AutogradStepControl:
    """Clip + schedule for a ``torch.optim.AdamW`` (+ ``GradScaler``) loop: ``step()`` stands where ``scaler.step(optimizer);
    scaler.update()`` (or ``optimizer.step()``) stood.  With ``max_grad_norm`` 0 and no schedule it does exactly what stood there."""

    def __init__(self, optimizer, scaler=None, max_grad_norm: float = 0.0, lr_schedule=None):
        self.optimizer, self.scaler = optimizer, scaler
        self.max_grad_norm = float(max_grad_norm)
        self.schedule = LrSchedule.coerce(lr_schedule)
        self.scheduler = make_lambda_lr(optimizer, self.schedule)
        self.last_norm = None          # tensor (no host read here: the logging site reads it where it synchronises anyway)
        self._applied = 0              # optimizer.step() calls that really ran (GradScaler.step leaves it out after an overflow)
        if self.scheduler is not None and scaler is not None:
            optimizer.register_step_post_hook(self._count)

    def _count(self, *_):
        self._applied += 1

    def _params(self):
        return [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]

    def step(self):
        import torch
        opt, sc = self.optimizer, self.scaler
        if self.max_grad_norm > 0.0:
            if sc is not None:
                sc.unscale_(opt)
            self.last_norm = torch.nn.utils.clip_grad_norm_(self._params(), self.max_grad_norm)
        if sc is not None:
            before = self._applied
            sc.step(opt)
            sc.update()
            applied = self._applied != before      # (only counted, and only read, when a scheduler has to know)
        else:
            opt.step()
            applied = True
        if self.scheduler is not None and applied:      # a step GradScaler skipped does not advance the schedule
            self.scheduler.step()

    def lr_mult(self) -> float:
        return 1.0 if self.scheduler is None else self.schedule.multiplier(self.scheduler.last_epoch)

    def resume_from_optimizer(self):
        """After ``optimizer.load_state_dict``: AdamW's per-parameter ``step`` counts the applied steps, which is all the schedule depends on."""
        if self.scheduler is None:
            return
        steps = [int(float(st["step"])) for st in self.optimizer.state.values() if "step" in st]
        if not steps:
            return
        self.scheduler.last_epoch = max(steps)
        mult = self.schedule.multiplier(self.scheduler.last_epoch)
        for g, base in zip(self.optimizer.param_groups, self.scheduler.base_lrs):
            g["lr"] = base * mult
