"""Learning-rate schedules: the factor the base learning rate is multiplied with at optimiser step t.

Pure Python, fp64, no torch: the model evaluates `factor(t)` once per optimiser step on the host and writes the product into the
device scalars its optimiser kernel reads, so a captured graph picks up each step's value.
"""
import math

KINDS = ('constant', 'cosine', 'step')


class LrSchedule:
    """factor(t) for t = 1, 2, ...: the optimiser step, i.e. the model's `iterations` after its increment.

    Warm-up, t <= W:   s + (1 - s) * t / W                       (W = warmup_steps, s = warmup_start_factor)
    afterwards, by kind:
      'constant'       1
      'cosine'         f + (1 - f) * 0.5 * (1 + cos(pi * q)),  q = clamp((t - W) / (T - W), 0, 1); holds at f after T
                       (T = total_steps, required, > W; f = final_factor)
      'step'           gamma ** (number of milestones <= t); milestones strictly increasing
    """

    def __init__(self, kind, warmup_steps=0, warmup_start_factor=0.0, total_steps=None, final_factor=0.01, milestones=(), gamma=0.1):
        if kind not in KINDS:
            raise ValueError('LrSchedule: kind must be one of {}, got {!r}'.format(', '.join(KINDS), kind))
        if isinstance(warmup_steps, bool) or int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError('LrSchedule: warmup_steps must be an integer >= 0, got {!r}'.format(warmup_steps))
        s = float(warmup_start_factor)
        if not 0.0 <= s <= 1.0:
            raise ValueError('LrSchedule: warmup_start_factor must be in [0, 1], got {!r}'.format(warmup_start_factor))
        self.kind = kind
        self.warmup_steps = int(warmup_steps)
        self.warmup_start_factor = s
        self.total_steps = None
        self.final_factor = float(final_factor)
        self.milestones = tuple(int(m) for m in milestones)
        self.gamma = float(gamma)
        if kind == 'cosine':
            if total_steps is None or isinstance(total_steps, bool) or int(total_steps) != total_steps:
                raise ValueError("LrSchedule: 'cosine' needs an integer total_steps, got {!r}".format(total_steps))
            if total_steps <= self.warmup_steps:
                raise ValueError('LrSchedule: total_steps ({}) must exceed warmup_steps ({})'.format(total_steps, self.warmup_steps))
            if not 0.0 <= self.final_factor <= 1.0:
                raise ValueError('LrSchedule: final_factor must be in [0, 1], got {!r}'.format(final_factor))
            self.total_steps = int(total_steps)
        if kind == 'step':
            if any(int(m) != m or m < 1 for m in milestones):
                raise ValueError('LrSchedule: milestones must be integers >= 1, got {!r}'.format(tuple(milestones)))
            if any(b <= a for a, b in zip(self.milestones, self.milestones[1:])):
                raise ValueError('LrSchedule: milestones must be strictly increasing, got {!r}'.format(self.milestones))
            if not (math.isfinite(self.gamma) and self.gamma > 0.0):
                raise ValueError('LrSchedule: gamma must be finite and > 0, got {!r}'.format(gamma))

    def factor(self, t):
        if isinstance(t, bool) or int(t) != t or t < 1:
            raise ValueError('LrSchedule.factor: t is the optimiser step 1, 2, ..., got {!r}'.format(t))
        t = int(t)
        W = self.warmup_steps
        if t <= W:
            s = self.warmup_start_factor
            return s + (1.0 - s) * t / W
        if self.kind == 'cosine':
            f = self.final_factor
            q = min(max((t - W) / (self.total_steps - W), 0.0), 1.0)
            return f + (1.0 - f) * 0.5 * (1.0 + math.cos(math.pi * q))
        if self.kind == 'step':
            return self.gamma ** sum(1 for m in self.milestones if m <= t)
        return 1.0
