"""Step cache of the denoise loop: on some sampler steps the DiT's block stack is not run; its effect on the residual stream is forecast
from what it did on the steps that were run (WanTI2V.denoise(step_cache=), README).

`StepCache` is the POLICY - which steps are computed - as an immutable host object; `plan` is pure Python in float64 and decides
everything before the first step, so the loop never reads the device. Three rules: `interval=` (the `cal_type` counter of the reference's
TaylorSeer for BAGEL, models/BAGEL/modeling/cache_utils/taylorseer.py), `schedule=` (explicit) and `rel_l1_thresh=` (TeaCache's
accumulated relative-L1 distance of the time embedding; its distances come from the device ONCE, before the loop).

`StepCacheState` owns the device buffers of one stacked forward (the residual r = x_out - x_in and its backward differences d0, d1, d2,
the copy of x_in, the 4-float control table the kernels read) and the two host counters (`have`, `last`). The arithmetic is
include/univid_hip.h: uv_step_cache_update / uv_step_cache_apply. The cache spans the WHOLE block stack, not every module as the
reference's does: at TI2V-5B size the per-module form would hold 60 times the memory.
"""
import math

import torch

ORDERS = (0, 1, 2)
INDICATORS = ("e0", "e")


class StepCache:
    """StepCache(order=1, *, interval=None | schedule=None | rel_l1_thresh=None, coefficients=(1.0, 0.0), indicator="e0",
    first_steps=None, last_steps=1): exactly one of the three rules.

    order: 0 reuses the last residual, 1 / 2 extrapolate it with first / second backward differences.
    Always computed: step 0, steps < first_steps, steps >= n_steps - last_steps, the steps `plan` is told are forced.
    interval=k (k >= 2): after a computed step k - 1 steps are skipped (first_steps defaults to 5, the reference's first_enhance).
    schedule: n_steps bools, True = computed, OR-ed with the rules above.
    rel_l1_thresh: on a free step acc += polyval(coefficients, distances[i]); the step is skipped iff acc < rel_l1_thresh, otherwise it
        is computed; every computed step resets acc to 0 (a NaN / inf distance computes the step). first_steps defaults to 1.
        coefficients: highest power first (numpy.polyval); the default is the identity - calibrated polynomials belong to trained
        checkpoints and are the caller's to pass. indicator: "e0" (the [6C] modulation rows) or "e" (the [C] rows) of WanModel._time_rows.
    """
    __slots__ = ("order", "interval", "schedule", "rel_l1_thresh", "coefficients", "indicator", "first_steps", "last_steps")

    def __init__(self, order=1, *, interval=None, schedule=None, rel_l1_thresh=None, coefficients=(1.0, 0.0), indicator="e0", first_steps=None,
                 last_steps=1):
        if isinstance(order, bool) or order not in ORDERS:
            raise ValueError(f"StepCache: order must be one of {ORDERS}, got {order!r}")
        given = [n for n, v in (("interval", interval), ("schedule", schedule), ("rel_l1_thresh", rel_l1_thresh)) if v is not None]
        if len(given) != 1:
            raise ValueError(f"StepCache: exactly one of interval=, schedule= and rel_l1_thresh= is expected, got {given or 'none'}")
        if interval is not None:
            if isinstance(interval, bool) or int(interval) != interval or interval < 2:
                raise ValueError(f"StepCache: interval must be an integer >= 2, got {interval!r}")
            interval = int(interval)
        if schedule is not None:
            schedule = tuple(bool(s) for s in schedule)
        if rel_l1_thresh is not None:
            rel_l1_thresh = float(rel_l1_thresh)
            if math.isnan(rel_l1_thresh) or rel_l1_thresh < 0.0:
                raise ValueError(f"StepCache: rel_l1_thresh must be >= 0, got {rel_l1_thresh!r}")
        coefficients = tuple(float(c) for c in coefficients)
        if not coefficients or not all(math.isfinite(c) for c in coefficients):
            raise ValueError(f"StepCache: coefficients must be a non-empty sequence of finite numbers, got {coefficients!r}")
        if indicator not in INDICATORS:
            raise ValueError(f"StepCache: indicator must be one of {INDICATORS}, got {indicator!r}")
        if first_steps is None:
            first_steps = 5 if interval is not None else 1
        for name, v in (("first_steps", first_steps), ("last_steps", last_steps)):
            if isinstance(v, bool) or int(v) != v or v < 0:
                raise ValueError(f"StepCache: {name} must be an integer >= 0, got {v!r}")
        for name, v in (("order", int(order)), ("interval", interval), ("schedule", schedule), ("rel_l1_thresh", rel_l1_thresh),
                        ("coefficients", coefficients), ("indicator", indicator), ("first_steps", int(first_steps)), ("last_steps", int(last_steps))):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("StepCache is immutable: build a new one")

    def __delattr__(self, name):
        raise AttributeError("StepCache is immutable: build a new one")

    def _key(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, StepCache) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        rule = ("interval", "schedule", "rel_l1_thresh")
        shown = [f"{n}={getattr(self, n)!r}" for n in self.__slots__[1:] if n not in rule or getattr(self, n) is not None]
        return f"StepCache({self.order}, {', '.join(shown)})"

    @property
    def needs_distances(self):
        """True for the rel_l1_thresh rule: `plan` wants the indicator distances."""
        return self.rel_l1_thresh is not None

    def plan(self, n_steps, distances=None, forced=()):
        """Tuple of n_steps bools, True = the step is computed. distances (rel_l1_thresh only): n_steps numbers, distances[i] for i >= 1 =
        relative L1 distance between the time-embedding rows of steps i and i - 1 (distances[0] is not read). forced: step indices that
        are computed whatever the rule says."""
        n = int(n_steps)
        if n < 0:
            raise ValueError(f"StepCache.plan: n_steps must be >= 0, got {n_steps!r}")
        if self.schedule is not None and len(self.schedule) != n:
            raise ValueError(f"StepCache.plan: the schedule has {len(self.schedule)} entries, the loop has {n} steps")
        if self.needs_distances:
            if distances is None:
                raise ValueError("StepCache.plan: the rel_l1_thresh rule needs distances=")
            distances = [float(d) for d in distances]
            if len(distances) != n:
                raise ValueError(f"StepCache.plan: {len(distances)} distances for {n} steps (distances[0] is a placeholder)")
        forced = frozenset(int(i) for i in forced)
        out = []
        counter, acc = 0, 0.0
        for i in range(n):
            compute = i == 0 or i < self.first_steps or i >= n - self.last_steps or i in forced
            if not compute:
                if self.interval is not None:
                    compute = counter == self.interval - 1
                elif self.schedule is not None:
                    compute = self.schedule[i]
                else:
                    p = 0.0
                    for c in self.coefficients:      # Horner, float64
                        p = p * distances[i] + c
                    acc += p
                    compute = not acc < self.rel_l1_thresh
            if compute:
                counter, acc = 0, 0.0
            else:
                counter += 1
            out.append(bool(compute))
        return tuple(out)


class StepCacheState:
    """The buffers and counters of one stacked forward under a step cache. The loop calls `reset()` at the start of a denoise and
    `advance(i, compute)` before the forward of step i (it writes the control table the kernels read - `have`, k, c1, c2 - as kernel
    arguments of four fills: no host buffer to race with a loop that runs ahead of the GPU); WanModel.forward(step_cache=(state,
    "compute" | "skip")) then saves x_in and launches the update, or launches the apply instead of the blocks."""

    def __init__(self, order):
        if isinstance(order, bool) or order not in ORDERS:
            raise ValueError(f"StepCacheState: order must be one of {ORDERS}, got {order!r}")
        self.order = int(order)
        self.key = None
        self.d = [None, None, None]     # d0, d1, d2: only d0 .. d[order] exist
        self.x_in = None
        self.ctl = None
        self.have, self.last = 0, None

    def reset(self):
        self.have, self.last = 0, None

    def _geometry(self, rows, C, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:      # "cuda" and "cuda:0" are one geometry: the loop and the forward must meet
            device = torch.device("cuda", torch.cuda.current_device())
        return (int(rows), int(C), self.order, device)

    def holds(self, rows, C, device):
        """True when the buffers exist for an fp32 stream [rows, C] on `device`."""
        return self.key is not None and self.key == self._geometry(rows, C, device)

    def buffers(self, rows, C, device):
        """The buffers for an fp32 stream [rows, C] on `device`, allocated once per (rows, C, order, device) by the LOOP before its first
        step - the forward only checks (`holds`), so nothing is ever allocated inside a capture. A new geometry resets the counters."""
        key = self._geometry(rows, C, device)
        if self.key != key:
            with torch.inference_mode(False):
                self.d = [torch.zeros(rows, C, dtype=torch.float32, device=device) if j <= self.order else None for j in range(3)]
                self.x_in = torch.zeros(rows, C, dtype=torch.float32, device=device)
                self.ctl = torch.zeros(4, dtype=torch.float32, device=device)
            self.key = key
            self.reset()
        return self

    def advance(self, i, compute):
        """Host side of step i, before its forward: the control table for the kernels of this step, then the counters as they stand after it."""
        if self.ctl is None:
            raise RuntimeError("StepCacheState.advance: no buffers yet (StepCacheState.buffers)")
        i = int(i)
        self.ctl[0:1].fill_(float(self.have))
        if compute:
            if self.have:
                self.ctl[1:2].fill_(float(i - self.last))
            self.have, self.last = min(self.have + 1, self.order + 1), i
            return
        if not self.have:
            raise RuntimeError(f"StepCacheState.advance: step {i} cannot be skipped, no step was computed yet")
        m = i - self.last
        if self.have >= 2:
            self.ctl[2:3].fill_(float(m))
        if self.have >= 3:
            self.ctl[3:4].fill_(m * m / 2)
