"""The Dormand-Prince 5(4) stepper of csrc/ode.hip restated in plain Python and fp64: the specification the step
kernels (sbi_amd_dopri5_init / _stage / _finish) and the host loop of samplers/ode_solvers/dopri5.py are held to.

* the tableau as exact fractions;
* ``Controller``: the 32-slot state block of include/sbi_amd_fmpe.h with Python floats (doubles);
* ``stage_ref`` / ``ratio_ref``: the two array operations in fp64 torch, with forward-error bounds for an fp32
  evaluation that are DERIVED from its operation count (never fitted to a kernel's output);
* ``drive``: a whole solve that takes every decision from ``Controller``;
* ``stage_fp32`` / ``ratio_fp32``: the kernels' own operation order in numpy fp32 (the bounds are conditions this plain
  restatement meets by itself, tests/test_ode_restatement_cpu.py);
* the synthetic inputs tests/test_ode_step_gpu.py feeds the kernels (shared with the CPU check of the bounds).
"""

from __future__ import annotations

import math
from fractions import Fraction as Fr

import numpy as np
import torch

# ---- Butcher tableau (Dormand & Prince 1980), exact ---------------------------------------------------------------
C = (Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1))
A = (
    (),
    (Fr(1, 5),),
    (Fr(3, 40), Fr(9, 40)),
    (Fr(44, 45), Fr(-56, 15), Fr(32, 9)),
    (Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)),
    (Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)),
    (Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)),
)
B5 = (Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84), Fr(0))
B4 = (Fr(5179, 57600), Fr(0), Fr(7571, 16695), Fr(393, 640), Fr(-92097, 339200), Fr(187, 2100), Fr(1, 40))
E = tuple(b5 - b4 for b5, b4 in zip(B5, B4))

STATE_FLOATS = 32
# fp32 slots of the state block (slots 0..15 are the eight doubles t, h, t_end, direction, atol, rtol, tiny, step)
SLOT_HS, SLOT_STAGE_T, SLOT_T, SLOT_FIN, SLOT_ACC, SLOT_REJ, SLOT_RATIO, SLOT_LAST = 16, 17, 23, 24, 25, 26, 27, 28

# an fp32 evaluation does at most 14 roundings on the way to one output element (coefficient, <= 6 multiply-adds --
# 12 roundings without fma contraction, 6 with -- the product with h, the final add or divide); 16 leaves room for the
# second-order terms of (1 + u)^14
GAMMA = 16 * 2.0**-24


class Controller:
    """The state block and its three transitions, in doubles.  ``control`` takes the error ratio as an argument: the
    arithmetic that produces it is ``ratio_ref``'s business."""

    def init(self, t0: float, t1: float, first_step: float, atol: float, rtol: float) -> "Controller":
        span = abs(t1 - t0)
        self.t, self.t_end = float(t0), float(t1)
        self.h = min(float(first_step), span)
        self.direction = 1.0 if t1 >= t0 else -1.0
        self.atol, self.rtol = float(atol), float(rtol)
        self.tiny = 1e-12 * max(span, 1.0)
        self.hs = 0.0
        self.accepted = self.rejected = 0
        self.ratio = 0.0
        self.set_step()
        return self

    def set_step(self) -> None:
        remaining = abs(self.t_end - self.t)
        hh = min(self.h, remaining)          # 0 once t has reached t_end
        self.hs = self.direction * hh        # the step t advances by (a double)
        self.stage_t = [self.t + self.hs * float(c) for c in C[1:]]      # times of stages 2..7
        self.finished = remaining <= self.tiny
        self.last = remaining > self.tiny and self.h >= remaining       # this attempt reaches t_end if accepted

    def control(self, ratio: float) -> bool:
        accept = ratio <= 1.0                # NaN rejects
        hh = abs(self.hs)
        if hh > 0.0:                         # an attempt after the end is a no-op: it moves no counter
            if accept:
                self.accepted += 1
            else:
                self.rejected += 1
        if accept:
            self.t += self.hs
        if ratio != ratio:
            factor = 0.2
        elif ratio <= 0.0:
            factor = 5.0
        else:
            factor = min(5.0, max(0.2, 0.9 * ratio**-0.2))      # (inf ** -0.2 is 0.0)
        if hh > 0.0:
            self.h = hh * factor
        self.ratio = ratio
        self.set_step()
        return accept

    def doubles(self) -> list:
        """Slots 0..15 as the eight doubles they hold."""
        return [self.t, self.h, self.t_end, self.direction, self.atol, self.rtol, self.tiny, self.hs]

    def floats(self) -> list:
        """Slots 16..28, as doubles still to be rounded to fp32."""
        return [self.hs, *self.stage_t, self.t, float(self.finished), float(self.accepted), float(self.rejected),
                self.ratio, float(self.last)]

    def slots(self) -> torch.Tensor:
        """All 32 fp32 slots, as the device holds them."""
        out = torch.zeros(STATE_FLOATS, dtype=torch.float32)
        out[:16] = torch.tensor(self.doubles(), dtype=torch.float64).view(torch.float32)
        out[16:29] = torch.tensor(self.floats(), dtype=torch.float64).to(torch.float32)
        return out


# ---- the two array operations, fp64 -------------------------------------------------------------------------------
def stage_ref(y, ks, i: int, hs: float):
    """y + hs * sum_{j < i} A[i][j] k_j in fp64 (the state handed to stage i + 1), i = 1..6."""
    s = torch.zeros_like(y, dtype=torch.float64)
    for a, k in zip(A[i], ks):
        if a != 0:
            s += float(a) * k.double()
    return y.double() + float(hs) * s


def stage_bound(y, ks, i: int, hs: float):
    """Per-element forward-error bound of an fp32 evaluation of ``stage_ref``."""
    mag = torch.zeros_like(y, dtype=torch.float64)
    for a, k in zip(A[i], ks):
        if a != 0:
            mag += abs(float(a)) * k.double().abs()
    return GAMMA * (y.double().abs() + abs(float(hs)) * mag)


def _error_terms(y, y5, ks, hs: float, atol: float, rtol: float):
    s = torch.zeros_like(y, dtype=torch.float64)
    mag = torch.zeros_like(y, dtype=torch.float64)
    for e, b5, b4, k in zip(E, B5, B4, ks):
        if e != 0:
            s += float(e) * k.double()
            mag += (abs(float(b5)) + abs(float(b4))) * k.double().abs()
    sc = float(atol) + float(rtol) * torch.maximum(y.double().abs(), y5.double().abs())
    r = float(hs) * s / sc
    # (|B5| + |B4|, not |B5 - B4|: the fp32 coefficients are formed by a subtraction that cancels)
    return r, GAMMA * (abs(float(hs)) * mag / sc + r.abs())


def ratio_ref(y, y5, ks, hs: float, atol: float, rtol: float) -> float:
    """RMS over the elements of hs * sum_j (B5 - B4)_j k_j / (atol + rtol * max(|y|, |y5|)), fp64."""
    r, _ = _error_terms(y, y5, ks, hs, atol, rtol)
    return float(torch.sqrt(torch.mean(r * r)))


def ratio_bound(y, y5, ks, hs: float, atol: float, rtol: float) -> float:
    """|ratio_fp32 - ratio_ref| <= RMS of the per-element bounds (triangle inequality of the RMS norm)."""
    _, b = _error_terms(y, y5, ks, hs, atol, rtol)
    return float(torch.sqrt(torch.mean(b * b)))


# ---- a whole solve -------------------------------------------------------------------------------------------------
def drive(f, y0, t0: float, t1: float, atol: float = 1e-6, rtol: float = 1e-5, first_step: float = 0.05,
          max_steps: int = 10_000, host_order: bool = False):
    """Integrate dy/dt = f(t, y) with every decision taken by ``Controller``.  Returns (y, log); log holds one
    (ratio, accepted, t_after, h_after) per attempt.

    The arithmetic is ``stage_ref`` / ``ratio_ref`` in the state's dtype; ``host_order=True`` keeps the controller but
    does the same sums in the operation order of ``dopri5._odeint_host`` (one axpy per term), which is what bitwise
    identity with it needs."""
    ctl = Controller().init(t0, t1, first_step, atol, rtol)
    dtype = y0.dtype
    y = y0.clone()
    tt = torch.empty(1, dtype=dtype, device=y.device)

    def rhs(time: float, state):
        tt.fill_(time)
        return f(tt, state)

    log = []
    k1 = rhs(ctl.t, y)
    for _ in range(max_steps):
        if ctl.finished:
            return y, log
        hs = ctl.hs
        ks = [k1]
        for i in range(1, 7):
            if host_order:
                yi = y.clone()
                for a, k in zip(A[i], ks):
                    if a != 0:
                        yi.add_(k, alpha=hs * float(a))
            else:
                yi = stage_ref(y, ks, i, hs).to(dtype)
            ks.append(rhs(ctl.stage_t[i - 1], yi))
        y5 = yi
        if host_order:
            err = torch.zeros_like(y)
            for b5, b4, k in zip(B5, B4, ks):
                if b5 != b4:
                    err.add_(k, alpha=hs * (float(b5) - float(b4)))
            scale = atol + rtol * torch.maximum(y.abs(), y5.abs())
            ratio = float(torch.sqrt(torch.mean((err / scale) ** 2)))
        else:
            ratio = ratio_ref(y, y5, ks, hs, atol, rtol)
        if ctl.control(ratio):
            y, k1 = y5, ks[6]
        log.append((ratio, ratio <= 1.0, ctl.t, ctl.h))
    raise RuntimeError("drive: max_steps exceeded")


# ---- the kernels' operation order in numpy fp32 --------------------------------------------------------------------
def _f32_div(p: int, q: int) -> np.float32:
    return np.float32(p) / np.float32(q)


def coefficients_fp32():
    """DP_A and DP_E as csrc/ode.hip spells them: fp32 quotients of integers, DP_E an fp32 difference of two."""
    a = [[np.float32(0)] * 6 for _ in range(7)]
    for i, row in enumerate(A):
        for j, v in enumerate(row):
            a[i][j] = _f32_div(v.numerator, v.denominator)
    e = [_f32_div(b5.numerator, b5.denominator) - _f32_div(b4.numerator, b4.denominator) for b5, b4 in zip(B5, B4)]
    return a, e


def stage_fp32(y, ks, i: int, hs) -> np.ndarray:
    a, _ = coefficients_fp32()
    s = np.zeros_like(y, dtype=np.float32)
    for j in range(i):
        if a[i][j] != 0:
            s = s + a[i][j] * ks[j]
    return y + np.float32(hs) * s


def ratio_fp32(y, y5, ks, hs, atol: float, rtol: float) -> float:
    _, e = coefficients_fp32()
    s = np.zeros_like(y, dtype=np.float32)
    for j in range(7):
        if j != 1:
            s = s + e[j] * ks[j]
    sc = np.float32(atol) + np.float32(rtol) * np.maximum(np.abs(y), np.abs(y5))
    with np.errstate(all="ignore"):
        r = (np.float32(hs) * s / sc).astype(np.float64)
    return float(np.float32(math.sqrt(float(np.sum(r * r)) / y.size)))      # (slot 27 is an fp32 slot)


# ---- the synthetic inputs of tests/test_ode_step_gpu.py ------------------------------------------------------------
# the smallest sizes at which each loop can go wrong: one element, around one block, one past the error kernel's
# 256 x 256 wrap, one past the 2048-block cap of the stage and control kernels
SIZES = (1, 255, 256, 257, 65_537, 524_289)
HS = 0.37            # |first_step| of the synthetic attempts; the kernels see its fp32 rounding


def hs_fp32(sign: float) -> float:
    return float(np.float32(sign * HS))


def synthetic(n: int, seed: int = 0):
    """y with entries near 0 and near 1e4, k1..k7 of mixed magnitude 1e-3 .. 1e3 and both signs; at the last element
    values no other element has.  fp32 CPU tensors."""
    g = torch.Generator().manual_seed(1000 * seed + n % 997)

    def mixed():
        mag = 10.0 ** (6.0 * torch.rand(n, generator=g) - 3.0)
        return (mag * torch.sign(torch.randn(n, generator=g))).float()

    y = torch.where(torch.rand(n, generator=g) < 0.5, 1e-3 * torch.randn(n, generator=g),
                    1e4 * (1.0 + 0.1 * torch.randn(n, generator=g))).float()
    ks = [mixed() for _ in range(7)]
    y[-1] = -2.5e4
    for j, k in enumerate(ks):
        k[-1] = 2000.0 + 100.0 * j
    return y, ks


RATIO_CONFIGS = ("mixed", "y5_larger", "y5_smaller", "rtol0", "atol0", "last_only")


def ratio_case(n: int, config: str):
    """(y, y5, ks, atol, rtol) for the error-ratio checks."""
    y, ks = synthetic(n, seed=1)
    g = torch.Generator().manual_seed(7 + n % 991)
    atol, rtol = 1e-6, 1e-5
    y5 = (y + 0.05 * y.abs() * torch.randn(n, generator=g)).float()
    if config in ("y5_larger", "y5_smaller"):
        # rtol |y| above atol almost everywhere, so that which of |y|, |y5| the scale takes shows in the ratio
        atol, rtol = 1e-9, 1e-3
        y5 = (y * ((1.5 if config == "y5_larger" else 0.1) + 0.5 * torch.rand(n, generator=g))).float()
    elif config == "rtol0":
        atol, rtol = 1e-3, 0.0
    elif config == "atol0":
        atol, rtol = 0.0, 1e-5
        y = torch.where(y.abs() < 1e-3, torch.full_like(y, 1e-3), y)     # (a zero scale would make every term inf)
    elif config == "last_only":
        # all of the error in the last element alone: a loop that stops short of it sees a ratio of 0
        ks = [torch.zeros(n) for _ in range(7)]
        for j, k in enumerate(ks):
            k[-1] = 2000.0 + 100.0 * j
    return y, y5, ks, atol, rtol
