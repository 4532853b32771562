"""The specification of the Dormand-Prince stepper (tests/ode_restatement.py) pinned by itself, without a GPU: the
tableau satisfies the order conditions exactly, the floats of samplers/ode_solvers/dopri5.py are that tableau, a solve
driven by the controller model is ``_odeint_host`` bit for bit, and the plain fp32 restatement of the two array
operations stays inside the derived forward-error bounds on every input the GPU tests use."""

import math
from fractions import Fraction as Fr
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import ode_restatement as R


# ---- order conditions ----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _forests(order: int, largest: int):
    """Multisets of rooted trees with ``order`` vertices in all, every tree of at most ``largest`` vertices (and
    canonically ordered, so each multiset appears once)."""
    if order == 0:
        return ((),)
    out = []
    for m in range(min(order, largest), 0, -1):
        for first in _trees(m):
            for rest in _forests(order - m, m):
                if not rest or (m, first) >= (_order(rest[0]), rest[0]):
                    out.append((first, *rest))
    return tuple(out)


@lru_cache(maxsize=None)
def _trees(order: int):
    """Rooted trees with ``order`` vertices, each the tuple of its root's subtrees."""
    return _forests(order - 1, order - 1)


def _order(tree) -> int:
    return 1 + sum(_order(c) for c in tree)


def _density(tree) -> int:            # gamma(tau)
    return _order(tree) * math.prod(_density(c) for c in tree)


_A7 = [[(R.A[i][j] if j < len(R.A[i]) else Fr(0)) for j in range(7)] for i in range(7)]


def _weights(tree):                   # Phi_i(tau), i = 1..7
    out = [Fr(1)] * 7
    for c in tree:
        phi = _weights(c)
        out = [o * sum(_A7[i][j] * phi[j] for j in range(7)) for i, o in enumerate(out)]
    return out


def _residual(b, tree) -> Fr:
    return sum(bi * w for bi, w in zip(b, _weights(tree))) - Fr(1, _density(tree))


def test_rooted_trees_are_counted_right():
    assert [len(_trees(p)) for p in range(1, 6)] == [1, 1, 2, 4, 9]
    assert len({t for p in range(1, 6) for t in _trees(p)}) == 17


def test_tableau_satisfies_the_order_conditions_exactly():
    for i in range(7):
        assert sum(R.A[i], Fr(0)) == R.C[i], f"row {i} of A does not sum to c"
    assert R.A[6] == R.B5[:6] and R.B5[6] == 0          # FSAL: stage 7 is evaluated at the fifth-order solution
    upto5 = [t for p in range(1, 6) for t in _trees(p)]
    upto4 = [t for p in range(1, 5) for t in _trees(p)]
    assert len(upto5) == 17 and len(upto4) == 8
    assert all(_residual(R.B5, t) == 0 for t in upto5)
    assert all(_residual(R.B4, t) == 0 for t in upto4)
    assert any(_residual(R.B4, t) != 0 for t in _trees(5))
    assert all((e == 0) == (j == 1) for j, e in enumerate(R.E))      # k2 alone carries no error weight


def test_floats_of_dopri5_are_the_exact_tableau_rounded_to_double():
    from sbi_amd.samplers.ode_solvers import dopri5

    assert dopri5._C == tuple(float(c) for c in R.C)
    assert dopri5._A == tuple(tuple(float(a) for a in row) for row in R.A)
    assert dopri5._B5 == tuple(float(b) for b in R.B5)
    assert dopri5._B4 == tuple(float(b) for b in R.B4)


def test_fp32_error_coefficients_cancel_by_at_most_what_the_bound_assumes():
    """DP_E is an fp32 difference of two fp32 quotients: its error, relative to |B5| + |B4|, is what the error-term
    bound charges for it (three of GAMMA's sixteen roundings at the very most)."""
    _, e32 = R.coefficients_fp32()
    worst = max(abs(Fr(float(e)) - ex) / (abs(b5) + abs(b4))
                for e, ex, b5, b4 in zip(e32, R.E, R.B5, R.B4) if ex != 0)
    print(f"fp32 DP_E: worst error {float(worst):.3e} of |B5| + |B4|")
    assert worst <= 3 * 2.0**-24
    assert e32[1] == 0


# ---- controller model ----------------------------------------------------------------------------------------------
def test_controller_model_transitions():
    c = R.Controller().init(1.0, 0.0, 0.05, 1e-6, 1e-5)
    assert (c.t, c.h, c.direction, c.hs, c.tiny) == (1.0, 0.05, -1.0, -0.05, 1e-12)
    assert c.stage_t == [1.0 - 0.05 * float(x) for x in R.C[1:]] and not c.finished and not c.last
    assert c.control(1.0) and c.t == 0.95 and c.h == 0.05 * 0.9 and c.accepted == 1          # ratio == 1 accepts
    assert not c.control(float("nan")) and c.t == 0.95 and c.rejected == 1                   # NaN rejects, factor 0.2
    assert c.h == 0.05 * 0.9 * 0.2
    h = c.h
    assert c.control(0.0) and c.h == h * 5.0                                                # factor 5 at ratio <= 0
    h = c.h
    assert not c.control(float("inf")) and c.h == h * 0.2                                   # clamps
    h = c.h
    assert c.control(1e-9) and c.h == h * 5.0
    s = c.slots()
    assert s.shape == (32,) and s[29:].eq(0).all()
    assert s[:16].view(torch.float64).tolist() == c.doubles()
    # first_step beyond the span: clamped at init, and the very first attempt is flagged as reaching t1
    c = R.Controller().init(0.0, 1e-3, 0.05, 1e-6, 1e-5)
    assert c.h == 1e-3 and c.last and c.tiny == 1e-12
    assert c.control(0.5) and c.finished and not c.last and c.hs == 0.0 and c.t == 1e-3
    # an attempt after the end is a no-op: no counter, t and h stay
    before = (c.doubles()[:7], c.accepted, c.rejected)
    c.control(0.0)
    c.control(float("nan"))
    assert (c.doubles()[:7], c.accepted, c.rejected) == before and c.finished
    c = R.Controller().init(0.25, 0.25, 0.05, 1e-6, 1e-5)
    assert c.finished and c.hs == 0.0


# ---- the driver against _odeint_host ------------------------------------------------------------------------------
def _rhs_smooth(t, y):
    return torch.sin(5.0 * t) * y - 0.7 * torch.tanh(2.0 * y)


def _rhs_stiff(t, y):
    return -40.0 * y


def _host_with_log(f, y0, t0, t1, atol, rtol, first_step):
    """_odeint_host, with the time of every right-hand-side call recorded (its attempts are six calls each)."""
    from sbi_amd.samplers.ode_solvers.dopri5 import _odeint_host

    times = []

    def counted(t, y):
        times.append(float(t))
        return f(t, y)

    return _odeint_host(counted, y0, t0, t1, atol, rtol, 10_000, first_step), times


@pytest.mark.parametrize("case", ["smooth forward", "smooth backward", "stiff forward", "stiff backward"])
def test_driver_is_odeint_host_bit_for_bit(case):
    g = torch.Generator().manual_seed(3)
    if case.startswith("smooth"):
        f, y0, first_step = _rhs_smooth, torch.randn(257, 5, generator=g, dtype=torch.float64), 0.05
        t0, t1 = (0.0, 2.0) if case.endswith("forward") else (1.0, 0.0)
    else:
        f, y0, first_step = _rhs_stiff, torch.full((64, 4), 2.0, dtype=torch.float64), 1.0
        t0, t1 = (0.0, 1.0) if case.endswith("forward") else (1.0, 0.9)     # (backward, -40 y grows: a short span)
    want, times = _host_with_log(f, y0, t0, t1, 1e-6, 1e-5, first_step)

    seen = []

    def counted(t, y):
        seen.append(float(t))
        return f(t, y)

    got, log = R.drive(counted, y0, t0, t1, 1e-6, 1e-5, first_step, host_order=True)
    assert torch.equal(got, want)
    # the same attempts: every right-hand-side call at the same time, one plus six per attempt
    assert seen == times and len(times) == 1 + 6 * len(log)
    accepted = [a for _, a, _, _ in log]
    print(f"{case}: {len(log)} attempts, {accepted.count(False)} rejected")
    assert accepted[-1] and abs(log[-1][2] - t1) <= 1e-12 * max(1.0, abs(t1 - t0))
    if case.startswith("stiff"):
        assert not accepted[0]                 # first_step = 1 is far too long for -40 y
    # stage 6 is evaluated at t + hs: the next attempt starts from there exactly when this one was accepted
    t_now = t0
    for k, (_, ok, t_after, _) in enumerate(log):
        assert t_after == (times[1 + 6 * k + 4] if ok else t_now)
        t_now = t_after
    # the helpers' operation order (one fused sum) takes the same decisions and lands on the same solution
    got2, log2 = R.drive(f, y0, t0, t1, 1e-6, 1e-5, first_step)
    assert [a for _, a, _, _ in log2] == accepted
    assert (got2 - want).abs().max().item() <= 1e-9 * max(1.0, want.abs().max().item())


def test_host_loop_shrinks_the_step_after_a_nan_attempt():
    """A right-hand side that overflows on a too-long first step: the error ratio is NaN, the attempt is rejected and
    the step shrinks by 0.2 (the device controller's rule), so the solve recovers instead of repeating the attempt."""
    from sbi_amd.samplers.ode_solvers.dopri5 import _odeint_host

    def f(t, y):
        return torch.where(y.abs() > 50.0, torch.full_like(y, float("nan")), -40.0 * y)

    y0 = torch.full((8,), 2.0, dtype=torch.float64)
    want, log = R.drive(f, y0, 0.0, 1.0, 1e-6, 1e-5, 1.0, host_order=True)
    assert math.isnan(log[0][0]) and not log[0][1] and log[0][3] == 0.2
    got = _odeint_host(f, y0, 0.0, 1.0, 1e-6, 1e-5, 10_000, 1.0)
    assert torch.equal(got, want)
    assert (got - 2.0 * math.exp(-40.0)).abs().max().item() <= 1e-6


# ---- the bounds are conditions a plain fp32 restatement meets on its own ------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_fp32_restatement_stays_inside_the_derived_bounds(n):
    worst_stage = worst_ratio = 0.0
    y, ks = R.synthetic(n)
    yn, kn = y.numpy(), [k.numpy() for k in ks]
    for sign in (1.0, -1.0):
        hs = R.hs_fp32(sign)
        for i in range(1, 7):
            got = R.stage_fp32(yn, kn, i, hs).astype(np.float64)
            err = (torch.from_numpy(got) - R.stage_ref(y, ks, i, hs)).abs()
            bound = R.stage_bound(y, ks, i, hs)
            assert (err <= bound).all(), f"stage {i} hs {hs}"
            worst_stage = max(worst_stage, (err / bound).max().item())
        for config in R.RATIO_CONFIGS:
            y_, y5, ks_, atol, rtol = R.ratio_case(n, config)
            got = R.ratio_fp32(y_.numpy(), y5.numpy(), [k.numpy() for k in ks_], hs, atol, rtol)
            ref, bound = R.ratio_ref(y_, y5, ks_, hs, atol, rtol), R.ratio_bound(y_, y5, ks_, hs, atol, rtol)
            assert math.isfinite(ref) and ref > 0.0
            assert abs(got - ref) <= bound, f"ratio {config} hs {hs}: {got} vs {ref}, bound {bound}"
            worst_ratio = max(worst_ratio, abs(got - ref) / bound)
    print(f"n = {n}: fp32 restatement uses {worst_stage:.3f} of the stage bound, {worst_ratio:.3f} of the ratio bound")
