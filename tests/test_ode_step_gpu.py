"""The Dormand-Prince step kernels (csrc/ode.hip) one attempt at a time: sbi_amd_dopri5_init / _stage / _finish called
through the C ABI on synthetic buffers and held to the fp64 restatement of tests/ode_restatement.py -- the stage sums
and the error ratio within forward-error bounds derived from the operation count, every slot of the state block after
every attempt, the accept / reject decision with its FSAL hand-over, the grid-stride wraps of all three array kernels,
the attempt after the end, the ABI's refusals, and the number of right-hand-side calls of a real solve.
tests/test_ode_gpu.py holds whole solves to a tight solve; this file is what notices a wrong coefficient, scale, flag
or counter that an adaptive solve would silently correct for."""

import math
from ctypes import c_void_p
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from tests import ode_restatement as R
from tests.parity_log import record

pytestmark = pytest.mark.gpu

U = 2.0**-24            # fp32 unit roundoff
DEV = "cuda:0"


def _lib():
    from sbi_amd import _lib as binding

    return binding, binding.load()


def _kptr(ks):
    b, _ = _lib()
    return (c_void_p * 7)(*[b.ptr(k) for k in ks], *([None] * (7 - len(ks))))


def _stream():
    b, _ = _lib()
    return b.current_stream(torch.device(DEV))


def _init(state, t0, t1, first_step, atol, rtol) -> int:
    b, lib = _lib()
    return lib.sbi_amd_dopri5_init(b.ptr(state), t0, t1, first_step, atol, rtol, _stream())


def _stage(y, ks, i, state, out, n=None) -> int:
    b, lib = _lib()
    return lib.sbi_amd_dopri5_stage(b.ptr(y), _kptr(ks), i, b.ptr(state), b.ptr(out),
                                    y.numel() if n is None else n, _stream())


def _finish(y, y5, ks, state, scratch, n=None) -> int:
    b, lib = _lib()
    return lib.sbi_amd_dopri5_finish(b.ptr(y), b.ptr(y5), _kptr(ks), b.ptr(state), b.ptr(scratch),
                                     y.numel() if n is None else n, _stream())


def _new_state(t0, t1, first_step, atol, rtol):
    state = torch.zeros(R.STATE_FLOATS, dtype=torch.float32, device=DEV)
    assert _init(state, t0, t1, first_step, atol, rtol) == 0
    return state, R.Controller().init(t0, t1, first_step, atol, rtol)


def _scratch():
    return torch.full((256,), float("nan"), dtype=torch.float64, device=DEV)


def _bits(a, b) -> bool:
    """Bit-for-bit equality (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_state(state, model, what=""):
    """Slots 0..15 (doubles) match the model to 1e-12 relative, slots 16..28 are its doubles rounded to fp32, slots
    29..31 stay zero."""
    torch.cuda.synchronize()
    s = state.cpu()
    for name, got, want in zip("t h t_end direction atol rtol tiny step".split(), s[:16].view(torch.float64).tolist(),
                               model.doubles()):
        assert abs(got - want) <= 1e-12 * abs(want), f"{what}: double slot {name}: {got!r} vs {want!r}"
    want32 = model.slots()[16:29]
    for slot, (got, want) in enumerate(zip(s[16:29].tolist(), want32.tolist()), start=16):
        assert got == want or (got != got and want != want), f"{what}: slot {slot}: {got!r} vs {want!r}"
    assert s[29:].eq(0).all(), f"{what}: slots 29..31 were written"
    return s


def _cuda(*ts):
    return [t.to(DEV) for t in ts]


# ---- stage kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("n", R.SIZES)
def test_stage_sums_within_the_derived_bound(n, sign):
    y, ks = R.synthetic(n)
    y, *ks = _cuda(y, *ks)
    state, model = _new_state(*((0.0, 1.0) if sign > 0 else (1.0, 0.0)), R.HS, 1e-6, 1e-5)
    hs = R.hs_fp32(sign)
    s = _assert_state(state, model, "after init")
    assert s[R.SLOT_HS].item() == hs
    before = [t.clone() for t in (y, *ks, state)]
    worst = 0.0
    for i in range(1, 7):
        out = torch.full_like(y, float("nan"))
        assert _stage(y, ks[:i], i, state, out) == 0          # k[j] for j >= i: null, as dopri5.py passes them
        assert torch.isfinite(out).all(), f"stage {i}: {int((~torch.isfinite(out)).sum())} elements not written"
        err = (out.double() - R.stage_ref(y, ks, i, hs)).abs()
        bound = R.stage_bound(y, ks, i, hs)
        assert (err <= bound).all(), f"stage {i}: worst {float((err / bound).max()):.3f} x bound"
        assert err[-1] <= bound[-1]                           # the last element carries values no other one has
        worst = max(worst, float((err / bound).max()))
    for a, b in zip(before, (y, *ks, state)):
        assert _bits(a, b)
    record("ode_step", f"stage n={n} hs={hs:+.2f}", worst_fraction_of_bound=worst, gamma=R.GAMMA)


def test_stage_one_hot_pins_every_tableau_entry():
    n = 257
    y = torch.zeros(n, device=DEV)
    ks = [torch.zeros(n, device=DEV) for _ in range(7)]
    for sign in (1.0, -1.0):
        state, _ = _new_state(*((0.0, 1.0) if sign > 0 else (1.0, 0.0)), R.HS, 1e-6, 1e-5)
        hs = Fr(R.hs_fp32(sign))
        for i in range(1, 7):
            for j in range(i):
                ks[j].fill_(1.0)
                out = torch.full_like(y, float("nan"))
                assert _stage(y, ks[:i], i, state, out) == 0
                ks[j].zero_()
                want = hs * R.A[i][j]
                # two roundings: the fp32 coefficient and its product with hs (1 * a, 0 + a and 0 + hs a are exact)
                assert (out == out[0]).all()
                assert abs(Fr(out[0].item()) - want) <= 3 * U * abs(want), f"A[{i}][{j}]: {out[0].item()} vs {float(want)}"
                if want == 0:
                    assert out[0].item() == 0.0


# ---- error ratio ---------------------------------------------------------------------------------------------------
def _check_ratio(got, ref, bound, what):
    if math.isfinite(ref):
        assert abs(got - ref) <= bound, f"{what}: ratio {got!r} vs {ref!r}: {abs(got - ref) / bound:.3f} x bound"
    else:
        assert got == ref or (got != got and ref != ref), f"{what}: ratio {got!r} vs {ref!r}"


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("n", R.SIZES)
def test_error_ratio_within_the_derived_bound(n, sign):
    hs = R.hs_fp32(sign)
    scratch = _scratch()
    for config in R.RATIO_CONFIGS:
        y, y5, ks, atol, rtol = R.ratio_case(n, config)
        y, y5, *ks = _cuda(y, y5, *ks)
        state, _ = _new_state(*((0.0, 1.0) if sign > 0 else (1.0, 0.0)), R.HS, atol, rtol)
        ref, bound = R.ratio_ref(y, y5, ks, hs, atol, rtol), R.ratio_bound(y, y5, ks, hs, atol, rtol)
        assert math.isfinite(ref) and ref > 100.0 * bound        # (last_only: a loop that stops short sees 0)
        assert _finish(y.clone(), y5, [ks[0].clone(), *ks[1:]], state, scratch) == 0
        torch.cuda.synchronize()
        got = state[R.SLOT_RATIO].item()
        print(f"n {n} hs {hs:+.2f} {config}: ratio {got:.9g} ref {ref:.9g} bound {bound:.3g} "
              f"({abs(got - ref) / bound:.3f} of it)")
        record("ode_step", f"ratio n={n} hs={hs:+.2f} {config}", got=got, ref=ref, bound=bound,
               fraction_of_bound=abs(got - ref) / bound)
        _check_ratio(got, ref, bound, config)


def test_error_one_hot_pins_every_error_coefficient():
    n, atol = 257, 1e-3
    y = torch.full((n,), 0.5, device=DEV)
    y5 = torch.full((n,), -0.25, device=DEV)
    scratch = _scratch()
    for sign in (1.0, -1.0):
        hs = R.hs_fp32(sign)
        for j in range(7):
            ks = [torch.zeros(n, device=DEV) for _ in range(7)]
            ks[j].fill_(1.0)
            state, _ = _new_state(*((0.0, 1.0) if sign > 0 else (1.0, 0.0)), R.HS, atol, 0.0)
            ref, bound = R.ratio_ref(y, y5, ks, hs, atol, 0.0), R.ratio_bound(y, y5, ks, hs, atol, 0.0)
            assert abs(ref - abs(hs * float(R.E[j])) / atol) <= 1e-12 * ref or (j == 1 and ref == 0.0)
            assert _finish(y.clone(), y5, ks, state, scratch) == 0
            torch.cuda.synchronize()
            got = state[R.SLOT_RATIO].item()
            record("ode_step", f"one-hot E[{j}] hs={hs:+.2f}", got=got, ref=ref, bound=bound)
            if j == 1:
                assert got == 0.0                 # k2's weight is exactly zero
            else:
                _check_ratio(got, ref, bound, f"E[{j}]")


# ---- decision, FSAL hand-over, controller --------------------------------------------------------------------------
def _dial(k7, target, hs, atol):
    """With rtol = 0 and only k7 = c non-zero the ratio is |hs c / 40| / atol: fill k7 so that it is ``target``."""
    if target != target or target == math.inf:
        k7.fill_(target)
    else:
        k7.fill_(target * 40.0 * atol / abs(hs))


@pytest.mark.parametrize("target", [0.0, 1e-5, 0.9, 1.1, 1e4, math.inf, math.nan])
@pytest.mark.parametrize("n", R.SIZES)
def test_decision_fsal_and_controller(n, target):
    atol = 1e-3
    g = torch.Generator().manual_seed(n)
    y = torch.randn(n, generator=g).to(DEV)
    y5 = y + 1.0 + torch.rand(n, generator=g).to(DEV)            # differs from y everywhere
    ks = [torch.zeros(n, device=DEV) for _ in range(7)]
    ks[1] = torch.randn(n, generator=g).to(DEV) * 1e3            # k2 carries no weight: it must not matter
    state, model = _new_state(0.0, 1.0, 0.25, atol, 0.0)
    hs = model.hs
    _dial(ks[6], target, hs, atol)
    if target != 0.0:
        assert (ks[6] != ks[0]).all()                            # (all k are zero at ratio 0: nothing to hand over)
    y[-1], y5[-1] = 123.0, -456.0                                # the last element: values no other one has
    ref, bound = R.ratio_ref(y, y5, ks, hs, atol, 0.0), R.ratio_bound(y, y5, ks, hs, atol, 0.0)
    if math.isfinite(ref):
        assert abs(ref - target) <= 1e-6 * target and abs(ref - 1.0) > 100 * bound     # the reference alone decides
    want_accept = ref <= 1.0
    y_in, k1_in, others = y.clone(), ks[0].clone(), [t.clone() for t in (y5, *ks[1:])]
    assert _finish(y, y5, ks, state, _scratch()) == 0
    torch.cuda.synchronize()
    got = state[R.SLOT_RATIO].item()
    _check_ratio(got, ref, bound, f"n {n} target {target}")
    # every element carries the same error term, so the device's double ratio is its fp32 slot to ~1e-15: feeding the
    # slot to the model (its distance to the reference is checked above) gives the step size the device must hold
    assert model.control(float(got)) == want_accept
    s = _assert_state(state, model, f"n {n} target {target}")
    d = s[:16].view(torch.float64)
    if want_accept:
        assert _bits(y, others[0]) and _bits(ks[0], others[6])   # y <- y5, k1 <- k7, the last element included
        assert y[-1].item() == -456.0
        assert (s[R.SLOT_ACC].item(), s[R.SLOT_REJ].item()) == (1.0, 0.0)
        assert d[0].item() == 0.0 + hs                           # t advanced by the double step
    else:
        assert _bits(y, y_in) and _bits(ks[0], k1_in)
        assert y[-1].item() == 123.0
        assert (s[R.SLOT_ACC].item(), s[R.SLOT_REJ].item()) == (0.0, 1.0)
        assert d[0].item() == 0.0
    for a, b in zip(others, (y5, *ks[1:])):                      # y5 and k2..k7 are never written
        assert _bits(a, b)


@pytest.mark.parametrize("n", [257, 65_537])
def test_a_ratio_of_exactly_one_is_accepted(n):
    """The one constructed ratio that is not kept away from 1: every operation on the way to it is exact, whatever the
    compiler fuses.  hs = 2^-2, atol = 2^-10 and k7 = c with fp32(DP_E[6] * c) = -2^-8 (found by search among c's
    neighbours) give an error term of exactly -1 in every element, a sum of squares of exactly n and a ratio of exactly
    1.0 -- which `<=` accepts."""
    _, e32 = R.coefficients_fp32()
    c = np.float32(-(2.0**-8) / float(e32[6]))
    cands = [c]
    for _ in range(4):
        cands = [np.nextafter(cands[0], np.float32(0)), *cands, np.nextafter(cands[-1], np.float32(1))]
    exact = [x for x in cands if e32[6] * x == np.float32(-(2.0**-8))]
    assert exact, "no fp32 c with DP_E[6] * c == -2^-8"
    atol = 2.0**-10
    y = torch.linspace(-1.0, 1.0, n, device=DEV)
    y5 = y + 2.0
    ks = [torch.zeros(n, device=DEV) for _ in range(7)]
    ks[6].fill_(float(exact[0]))
    k7_in = ks[6].clone()
    state, model = _new_state(0.0, 1.0, 0.25, atol, 0.0)
    ref, bound = R.ratio_ref(y, y5, ks, 0.25, atol, 0.0), R.ratio_bound(y, y5, ks, 0.25, atol, 0.0)
    assert abs(ref - 1.0) <= bound                               # (the reference agrees that this is 1, to rounding)
    assert _finish(y, y5, ks, state, _scratch()) == 0
    torch.cuda.synchronize()
    assert state[R.SLOT_RATIO].item() == 1.0
    assert model.control(1.0)
    s = _assert_state(state, model, "ratio == 1")
    assert _bits(y, y5) and _bits(ks[0], k7_in) and s[R.SLOT_ACC].item() == 1.0 and s[R.SLOT_REJ].item() == 0.0


# ---- the state block over whole sequences of attempts --------------------------------------------------------------
@pytest.mark.parametrize("t0,t1,first_step", [(1.0, 0.0, 0.05), (0.0, 2.0, 0.05), (0.0, 1e-3, 1e-4),
                                              (0.0, 1e-3, 0.05), (0.0, 2.0, 5.0), (3.0, 1.0, 2.0)])
def test_state_block_follows_the_model_over_a_whole_solve(t0, t1, first_step):
    n, atol = 257, 1e-3
    pattern = [0.5, 2.0, 1e-6, 0.8]
    y = torch.linspace(-1.0, 1.0, n, device=DEV)
    ks = [torch.zeros(n, device=DEV) for _ in range(7)]
    scratch = _scratch()
    state, model = _new_state(t0, t1, first_step, atol, 0.0)
    span = abs(t1 - t0)
    assert model.last == (first_step >= span)                    # known already after init
    attempts = clamped = 0
    while True:
        s = _assert_state(state, model, f"before attempt {attempts}")
        d = s[:16].view(torch.float64).tolist()
        remaining = abs(d[2] - d[0])
        # "reaches t1" is set exactly on the attempts whose h was clamped to what remains
        assert (s[R.SLOT_LAST].item() == 1.0) == (remaining > d[6] and d[1] >= remaining)
        assert abs(d[7]) == min(d[1], remaining)
        if s[R.SLOT_FIN].item() == 1.0:
            break
        clamped += int(s[R.SLOT_LAST].item())
        assert attempts < 100
        target = pattern[attempts % 4]
        hs32 = s[R.SLOT_HS].item()
        ks[0].zero_()                                            # (an accepted attempt left the last k7 there)
        _dial(ks[6], target, hs32, atol)
        y5 = y + 1.0
        ref, bound = R.ratio_ref(y, y5, ks, hs32, atol, 0.0), R.ratio_bound(y, y5, ks, hs32, atol, 0.0)
        assert abs(ref - target) <= 1e-6 * target
        y_in = y.clone()
        assert _finish(y, y5, ks, state, scratch) == 0
        torch.cuda.synchronize()
        got = state[R.SLOT_RATIO].item()
        _check_ratio(got, ref, bound, f"attempt {attempts}")
        accepted = model.control(float(got))
        assert accepted == (target <= 1.0) and _bits(y, y5 if accepted else y_in)
        attempts += 1
    # the last accepted step lands t on t1 (within tiny), although the fp32 copy of that step may round past it
    assert abs(d[0] - t1) <= d[6] and d[6] == 1e-12 * max(span, 1.0)
    assert clamped >= 1 and model.accepted + model.rejected == attempts
    if (t0, t1, first_step) == (0.0, 1e-3, 0.05):
        assert attempts == 1 and float(np.float32(1e-3)) - 1e-3 > d[6]      # fp32(1e-3) overshoots t1 by 4.7e-11
    print(f"{t0} -> {t1}, first step {first_step}: {attempts} attempts, {model.rejected} rejected, {clamped} clamped")
    # finished stays: one more attempt is a no-op
    _dial(ks[6], 0.5, 1.0, atol)
    assert _finish(y, y.clone(), [ks[6].clone(), *ks[1:]], state, scratch) == 0
    model.control(0.0)
    s = _assert_state(state, model, "after the end")
    assert s[R.SLOT_FIN].item() == 1.0 and s[R.SLOT_LAST].item() == 0.0


def test_equal_end_points_are_finished_straight_after_init():
    state, model = _new_state(0.25, 0.25, 0.05, 1e-6, 1e-5)
    s = _assert_state(state, model, "t0 == t1")
    assert s[R.SLOT_FIN].item() == 1.0 and s[R.SLOT_LAST].item() == 0.0 and s[R.SLOT_HS].item() == 0.0


@pytest.mark.parametrize("k7", ["k1", "inf", "nan"])
def test_attempt_after_the_end_is_a_no_op(k7):
    """h = 0: the stage kernels hand y back (y5 = y) and a right-hand side returns k1 again; y, k1, t, h and the flags
    stay bit for bit -- also when k7 is not finite (0 * inf: the ratio is NaN) -- and neither counter moves."""
    n = 65_537
    g = torch.Generator().manual_seed(5)
    y = torch.randn(n, generator=g).to(DEV)
    ks = [torch.zeros(n, device=DEV) for _ in range(7)]
    scratch = _scratch()
    state, model = _new_state(0.0, 1.0, 2.0, 1e-3, 0.0)
    assert _finish(y, y + 1.0, ks, state, scratch) == 0          # ratio 0: accepted, t = t1
    model.control(0.0)
    s0 = _assert_state(state, model, "the step to t1")
    assert s0[R.SLOT_FIN].item() == 1.0 and s0[R.SLOT_ACC].item() == 1.0 and s0[R.SLOT_HS].item() == 0.0
    ks = [torch.randn(n, generator=g).to(DEV) for _ in range(7)]
    y5 = torch.full_like(y, float("nan"))
    assert _stage(y, ks[:6], 6, state, y5) == 0
    assert _bits(y5, y)                                          # hs = 0: the stage state is y itself
    if k7 == "k1":
        ks[6] = ks[0].clone()
    else:
        ks[6][::3] = float(k7)
    y_in, k1_in = y.clone(), ks[0].clone()
    assert _finish(y, y5, ks, state, scratch) == 0
    torch.cuda.synchronize()
    s1 = state.cpu()
    assert _bits(y, y_in) and _bits(ks[0], k1_in)
    assert _bits(s1[:16], s0[:16])                               # t, h and the other doubles
    for slot in (R.SLOT_HS, R.SLOT_T, R.SLOT_FIN, R.SLOT_LAST):
        assert s1[slot].item() == s0[slot].item()
    # a no-op attempt is neither accepted nor rejected
    assert (s1[R.SLOT_ACC].item(), s1[R.SLOT_REJ].item()) == (1.0, 0.0)
    assert s1[29:].eq(0).all()


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched():
    b, lib = _lib()
    bad = b.E_BADARG
    n = 257
    nan = float("nan")
    state = torch.full((R.STATE_FLOATS,), 3.0, device=DEV)
    for args in [(0.0, 1.0, 0.0, 1e-6, 1e-5), (0.0, 1.0, -0.05, 1e-6, 1e-5), (0.0, 1.0, nan, 1e-6, 1e-5),
                 (0.0, 1.0, 0.05, -1e-6, 1e-5), (0.0, 1.0, 0.05, nan, 1e-5), (0.0, 1.0, 0.05, 1e-6, -1e-5),
                 (0.0, 1.0, 0.05, 1e-6, nan)]:
        assert _init(state, *args) == bad, args
    assert lib.sbi_amd_dopri5_init(None, 0.0, 1.0, 0.05, 1e-6, 1e-5, _stream()) == bad
    torch.cuda.synchronize()
    assert state.eq(3.0).all()

    state, _ = _new_state(0.0, 1.0, 0.05, 1e-6, 1e-5)
    y = torch.full((n,), 5.0, device=DEV)
    out = torch.full((n,), 7.0, device=DEV)
    ks = [torch.full((n,), 9.0, device=DEV) for _ in range(7)]
    scratch = torch.full((256,), 11.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    state_in = state.clone()
    stream = _stream()
    assert _stage(y, ks[:6], 0, state, out) == bad
    assert _stage(y, ks[:6], 7, state, out) == bad
    assert _stage(y, ks[:6], -1, state, out) == bad
    assert _stage(y, ks[:3], 3, state, out, n=0) == bad
    assert _stage(y, ks[:3], 3, state, out, n=-5) == bad
    for j in range(4):                                           # a null k[j] for some j < stage
        holed = list(ks[:4])
        holed[j] = None
        assert _stage(y, holed, 4, state, out) == bad
    assert _stage(None, ks[:3], 3, state, out, n=n) == bad
    assert _stage(y, ks[:3], 3, None, out) == bad
    assert _stage(y, ks[:3], 3, state, None) == bad
    assert lib.sbi_amd_dopri5_stage(b.ptr(y), None, 3, b.ptr(state), b.ptr(out), n, stream) == bad
    y5 = torch.full((n,), 6.0, device=DEV)
    for j in range(7):                                           # finish needs all seven
        holed = list(ks)
        holed[j] = None
        assert _finish(y, y5, holed, state, scratch) == bad
    assert _finish(y, y5, ks, state, scratch, n=0) == bad
    assert _finish(None, y5, ks, state, scratch, n=n) == bad
    assert _finish(y, None, ks, state, scratch) == bad
    assert _finish(y, y5, ks, None, scratch) == bad
    assert _finish(y, y5, ks, state, None) == bad
    assert lib.sbi_amd_dopri5_finish(b.ptr(y), b.ptr(y5), None, b.ptr(state), b.ptr(scratch), n, stream) == bad
    torch.cuda.synchronize()
    assert y.eq(5.0).all() and y5.eq(6.0).all() and out.eq(7.0).all() and scratch.eq(11.0).all()
    assert all(k.eq(9.0).all() for k in ks) and _bits(state, state_in)


# ---- real solves ---------------------------------------------------------------------------------------------------
def _rhs(t, y):                      # the right-hand side of tests/test_ode_gpu.py
    return torch.sin(5.0 * t) * y - 0.7 * torch.tanh(2.0 * y)


@pytest.mark.parametrize("span", [(0.0, 2.0), (1.0, 0.0)])
@pytest.mark.parametrize("shape", [(257, 5), (65_537,)])
def test_real_solve_calls_the_right_hand_side_once_plus_six_per_attempt(shape, span):
    """The pipelined host loop never enqueues an attempt behind the end: the right-hand side is called 1 + 6 x
    attempts times, attempts being those of the restatement driver in fp32 on the CPU.  Every error ratio of that
    run is outside [0.9, 1.1] (asserted on the CPU run alone), so no decision can differ between the two."""
    from sbi_amd.samplers.ode_solvers.dopri5 import _odeint_device

    t0, t1 = span
    y0 = torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    want, log = R.drive(_rhs, y0, t0, t1, 1e-6, 1e-5, 0.03, host_order=True)
    ratios = [r for r, _, _, _ in log]
    assert all(not 0.9 <= r <= 1.1 for r in ratios), ratios
    assert any(r > 1.0 for r in ratios)                          # the reject path runs
    calls = [0]

    def counted(t, y):
        calls[0] += 1
        return _rhs(t, y)

    got = _odeint_device(counted, y0.to(DEV), t0, t1, 1e-6, 1e-5, 10_000, 0.03)
    torch.cuda.synchronize()
    print(f"shape {shape} span {span}: {len(log)} attempts, {calls[0]} calls")
    assert calls[0] == 1 + 6 * len(log)
    assert (got.cpu() - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("span", [(0.0, 2.0), (1.0, 0.0)])
def test_the_loop_of_the_integration_guide_reproduces_odeint_dopri5(span):
    """The ABI used exactly as INTEGRATION.md sketches it: one y_i buffer, slots 16 + i as the stage times, slot 24 to
    stop (read after every attempt)."""
    from sbi_amd.samplers.ode_solvers import odeint_dopri5

    b, lib = _lib()
    t0, t1 = span
    y0 = torch.randn(257, 5, generator=torch.Generator().manual_seed(3)).to(DEV)
    want = odeint_dopri5(_rhs, y0, t0, t1)

    y, y_i = y0.clone(), torch.empty_like(y0)
    state = torch.zeros(R.STATE_FLOATS, device=DEV)
    scratch = torch.empty(256, dtype=torch.float64, device=DEV)
    stream = _stream()
    assert lib.sbi_amd_dopri5_init(state.data_ptr(), t0, t1, 0.05, 1e-6, 1e-5, stream) == 0
    k = [_rhs(state[23:24], y)]
    attempts = 0
    while True:
        for i in range(1, 7):
            ks = (c_void_p * 7)(*[t.data_ptr() for t in k], *[None] * (7 - len(k)))
            assert lib.sbi_amd_dopri5_stage(y.data_ptr(), ks, i, state.data_ptr(), y_i.data_ptr(), y.numel(),
                                            stream) == 0
            k.append(_rhs(state[16 + i : 17 + i], y_i))
        ks = (c_void_p * 7)(*[t.data_ptr() for t in k])
        assert lib.sbi_amd_dopri5_finish(y.data_ptr(), y_i.data_ptr(), ks, state.data_ptr(), scratch.data_ptr(),
                                         y.numel(), stream) == 0
        k = k[:1]
        attempts += 1
        assert attempts < 1000
        if state[24].item() == 1.0:                              # (synchronises)
            break
    s = state.cpu()
    assert _bits(y, want)
    assert s[R.SLOT_ACC].item() + s[R.SLOT_REJ].item() == attempts and s[R.SLOT_REJ].item() >= 1.0
    assert abs(s[:16].view(torch.float64)[0].item() - t1) <= 1e-12 * max(1.0, abs(t1 - t0))
