"""Keeps tests/lru_envelope.py honest, without a device: its slot table against the C ABI's offsets and the module's
parameters, its LDS image against the plan, the LDS corners include/sbi_amd_lru.h names, every GPU case inside the plan,
and the teeth of the per-slot bound: seeded defects that the whole-vector bound of tests/test_lru_embedding_gpu.py lets
through and `slot_check` names.

Measured here for the seeded defects (fp32 module on the CPU against the fp64 oracle, the suite's `spread(., 0)` weights
and inputs; whole-vector bar = 4 x the eager error over all parameters):
  (65, 17, 3, 72, 33, unidirectional, 3 blocks, mean), whole-vector bar 3.1e-2
    b0.bg x 1.002                  defect 1.1e-2   slot bar 6.3e-5
    b1.D x 1.002                   defect 2.4e-2   slot bar 1.3e-4
    b2.log_nu x (1 - 1/T)          defect 2.4e-1   slot bar 1.5e-4   the whole-vector bound rejects it too
    b2.log_nu x (1 - 1/(16 T))     defect 1.5e-2   slot bar 1.5e-4
  (65, 17, 3, 72, 33, bidirectional, 3 blocks, mean), whole-vector bar 6.0e-1
    b1.log_theta.rev x (1 - 1/T)         defect 3.7e+1   slot bar 4.2e-2   the whole-vector bound rejects it too
    b1.log_theta.rev x (1 - 1/(128 T))   defect 2.9e-1   slot bar 4.2e-2
A whole step of 65 missing from log_nu (max|ref| 15) or log_theta (max|ref| 2.4e3) is 8 and 60 times the whole-vector
bar: the old bound did see that.  What it let through are the same defects at 1/16 resp. 1/128 of a step, and anything
in the small slots (bg, D).  log_theta carries the whole vector's largest entries and errors, so its own slots gain the
least: a factor 14 in b1.log_theta.rev, against 490 in b0.bg.  In every case only the seeded slot fails: the forward
half of a tensor whose reversed half is scaled passes."""
import ctypes
import functools

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import LRUEmbedding
from sbi_amd.neural_nets.embedding_nets import lru as L
from tests import lru_envelope as env
from tests.test_lru_embedding_gpu import check

CASE_IDS = [env.case_id(c) for c in env.ALL_CASES]


def plan_of(dims, B=2, T=33):
    lds, fwd = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = _lib.load().sbi_amd_lru_plan(ctypes.byref(L.lru_config(dims)), B, T, ctypes.byref(lds), ctypes.byref(fwd))
    return rc, lds.value, fwd.value


def dims(I, H, S, bidir):
    return (I, H, S, 2, int(bidir), 0)


@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_slot_table_is_the_flat_image(case):
    d = env.dims_of(case)
    net = LRUEmbedding(d[0], 5, state_dim=d[2], hidden_dim=d[1], num_blocks=d[3], bidirectional=bool(d[4]),
                       aggregate_fcn=case[7])
    assert net.dims == d
    tensors = env.tensor_table(d)
    params = net.kernel_parameters()
    assert [n for _, _, n in tensors] == [L.real_view(p).numel() for p in params]
    assert [o for _, o, _ in tensors] == [sum(n for _, _, n in tensors[:i]) for i in range(len(tensors))]
    offsets = (ctypes.c_int64 * (1 + d[3]))()
    P = _lib.load().sbi_amd_lru_param_count(ctypes.byref(L.lru_config(d)), offsets)
    assert P == tensors[-1][1] + tensors[-1][2] == L.flat_image(params).numel()
    by_name = {name: o for name, o, _ in tensors}
    assert list(offsets) == [by_name["input.W"]] + [by_name[f"b{i}.log_nu"] for i in range(d[3])]
    # the slots partition [0, P)
    slots = env.slot_table(d)
    assert len({name for name, _ in slots}) == len(slots)
    assert torch.equal(torch.cat([idx for _, idx in slots]).sort().values, torch.arange(P))
    # ... and a split slot holds the entries of its half: mark every parameter with its state's half, read it back
    with torch.no_grad():
        for blk in net.lru_blocks:
            u, S = blk.lru, d[2]
            for p, axis in ((u.log_nu, 0), (u.log_theta, 0), (u.log_gamma, 0), (u.B, 0), (u.C, 1)):
                half = (torch.arange(p.shape[axis]) >= S).float() + 1.0          # 1 forward, 2 reversed
                shape = [-1 if a == axis else 1 for a in range(p.dim())]
                p.copy_(half.view(shape).expand(p.shape) * (1 + 1j if p.is_complex() else 1))    # re = im = mark
    flat = L.flat_image(net.kernel_parameters())
    lengths = {name: n for name, _, n in tensors}
    for name, idx in slots:
        if name.endswith((".fwd", ".rev")):
            assert (flat[idx] == (1.0 if name.endswith(".fwd") else 2.0)).all(), name
            assert 2 * idx.numel() == lengths[name.rsplit(".", 1)[0]], name
    assert d[4] == any(name.endswith(".rev") for name, _ in slots)


@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_image_formula_is_the_plan_s_and_every_case_plans(case):
    d = env.dims_of(case)
    rc, lds, fwd = plan_of(d, case[1], case[0])
    S2 = d[2] * (2 if d[4] else 1)
    assert (4 * env.lds_floats(d[0], d[1], S2)[0], 4 * env.lds_floats(d[0], d[1], S2)[1]) == (lds, fwd)
    assert rc == 0 and env.fits(d[0], d[1], S2) and L.plan(d, case[1], case[0]) == 0


def test_the_lds_corners_of_the_header_through_the_plan():
    """H = 128 up to S2 = 17, H = 72 up to S2 = 76 (either direction), S = 128 unidirectional with I = 1 up to H = 47,
    I = 64 with S2 = 16 up to the H the case table uses: the last that fits and the first that does not."""
    I = env.BASE[2]
    fits, over = [dims(I, 128, 17, False), dims(I, 72, 76, False), dims(I, 72, 38, True), dims(1, 47, 128, False)], \
                 [dims(I, 128, 18, False), dims(I, 128, 9, True), dims(I, 72, 77, False), dims(1, 72, 77, False),
                  dims(1, 48, 128, False)]
    H64 = env.largest_hidden(64, env.CORNER_I64_S2)
    fits.append(dims(64, H64, env.CORNER_I64_S2 // 2, True))
    assert H64 == 127          # so H64 + 1 is still inside the envelope and must answer E_LDS
    over.append(dims(64, H64 + 1, env.CORNER_I64_S2 // 2, True))
    for d in fits:
        rc, lds, _ = plan_of(d)
        assert rc == 0 and lds <= env.LDS_LIMIT_BYTES, (d, rc, lds)
    for d in over:
        rc, lds, _ = plan_of(d)
        assert rc == _lib.E_LDS and lds > env.LDS_LIMIT_BYTES, (d, rc, lds)
    corner_dims = [env.dims_of(c)[:3] + (env.dims_of(c)[4],) for c, _ in env.LDS_CORNERS]
    assert corner_dims == [(I, 128, 17, 0), (I, 72, 76, 0), (I, 72, 38, 1), (I, 47, 128, 0), (64, H64, 8, 1)]
    # the corners are the largest images of the table: within 2 % of the limit
    assert all(plan_of(env.dims_of(c))[1] > 0.98 * env.LDS_LIMIT_BYTES for c, _ in env.LDS_CORNERS)


def test_the_case_table_reaches_the_edges_it_names():
    cases = [c for c, _ in env.GPU_CASES]
    assert all(why for _, why in env.GPU_CASES) and len(set(cases)) == len(cases)

    def one_factor(i):
        return {c[i] for c in cases if all(c[j] == env.BASE[j] for j in range(8) if j not in (i, 4, 5))}

    assert {c[3] for c in cases} >= {1, 2, 3, 5, 15, 17, 18, 19, 50, 127, 128}
    assert {c[3] % 4 for c in cases} == {0, 1, 2, 3}
    assert {(c[4], c[5]) for c in cases} >= {(1, True), (2, True), (15, True), (16, True), (17, True), (64, True),
                                             (65, False), (128, False)}
    assert one_factor(2) >= {2, 4, 5, 16, 17, 63, 64}
    assert {(c[6], c[5]) for c in cases} >= {(8, True), (8, False)}
    steps = [c for c, _ in env.STEPS]
    for T in env.STEP_VALUES:
        assert {c[5] for c in steps if c[0] == T} == {True, False} and {c[7] for c in steps if c[0] == T} == {
            "mean", "last_step"}
    assert {(c[5], c[7]) for c in steps} == {(b, a) for b in (True, False) for a in env.AGGREGATIONS}
    assert set(env.STEP_VALUES) == {1, 2, 16, 17, 31, 32, 33, 48, 49}
    assert [c[1] for c, _ in env.BATCHES] == [511, 512, 513, 1025]
    assert all(c[0] == 130 and -(-c[0] // env.TILE) == 9 for c, _ in env.CONDITIONING)


def test_the_conditioned_nets_are_what_the_table_says():
    for case, what in env.CONDITIONING:
        net = env.inputs(case, conditioned=what)[0]
        for blk in net.lru_blocks:
            lam = blk.lru.lambda_complex.detach().to(torch.complex128)
            if what == "radius":
                assert (lam.abs() - (1 - 1e-3)).abs().max() < 1e-6
            else:
                phase = torch.exp(blk.lru.log_theta.detach().double())
                assert (phase - torch.pi).abs().max() <= 1e-3 and (lam.real < 0).all()


def test_repeated_batches_are_a_weighted_sum_of_their_distinct_rows():
    case = env.vary(T=5, B=40, I=1, H=4, S=2)
    net, x, wts, n = env.inputs(case)
    assert n == 17 and torch.equal(x[17:34], x[:17]) and torch.equal(wts[34:], wts[:6])
    features, grad, mag = env.per_sequence(net, x, wts, n)
    all_features, all_grad, all_mag = env.per_sequence(net, x, wts)
    assert torch.equal(features, all_features)
    assert (grad - all_grad).abs().max() <= 1e-12 * mag.max() and (mag - all_mag).abs().max() <= 1e-12 * mag.max()
    assert (mag >= grad.abs() - 1e-12 * mag.max()).all()


# ---- the per-slot bound has teeth ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stand_in(bidirectional):
    """(case, dims, fp32 gradient of the mode="scan" module, of the mode="loop" module, fp64 features, gradient,
    sum_b |g_b|) on the CPU"""
    case = (65, 17, 3, 72, 33, bidirectional, 3, "mean")
    net, x, wts, n = env.inputs(case)
    features, ref, mag = env.per_sequence(net, x, wts, n)
    grads = []
    for mode in ("scan", "loop"):
        m = LRUEmbedding(case[2], 5, state_dim=case[4], hidden_dim=case[3], num_blocks=case[6],
                         bidirectional=bidirectional, aggregate_fcn=case[7], mode=mode)
        m.load_state_dict(net.state_dict(), strict=True)
        (m.features(x) * wts).sum().backward()
        grads.append(L.flat_image([p.grad for p in m.kernel_parameters()]))
    return case, grads[0], grads[1], ref, mag


def test_the_unmodified_stand_in_passes_every_slot():
    for bidirectional in (False, True):
        case, kernel, eager, ref, mag = stand_in(bidirectional)
        figures = env.slot_check("lru_envelope_cpu_stand_in", case, kernel, eager, ref, mag)
        assert len(figures) == 2 + 3 * (13 if bidirectional else 8)
        check("lru_envelope_cpu_stand_in", env.case_id(case), "param_grad", kernel, eager, ref)


T65 = 65
# (bidirectional, slot, factor, whether the whole-vector bound lets it through)
DEFECTS = [(False, "b0.bg", 1.002, True),
           (False, "b1.D", 1.002, True),
           (False, "b2.log_nu", 1 - 1 / T65, False),                   # one step of 65: 0.24 against a bar of 3.1e-2
           (False, "b2.log_nu", 1 - 1 / (16 * T65), True),             # ... of one sequence in 16
           (True, "b1.log_theta.rev", 1 - 1 / T65, False),             # one step of 65: 37 against a bar of 0.60
           (True, "b1.log_theta.rev", 1 - 1 / (128 * T65), True)]


@pytest.mark.parametrize("bidirectional,slot,factor,old_passes", DEFECTS,
                         ids=[f"{d[1]}-{abs(1 - d[2]):.1e}" for d in DEFECTS])
def test_a_seeded_defect_fails_its_slot_and_which_of_them_the_whole_vector_bound_lets_through(bidirectional, slot,
                                                                                               factor, old_passes):
    case, kernel, eager, ref, mag = stand_in(bidirectional)
    idx = dict(env.slot_table(env.dims_of(case)))[slot]
    broken = kernel.clone()
    broken[idx] *= factor
    defect = (broken - kernel).abs().max().item()
    whole_bar = 4 * (eager.double() - ref).abs().max().item()
    good = env.slot_figures(env.dims_of(case), kernel, eager, ref, mag)[slot]
    print(f"{slot} x {factor:.6f}: defect {defect:.3e}, whole-vector bar {whole_bar:.3e}, slot bar {good['bound']:.3e}")
    assert defect > 2 * good["bound"] + good["kernel_err"]
    if old_passes:
        assert defect + good["kernel_err"] < whole_bar
        check("lru_envelope_cpu_defect", env.case_id(case), slot, broken, eager, ref)
    else:
        with pytest.raises(AssertionError):
            check("lru_envelope_cpu_defect", env.case_id(case), slot, broken, eager, ref)
    with pytest.raises(AssertionError) as e:
        env.slot_check("lru_envelope_cpu_defect", case, broken, eager, ref, mag, tag=f"{slot}x{factor:.6f}")
    failing = e.value.args[0][1]
    assert list(failing) == [slot], failing
