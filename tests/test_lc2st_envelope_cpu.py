"""Keeps the case table of tests/lc2st_envelope.py honest, without a device: the table reaches every tile, chunk and
row-block edge of csrc/lc2st_kernel.h it is there for; the bounds of tests/test_lc2st_envelope_gpu.py hold for the
fp32 eager oracle alone with a factor 5 to spare; the rows and columns a wrong tile bound would drop carry a visible
share of the gradient at some case; and dropping one breaks the bound.

Measured on the CPU with the table's recipe (R = 150, default_rng(sum(shape) + 1000), initial seeds 100 + m), fp32
oracle against fp64: whole gradient at most 3.7e-5 of its largest entry at (1, 1, 1) and 5.2e-7 at every other shape
(bound 2e-4), worst block 3.7e-5 (bound 3e-4), loss within 0.7 % of its tolerance, evaluation probability 2.3e-7; the
smallest edge share is 0.18 (db2's last entry at (48, 16, 128)); more than 0.93 of the entries of the first-step
members' gradients are above 1e-6 at every shape."""
import pytest
import torch

from tests import lc2st_envelope as env
from tests import lc2st_oracle as O

SPARE = 5.0


def test_the_table_reaches_every_edge_it_names():
    plans = [env.plan(s) for s in env.SHAPE_LIST]
    assert all(p["Fp"] % 16 == 0 and p["Fp"] - 16 < p["F"] <= p["Fp"] <= 64 for p in plans)
    assert all(p["Hp"] % 16 == 0 and p["Hp"] - 16 < p["H"] <= p["Hp"] <= 128 for p in plans)
    assert {p["FB"] for p in plans} == {1, 2, 3, 4}
    assert {p["HB"] for p in plans} >= {1, 2, 3, 4, 7, 8}
    assert any(p["H"] % 16 == 1 and p["HB"] > 1 for p in plans)           # a tile with one live row
    assert any(p["F"] % 16 == 1 and p["FB"] > 1 for p in plans)           # ... and one live column
    assert {p["HB"] for p in plans if p["H"] % 16 == 1} >= {2, 3, 4, 8}   # H = 17, 33, 49, 113
    assert {p["FB"] for p in plans if p["F"] % 16 == 1} >= {2, 3, 4}      # F = 17, 33, 49
    assert any(p["K1"] == p["D"] for p in plans) and any(p["K1"] == p["D"] + 15 for p in plans)
    assert {p["D"] for p in plans} >= {15, 16, 17, 32, 33} and {(p["D"], p["Dx"]) for p in plans} >= {(63, 1), (1, 63)}
    assert any(p["H"] == 128 and p["F"] == 64 for p in plans)
    assert any(p["Hp"] == p["H"] and p["Fp"] == p["F"] and p["HB"] == p["FB"] == 1 for p in plans)

    nts, nvs = [s[0] for s in env.MEMBER_SIZES], [s[1] for s in env.MEMBER_SIZES]
    assert max(nt + nv for nt, nv in env.MEMBER_SIZES) <= env.DATA_ROWS          # row lists are subsets of the rows
    assert 1 in nts and 2 in nts
    assert any(nv % 32 == 0 for nv in nvs) and any(nv % 32 == 1 for nv in nvs) and {32, 64} <= set(nvs)
    per_b = {B: [env.batches(nt, B) for nt in nts] for B in env.GRAD_BATCH_SIZES}
    last_rows = {(B, bs[-1][1]) for B, all_b in per_b.items() for bs in all_b}
    assert (32, 1) in last_rows                                           # nt = 97, B = 32: a one-row last batch
    assert any(B > 1 and r == 1 and len(bs) > 1 for B, all_b in per_b.items() for bs in all_b for r in [bs[-1][1]])
    assert any(nt < B for B in env.GRAD_BATCH_SIZES for nt in nts)
    assert any(nt == B for B in env.GRAD_BATCH_SIZES for nt in nts)
    assert {1, 32, 33, 64} <= set(env.GRAD_BATCH_SIZES) and any(B < 32 for B in env.GRAD_BATCH_SIZES)
    shapes_of_chunks = {env.chunks(rows) for all_b in per_b.values() for bs in all_b for _, rows in bs}
    assert {(1, 1), (1, 31), (1, 32), (2, 1), (2, 32), (4, 1)} <= shapes_of_chunks      # (chunks, rows of the last)
    for B in env.GRAD_BATCH_SIZES:
        idx = env.grad_batches(B)
        assert idx[0] == 0 and all(idx[-1] * B >= nt for nt in nts)       # the last index is past every member's end
        assert all(len(env.batches(nt, B)) - 1 in idx for nt in nts)
    assert set(env.TRAJECTORY_BATCH_SIZES) == {32, 33} and 1 not in env.TRAJECTORY_BATCH_SIZES
    assert all(len(env.batches(env.MEMBER_SIZES[m][0], env.FIRST_STEP_BATCH_SIZE)) == 1
               for m in env.FIRST_STEP_MEMBERS)

    assert {n % env.EVAL_ROWS for n in env.EVAL_SIZES} >= {0, 1, 511} and max(env.EVAL_SIZES) > 1024
    assert {1, 31, 32, 33} <= set(env.EVAL_SIZES)
    assert set(env.EVAL_LAYOUTS) == {(1, False), (1, True), (3, False), (3, True)}
    data, members, params0 = env.inputs(env.SHAPE_LIST[0])
    assert len(set(members.member_id.tolist())) == 5 and (members.member_id != range(5)).all()
    assert members.init_seed.tolist() == [100, 101, 102, 103, 104]


@pytest.mark.parametrize("shape", env.SHAPE_LIST, ids=env.shape_id)
def test_the_fp32_oracle_alone_keeps_the_gradient_bounds_with_room(shape):
    data, members, params0 = env.inputs(shape)
    worst = dict(loss=0.0, rel=0.0, block=0.0)
    for (B, which, epoch, batch, m), (rows, lab, l64, g64) in env.grad_references(shape).items():
        h = env.hyper(shape, batch_size=B)
        l32, g32 = O.loss_and_grad(h, params0[m], data, rows, lab, torch.float32)
        worst["loss"] = max(worst["loss"], ((l32.double() - l64).abs() / (env.LOSS_ABS + env.LOSS_REL * l64.abs())).item())
        worst["rel"] = max(worst["rel"], (g32.double() - g64).abs().max().item() / g64.abs().max().item())
        worst["block"] = max(worst["block"], max(e for _, e in env.block_metric(h, g32.double(), g64)))
    print(f"{env.shape_id(shape)}: fp32 oracle vs fp64: loss {worst['loss']:.3f} of its tolerance, "
          f"gradient {worst['rel']:.2e}, worst block {worst['block']:.2e}")
    assert SPARE * worst["loss"] <= 1.0
    assert SPARE * worst["rel"] <= env.GRAD_REL
    assert SPARE * worst["block"] <= env.BLOCK_REL


@pytest.mark.parametrize("shape", env.SHAPE_LIST, ids=env.shape_id)
def test_the_fp32_oracle_alone_keeps_the_evaluation_bound_with_room(shape):
    """The GPU bound is 2 x this distance + 1e-5, so the floor decides while the distance stays below 1e-5 / 5."""
    worst_p = worst_s = 0.0
    for p64, s64, p32, s32 in env.eval_references(shape).values():
        worst_p = max(worst_p, (p32.double() - p64).abs().max().item())
        worst_s = max(worst_s, (s32.double() - s64).abs().max().item())
    print(f"{env.shape_id(shape)}: eval fp32 oracle vs fp64: proba {worst_p:.2e} score {worst_s:.2e}")
    assert SPARE * worst_p <= 1e-5 and SPARE * worst_s <= 1e-5


@pytest.mark.parametrize("shape", env.SHAPE_LIST, ids=env.shape_id)
def test_the_edge_rows_are_observable_and_the_bounds_have_teeth(shape):
    """A condition on the inputs, not a measurement: at some case each edge row / column / entry reaches 0.1 of its
    block's largest entry in the fp64 gradient of the loss alone; zeroing it there pushes the gradient test's block
    metric over its bound."""
    data, members, params0 = env.inputs(shape)
    h0 = env.hyper(shape, weight_decay=0.0)
    for name, (share, key) in env.edge_observability(shape).items():
        print(f"{env.shape_id(shape)}: {name}: {share:.3f} of its block at (B, which, epoch, batch, member) = {key}")
        assert share >= 0.1, (name, share)
        rows, lab, _, _ = env.grad_references(shape)[key]
        _, g = O.loss_and_grad(h0, params0[key[4]], data, rows, lab, torch.float64)
        b, idx = env.edge_entries(shape)[name]
        dropped = [t.clone() for t in O.split_params(h0, g)]
        dropped[b][idx] = 0.0
        broken = torch.cat([t.reshape(-1) for t in dropped])
        metric = dict(env.block_metric(h0, broken, g))
        assert max(metric.values()) > env.BLOCK_REL, (name, metric)


@pytest.mark.parametrize("shape", env.SHAPE_LIST, ids=env.shape_id)
def test_the_first_step_members_leave_enough_entries_to_pin(shape):
    """The first-step test pins entries with |g64| > 1e-6 and needs more than 0.3 of all entries: an input condition."""
    data, members, params0 = env.inputs(shape)
    h = env.hyper(shape, batch_size=env.FIRST_STEP_BATCH_SIZE)
    for m in env.FIRST_STEP_MEMBERS:
        rows, lab = O.member_batch(members, m, h, env.SEED, 0, 0)
        _, g64 = O.loss_and_grad(h, params0[m], data, rows, lab, torch.float64)
        share = (g64.abs() > 1e-6).double().mean().item()
        print(f"{env.shape_id(shape)} member {m}: {share:.3f} of the entries have |g64| > 1e-6")
        assert share > 0.3 or (shape, m) in env.FIRST_STEP_LEFT_OUT
