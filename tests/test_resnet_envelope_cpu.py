"""Keeps tests/resnet_envelope.py honest, without a device: its slot table against the C ABI's offsets and the module's
state_dict, its restated plan against `sbi_amd_resnet_plan` and `sbi_amd_resnet_workspace_bytes`, every property the
case table's reasons claim, the kink share of every case, the outer-product scale against per-row autograd, and the
teeth of the per-slot bound: seeded defects that the flat bound of tests/test_resnet_embedding_gpu.py (`check` over
the whole gradient) lets through and `slot_check` names.

Measured here for the seeded defects (the fp32 module on the CPU stands in for the kernels, against the fp64 oracle):
  (1025, 15, 31, 2, 3): flat bound 6.1e-5, set by the head (final.4.bias: scale 8.3e2); the trunk's slots get 6.2e-6
  (blocks.0.f.0.weight) to 5.3e-5 (blocks.1.f.4.bias) alone, blocks.0.f.0.bias 7.6e-6, blocks.0.f.2.weight 9.8e-6.
    the last real row missing from blocks.0.f.0.bias       defect 3.0e-2: the flat bound rejects it too
    the same at 2^-9 of the row                            defect 5.8e-5: flat passes, the slot fails
    the last split (512 of 1088 rows) missing from blocks.0.f.2.weight   defect 5.7e-1: the flat bound rejects it too
    the same at 2^-14 of the split's partial               defect 3.5e-5: flat passes, the slot fails
  (33, 16, 16, 64, "id"): flat bound 1.2e-5, blocks.0.f.0.bias alone 2.6e-7 (46 times less);
    blocks.0.f.0.bias x (1 + 2^-14)                        defect 7.2e-6: flat passes, the slot fails
At these widths one whole row or split is far above either bound; what the flat bound let through is anything up to 8
(1025 rows) or 46 (64 blocks) times what the tensor's own figures allow.  The power of two of every scaled defect is
found by the test: the largest that still passes the flat bound."""
import functools

import pytest
import torch

from sbi_amd.neural_nets.embedding_nets import resnet as RN
from tests import resnet_embedding_oracle as O
from tests import resnet_envelope as env
from tests.test_resnet_embedding_gpu import check, make

CASE_IDS = [env.case_id(c) for c in env.ALL_CASES]
GPU = {c: why for c, why in env.GPU_CASES}


def config_of(case):
    return make(env.kwargs_of(case)).kernel_config()


# ---- the slot table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_slot_table_is_the_flat_gradient(case):
    sizes = env.sizes_of(case)
    cin, ci, ch, nb, hf, cout = sizes
    net = make(env.kwargs_of(case))
    tensors = env.tensor_table(sizes)
    named = list(net.named_parameters())
    assert [n for n, _, _, _ in tensors] == [n for n, _ in named] == list(net.state_dict())
    assert [(r, c) if c else (r,) for _, _, r, c in tensors] == [tuple(p.shape) for _, p in named]
    assert env.param_count(sizes) == sum(p.numel() for _, p in named)
    # the trunk's tensors in the kernels' own order: the ABI's offsets, and the parameters the module hands over
    trunk = env.trunk_table(sizes)
    P, offsets = RN.param_count(config_of(case))
    lengths = [r * max(c, 1) for _, r, c in trunk]
    assert len(trunk) == len(offsets) == 6 * nb + (2 if cin != ci else 0)
    assert offsets == [sum(lengths[:i]) for i in range(len(trunk))] and P == sum(lengths) == env.plan_of(case)[
        "trunk_params"]
    by_id = {id(p): n for n, p in named}
    assert [by_id[id(p)] for p in net.kernel_parameters()] == [n for n, _, _ in trunk]
    # the slots tile [0, P) in order, the head's six among them
    slots = env.slot_table(sizes)
    assert len(slots) == len(trunk) + 6 and len({n for n, _, _ in slots}) == len(slots)
    assert slots[0][1] == 0 and slots[-1][2] == env.param_count(sizes)
    assert all(a[2] == b[1] and a[1] < a[2] for a, b in zip(slots, slots[1:]))
    assert sum(n.startswith("final.") for n, _, _ in slots) == 6
    # ... and every slot holds its own tensor: mark each, read the flat vector back in `flat_grad`'s order
    for i, (_, p) in enumerate(named):
        p.grad = torch.full_like(p, float(i + 1))
    flat = O.flat_grad(net)
    for i, (name, lo, hi) in enumerate(slots):
        assert (flat[lo:hi] == i + 1).all(), name


# ---- the plan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_restated_plan_is_the_plan(case):
    p = env.plan_of(case)
    cfg = config_of(case)
    rc, tile, lds, splits = RN.plan(cfg, case[0])
    assert rc == 0 and (tile, splits) == (p["tile"], p["S"]) and lds == [p["lds_bytes"]] * 2
    assert lds[0] <= 160 * 1024
    assert RN.workspace_bytes(cfg, case[0], False) == 4 * p["workspace_floats"][0]
    assert RN.workspace_bytes(cfg, case[0], True) == 4 * p["workspace_floats"][1] < RN.MAX_WORKSPACE_BYTES
    # what the restatement adds to the ABI's answers hangs together
    assert p["Rp"] % 64 == 0 and 0 <= p["Rp"] - case[0] < 64 and p["Rp"] % p["tile"] == 0
    assert p["chunk"] % 64 == 0 and (p["S"] - 1) * p["chunk"] < p["Rp"] <= p["S"] * p["chunk"]
    assert p["last_split"] % 64 == 0 and 0 < p["last_split"] <= p["chunk"] and p["S"] <= env.MAX_SPLITS
    assert p["panel_rows"] == (32 if p["tile"] == 64 else 64)
    for k, (count, last) in p["panels"].items():
        assert (count - 1) * p["panel_rows"] + last == p["widths"][k] and 0 < last <= p["panel_rows"] and last % 16 == 0
    if case in GPU:      # the module sends it to the kernels
        assert case[0] < RN.MAX_ROWS_TRAINING and case[0] < RN.MAX_ROWS_FORWARD


# every property the reasons of the table claim, from the restatement
CLAIMS = {
    (4096, 5, 3, 2, 2): dict(tile=16, tiles=256, tiles_per_workgroup=1, S=4, last_split=1024),
    (4097, 113, 97, 2, 65): dict(tile=32, panel_rows=64, widths={"CI": 128, "CH": 112, "CN": 80},
                                 panels={"CI": (2, 64), "CH": (2, 48), "CN": (2, 16)}),
    (16384, 33, 65, 2, "id"): dict(tile=32, tiles=512, tiles_per_workgroup=2, widths={"CI": 48, "CH": 80},
                                   panels={"CI": (1, 48), "CH": (2, 16)}),
    (16385, 97, 33, 2, 17): dict(tile=64, tiles=257, tiles_per_workgroup=2, real_rows_last_tile=1, panel_rows=32,
                                 widths={"CI": 112, "CH": 48, "CN": 32},
                                 panels={"CI": (4, 16), "CH": (2, 16), "CN": (1, 32)}, S=17, chunk=1024, last_split=64),
    (16385, 128, 128, 1, "id"): dict(tile=64, panel_rows=32, widths={"CI": 128, "CH": 128},
                                     panels={"CI": (4, 32), "CH": (4, 32)}, real_rows_last_tile=1),
    (1024, 15, 31, 2, 3): dict(S=1, chunk=1024),
    (1025, 15, 31, 2, 3): dict(S=2, chunk=576, last_split=512, Rp=1088),
    (2048, 17, 4, 3, "id"): dict(S=2, chunk=1024, last_split=1024),
    (2049, 17, 4, 3, "id"): dict(S=3, chunk=704, last_split=704),
    (65535, 3, 5, 2, 2): dict(tile=64, S=64, chunk=1024, last_split=1024, tiles_per_workgroup=4),
    (64, 127, 112, 2, 113): dict(tile=16, widths={"CI": 128, "CH": 112, "CN": 128},
                                 panels={"CI": (2, 64), "CH": (2, 48), "CN": (2, 64)}),
    (63, 112, 113, 2, 127): dict(tile=16, widths={"CI": 112, "CH": 128, "CN": 128},
                                 panels={"CI": (2, 48), "CH": (2, 64), "CN": (2, 64)}),
    (65, 64, 65, 3, 63): dict(tile=16, widths={"CI": 64, "CH": 80, "CN": 64},
                              panels={"CI": (1, 64), "CH": (2, 16), "CN": (1, 64)}),
    (16, 65, 64, 3, "id"): dict(tile=16, widths={"CI": 80, "CH": 64}, panels={"CI": (2, 16), "CH": (1, 64)}),
    (17, 80, 81, 2, 79): dict(tile=16, widths={"CI": 80, "CH": 96, "CN": 80},
                              panels={"CI": (2, 16), "CH": (2, 32), "CN": (2, 16)}),
    (1, 128, 128, 64, 128): dict(tile=16, S=1, widths={"CI": 128, "CH": 128}, panels={"CI": (2, 64), "CH": (2, 64)}),
    (2, 1, 1, 64, "id"): dict(tile=16, S=1, widths={"CI": 16, "CH": 16}),
    # the ABI cases
    (200, 50, 17, 3, 10): dict(tile=16, S=1, Rp=256),
    (65537, 3, 5, 2, 2): dict(tile=64, Rp=65600, S=61, chunk=1088, last_split=320, real_rows_last_tile=1),
    (131072, 3, 5, 2, 2): dict(tile=64, S=64, chunk=2048, last_split=2048),
}


def test_the_case_table_reaches_the_edges_it_names():
    cases = [c for c, _ in env.GPU_CASES]
    assert all(why for _, why in env.GPU_CASES) and len(set(cases)) == len(cases) == 17
    assert set(CLAIMS) == set(cases) | set(env.ABI_CASES)
    for case, claims in CLAIMS.items():
        p = env.plan_of(case)
        assert {k: p[k] for k in claims} == claims, (case, {k: p[k] for k in claims})
    # both sides of every threshold of the plan
    rows = {c[0] for c in cases}
    assert rows >= {4096, 4097, 16384, 16385, 1024, 1025, 2048, 2049, 65535}
    assert (env.plan_of((4096, 5, 3, 2, 2))["tile"], env.plan_of((4097, 5, 3, 2, 2))["tile"]) == (16, 32)
    assert (env.plan_of((16384, 5, 3, 2, 2))["tile"], env.plan_of((16385, 5, 3, 2, 2))["tile"]) == (32, 64)
    assert RN.MAX_ROWS_TRAINING == 65536 and env.plan_of((65535, 3, 5, 2, 2))["Rp"] // env.SPLIT_ROWS == env.MAX_SPLITS
    # the cap of the splits is reachable only through the ABI: uncapped, 65 600 rows would take 65 splits
    assert -(-65600 // env.SPLIT_ROWS) == 65 > env.MAX_SPLITS and env.ABI_CASES[2][0] > RN.MAX_ROWS_TRAINING
    assert env.plan_of(env.ABI_CASES[3])["chunk"] > env.SPLIT_ROWS
    # more than one panel with a short last one at every tile size, in the forward's K (CI, CH) and the delta pass's
    short = {(env.plan_of(c)["tile"]) for c in cases
             if any(n > 1 and last < env.plan_of(c)["panel_rows"] for n, last in env.plan_of(c)["panels"].values())}
    assert short == {16, 32, 64}
    # the module routes the first two ABI cases to the kernels, the other two only the ABI reaches
    assert [c[0] < RN.MAX_ROWS_TRAINING for c in env.ABI_CASES] == [True, True, False, False]
    assert 4 * env.plan_of(env.ABI_CASES[3])["workspace_floats"][1] < 80e6


# ---- kinks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_no_case_zeroes_more_than_a_third_of_its_rows(case):
    net, x, wts, near, ref, scale = env.draw(case)
    print(f"{env.case_id(case)}: {len(near)} of {case[0]} rows within the margin of a kink")
    assert 3 * len(near) <= case[0]
    assert (wts[near] == 0).all() and (wts != 0).any()


@pytest.mark.parametrize("variant", ["unit", "stream"])
def test_the_dead_unit_nets_are_dead_where_the_table_says(variant):
    net, x, wts, near, ref, scale, zero = env.dead_unit_net(variant)
    print(f"dead {variant}: {len(near)} of {x.shape[0]} rows within the margin of a kink")
    assert 3 * len(near) <= x.shape[0]
    sizes = env.sizes_of(env.DEAD_UNIT)
    eager = cpu_gradient(net, x, wts)
    figures = env.slot_check("resnet_envelope_cpu_dead", env.DEAD_UNIT, eager, eager, ref[2], scale, tag=variant,
                             exact_zero=zero)
    assert len(zero) == (3 if variant == "unit" else 14)
    for what, lo, hi, step in zero:
        assert (ref[2][lo:hi:step] == 0).all() and (scale[lo:hi:step] == 0).all(), what
    # the rest of the net is alive: block 2 and the head everywhere, and in "unit" the other rows of the same tensors
    alive = [n for n in figures if n.startswith(("final.", "blocks.2.")) and n != "blocks.2.f.0.weight"]
    alive += [n for n in figures if variant == "unit"]
    assert alive and all(figures[n]["scale"] > 0 for n in alive)
    assert ref[0].abs().max() > 0
    # a leak of one float into a dead range fails
    broken = eager.clone()
    broken[zero[0][1]] = 1e-30
    with pytest.raises(AssertionError) as e:
        env.slot_check("resnet_envelope_cpu_dead", env.DEAD_UNIT, broken, eager, ref[2], scale, tag=variant + ":leak",
                       exact_zero=zero)
    # (a slot that is dead as a whole has bound 0 and fails by its figures as well)
    whole = [zero[0][0]] if variant == "stream" else []
    assert list(e.value.args[0][1]) == whole + [f"{zero[0][0]} (kernel route, not exactly zero)"]


# ---- the scale -------------------------------------------------------------------------------------------------------
def test_the_outer_product_scale_is_the_sum_of_the_per_row_gradients_magnitudes():
    net, x, wts, near, ref, scale = env.draw(env.SCALE_CASE)
    sd = net.state_dict()
    rows = [O.reference(sd, x[r:r + 1], wts[r:r + 1], {})[2] for r in range(x.shape[0])]
    total, mag = sum(rows), sum(g.abs() for g in rows)
    assert (mag > 0).sum() > mag.numel() // 2 and (scale - mag).abs().max() <= 1e-13 * mag.max()
    assert (total - ref[2]).abs().max() <= 1e-13 * mag.max()
    assert (scale >= ref[2].abs() - 1e-13 * mag.max()).all() and (scale > 2 * ref[2].abs()).any()
    # one row: the scale is |ref|
    one = env.draw((1, 128, 128, 64, 128))
    assert (one[5] - one[4][2].abs()).abs().max() <= 1e-13 * one[5].max()


# ---- the eager formula alone meets the bound -------------------------------------------------------------------------
def cpu_gradient(net, x, wts):
    """the flat fp32 gradient of the module's eager route on the host, which also stands in for the kernels"""
    net.zero_grad()
    (net(x) * wts).sum().backward()
    return O.flat_grad(net).clone()


@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_eager_route_alone_passes_every_slot(case):
    """the bound is one the reference computation meets: finite, non-zero figures in every slot"""
    net, x, wts, near, ref, scale = env.draw(case)
    eager = cpu_gradient(net, x, wts)
    figures = env.slot_check("resnet_envelope_cpu", case, eager, eager, ref[2], scale)
    sizes = env.sizes_of(case)
    assert len(figures) == 6 * case[3] + (0 if sizes[0] == sizes[1] else 2) + 6
    dead = [n for n, f in figures.items() if f["scale"] == 0]
    print(f"{env.case_id(case)}: {len(dead)} slots without any gradient")
    assert all(f["eager_err"] <= 1e-3 * f["scale"] for f in figures.values())
    # one unit wide and 64 blocks deep, the stream dies on the way: only the head and the last blocks carry a gradient,
    # and everything before has to be exactly zero on the kernel route (bound 0)
    assert not dead or (case == (2, 1, 1, 64, "id") and not any(n.startswith("final.") for n in dead))


# ---- the per-slot bound has teeth ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stand_in(case):
    """(stand-in kernel gradient = eager gradient, fp64 gradient, scale)"""
    net, x, wts, near, ref, scale = env.draw(case)
    return cpu_gradient(net, x, wts), ref[2], scale


def seed(case, slot, missing, first_k, tag):
    """`missing` (fp64, the slot's length) times 2^-k taken out of the stand-in's slot, k = first_k, first_k + 1, ...:
    every k whose defect the flat bound rejects is asserted to be rejected; the first that passes it (the real `check`
    of tests/test_resnet_embedding_gpu.py) has to fail `slot_check` in exactly that slot.  Returns that k."""
    kernel, ref, scale = stand_in(case)
    sizes = env.sizes_of(case)
    lo, hi = {n: (a, b) for n, a, b in env.slot_table(sizes)}[slot]
    flat = env.flat_bound(kernel, ref)
    good = env.slot_figures(sizes, kernel, kernel, ref, scale)[slot]
    for k in range(first_k, 40):
        broken = kernel.clone()
        broken[lo:hi] -= (2.0**-k * missing).float()
        defect = (broken - kernel).abs().max().item()
        print(f"{tag} x 2^-{k}: defect {defect:.3e}, flat bound {flat:.3e}, slot bound {good['bound']:.3e}")
        if env.worst(broken, ref) > flat:
            with pytest.raises(AssertionError):
                check("resnet_envelope_cpu_defect", env.case_id(case), f"{tag}:2^-{k}", broken, kernel, ref)
            continue
        check("resnet_envelope_cpu_defect", env.case_id(case), f"{tag}:2^-{k}", broken, kernel, ref)
        with pytest.raises(AssertionError) as e:
            env.slot_check("resnet_envelope_cpu_defect", case, broken, kernel, ref, scale, tag=f"{tag}:2^-{k}")
        assert list(e.value.args[0][1]) == [slot], e.value.args[0][1]
        return k
    raise AssertionError("no power of two of the defect passes the flat bound")


def test_the_unmodified_stand_ins_pass_and_the_flat_bound_is_the_head_s():
    for case in (env.SEEDED_ROWS, env.SEEDED_DEEP):
        kernel, ref, scale = stand_in(case)
        figures = env.slot_check("resnet_envelope_cpu_stand_in", case, kernel, kernel, ref, scale)
        check("resnet_envelope_cpu_stand_in", env.case_id(case), "param_grad", kernel, kernel, ref)
        flat = env.flat_bound(kernel, ref)
        trunk = {n: f["bound"] for n, f in figures.items() if not n.startswith("final.")}
        print(f"{env.case_id(case)}: flat bound {flat:.3e}; the trunk's slots {min(trunk.values()):.3e} .. "
              f"{max(trunk.values()):.3e}")
        # the median trunk tensor's own bound is several times below the flat one
        assert sorted(trunk.values())[len(trunk) // 2] < flat / 3
    assert flat / figures["blocks.0.f.0.bias"]["bound"] > 20          # the 64-block case


def test_a_missing_last_row_fails_the_bias_slot_of_block_0():
    case, slot = env.SEEDED_ROWS, "blocks.0.f.0.bias"
    net, x, wts, near, ref, scale = env.draw(case)
    last = case[0] - 1
    assert last == 1024 and last not in near and env.plan_of(case)["real_rows_last_tile"] == 1
    d = O.reference_with_operands(net.state_dict(), x, wts, {})[3]["blocks.0.f.0"][1]
    assert d[last].abs().max() > 0
    k = seed(case, slot, d[last], 0, "last_row_missing")
    assert k > 0           # the whole row is rejected by the flat bound too; a 2^-k share of it is not


def test_a_missing_last_split_fails_the_weight_slot_of_block_0():
    case, slot = env.SEEDED_ROWS, "blocks.0.f.2.weight"
    net, x, wts, near, ref, scale = env.draw(case)
    p = env.plan_of(case)
    assert (p["S"], p["chunk"], p["last_split"]) == (2, 576, 512)
    lo, hi = {n: (a, b) for n, a, b in env.slot_table(env.sizes_of(case))}[slot]
    first_split = O.reference(net.state_dict(), x[:576], wts[:576], {})[2]        # the defective value
    k = seed(case, slot, ref[2][lo:hi] - first_split[lo:hi], 0, "last_split_missing")
    assert k > 0


def test_a_relative_defect_in_the_deepest_trunk_fails_the_bias_slot_of_block_0():
    case, slot = env.SEEDED_DEEP, "blocks.0.f.0.bias"
    kernel, ref, scale = stand_in(case)
    lo, hi = {n: (a, b) for n, a, b in env.slot_table(env.sizes_of(case))}[slot]
    k = seed(case, slot, -kernel[lo:hi].double(), 1, "bias_times_1_plus")
    print(f"blocks.0.f.0.bias x (1 + 2^-{k}) is the largest step the flat bound passes")
    assert k <= 16         # wrong in its fifth digit, and the flat bound passed it
