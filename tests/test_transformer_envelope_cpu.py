"""Keeps tests/transformer_envelope.py honest, without a device: its slot table against the C ABI's offsets and the
module's parameters, its six LDS images against the plan, the 48 KiB / 64 KiB thresholds the case table is built on,
every GPU case inside the plan and the module's routing limits, and the teeth of the per-slot bound: seeded defects
that the whole-vector bound of tests/test_transformer_embedding_gpu.py lets through and `slot_check` names.

Measured here for the seeded defects (fp32 module on the CPU against the fp64 oracle, `spread(., 0)` weights, case
(B, T, (F, H, KV), I, L) = (3, 65, (72, 4, 4), 64, 3), positional, every key, gelu, features input): the whole-vector
bar, 4 x the eager error over all parameters, is 4.3e-4 and is set by layers.0.input_layernorm.weight (max|ref| 31).
    aggregator.bias x (1 + 3e-5)                   defect 1.0e-4   slot bar 3.2e-6 (the 16-ulp floor at scale 3.4)
    layers.2.input_layernorm.weight x (1 + 5e-5)   defect 1.8e-4   slot bar 4.4e-5
    layers.1.ffn.gate_up_proj.weight, gate and up rows swapped: both slots fail, no other
Layer 2's tensors and norm.weight have slot bars of 1.8e-5 .. 8.8e-5, layer 1's 3.5e-5 .. 1.8e-4, layer 0's 1.6e-4 ..
4.3e-4: the whole-vector bound hid errors 10 (layer 2) to 130 (aggregator.bias) times what a slot allows."""
import functools

import pytest
import torch

from sbi_amd.neural_nets import TransformerEmbedding
from sbi_amd.neural_nets.embedding_nets import transformer as TR
from tests import transformer_embedding_oracle as O
from tests import transformer_envelope as env
from tests.test_transformer_embedding_gpu import check

CASE_IDS = [env.case_id(c) for c in env.ALL_CASES]
KIB = env.KIB


def config_of(case):
    return TransformerEmbedding(**env.kwargs_of(case)).kernel_config(case[8] == "scalar")


def plan_of(case):
    return TR.plan(config_of(case), case[0], case[1])


def tail_case(F, I):
    return env.vary(I=I, heads=(F, 2, 2))


def long_case(T, hd):
    return env.vary(B=1, T=T, heads=(2 * hd, 2, 1), I=4)


@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_slot_table_is_the_flat_image(case):
    sizes = env.sizes_of(case)
    F, H, KV, hd, I, L, E = sizes
    net = TransformerEmbedding(**env.kwargs_of(case))
    tensors = env.tensor_table(sizes)
    named = list(net.named_parameters())
    assert [n for n, _, _, _ in tensors] == [n for n, _ in named] == list(net.state_dict())
    assert [(r, c) if c else (r,) for _, _, r, c in tensors] == [tuple(p.shape) for _, p in named]
    P, offsets = TR.param_count(config_of(case))
    assert P == env.param_count(sizes) == sum(p.numel() for _, p in named)
    assert offsets == [o for _, o, _, _ in tensors] and len(offsets) == 6 * L + 5
    # the slots tile [0, P) in order
    slots = env.slot_table(sizes)
    assert len(slots) == 9 * L + 5 and len({n for n, _, _ in slots}) == len(slots)
    assert slots[0][1] == 0 and slots[-1][2] == P
    assert all(a[2] == b[1] and a[1] < a[2] for a, b in zip(slots, slots[1:]))
    # ... and a split slot holds its own rows: mark the rows of every split tensor, read the flat image back
    marks = {"q": 1.0, "k": 2.0, "v": 3.0, "gate": 4.0, "up": 5.0}
    with torch.no_grad():
        for layer in net.layers:
            w = layer.self_attn.qkv_proj.weight
            w[:H * hd], w[H * hd:(H + KV) * hd], w[(H + KV) * hd:] = marks["q"], marks["k"], marks["v"]
            w = layer.ffn.gate_up_proj.weight
            w[:I], w[I:] = marks["gate"], marks["up"]
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    lengths = {"q": H * hd * F, "k": KV * hd * F, "v": KV * hd * F, "gate": I * F, "up": I * F}
    seen = 0
    for name, lo, hi in slots:
        part = name.rsplit(".", 1)[-1]
        if part in marks:
            assert (flat[lo:hi] == marks[part]).all() and hi - lo == lengths[part], name
            seen += 1
    assert seen == 5 * L


@pytest.mark.parametrize("case", env.ALL_CASES, ids=CASE_IDS)
def test_the_images_are_the_plan_s_and_every_case_is_routed_to_the_kernels(case):
    B, T = case[0], case[1]
    F, H, KV, hd, I, L, E = env.sizes_of(case)
    cfg = config_of(case)
    rc, lds, key_tile, G = TR.plan(cfg, B, T)
    assert rc == 0 and tuple(lds) == env.lds_bytes(case) and key_tile == env.KEY_STEP
    assert max(lds) <= env.LDS_LIMIT_BYTES
    assert G == env.partition(B, T)[2]
    assert B * T * F * L < TR.MAX_TRAINING_WORK
    for training in (False, True):
        assert 0 < TR.workspace_bytes(cfg, B, T, training) < TR.MAX_WORKSPACE_BYTES


def test_the_thresholds_lie_where_the_formulas_say():
    """the last intermediate_size at or under and the first over 48 KiB and 64 KiB of tail-backward LDS at F = 128,
    the last T at and the first over 64 KiB of attention-backward LDS at hd = 2, all through the plan"""
    for limit, last in ((48 * KIB, env.I48), (64 * KIB, env.I64)):
        under, over = plan_of(tail_case(128, last))[1][3], plan_of(tail_case(128, last + 1))[1][3]
        assert under <= limit < over and over - under == 4 * env.TOK * 3, (limit, last, under, over)
        assert (under, over) == (env.tail_backward_bytes(128, last), env.tail_backward_bytes(128, last + 1))
    assert plan_of(tail_case(128, 512))[1][3] == 4 * (8 * (5 * 128 + 3 * 512) + 16) > 64 * KIB
    under, over = plan_of(long_case(env.T64, 2))[1][4], plan_of(long_case(env.T64 + 1, 2))[1][4]
    assert under == 64 * KIB < over == 64 * KIB + 4 * env.WAVES * 2
    # the suite outside this table stays under the default limit in the tail backward (F = 96, I = 256 its largest)
    assert env.tail_backward_bytes(96, 256) <= 48 * KIB
    # the case table is built on them
    assert [c[3] for c, _ in env.INTER_LDS] == [env.I48, env.I48 + 1, env.I64, env.I64 + 1, 512]
    assert all(c[2][0] == 128 for c, _ in env.INTER_LDS)
    assert [c[1] for c, _ in env.LONG_ROWS] == [env.T64, env.T64, env.T64 + 1, env.T64 + 1, 4096, 4096]
    assert all(c[2][0] // c[2][1] == 2 for c, _ in env.LONG_ROWS[:5]) and env.LONG_ROWS[5][0][2] == (4, 1, 1)
    assert all(plan_of(c)[1][4] > 64 * KIB and c[4] == 2 for c, _ in env.LONG_ROWS[2:])


def test_the_case_table_reaches_the_edges_it_names():
    cases = [c for c, _ in env.GPU_CASES + env.PARTITION]
    assert all(why for _, why in env.GPU_CASES + env.PARTITION) and len(set(cases)) == len(cases)
    assert all(c[4] >= 2 for c in cases if c not in (env.LAYERS[0][0],))

    def one_factor(i):
        return {c[i] for c in cases if all(c[j] == env.BASE[j] for j in range(9) if j != i) and len(c) == 9}

    assert one_factor(3) >= {1, 2, 3, 5, 511, 512}
    assert one_factor(4) >= {1, 8}
    assert one_factor(2) >= {(2, 1, 1), (4, 2, 1), (128, 64, 1), (128, 2, 1), (126, 3, 3)}
    finals = {(c[2][0], env.extras_of(c)["final_emb_dimension"]) for c, _ in env.FINAL}
    assert finals == {(36, 1), (36, 2), (36, 35), (36, 36), (128, 128)}
    steps = [c for c, _ in env.STEPS]
    assert [c[1] for c in steps] == [7, 8, 9, 63, 64, 65, 127, 128, 129]
    assert [c[6] for c in steps] == [i % 2 == 0 for i in range(9)]
    assert {(c[5], c[6]) for c in steps} == {(p, c) for p in env.POS for c in (True, False)}
    # the partition: per = ceil(tiles / 256), G = ceil(tiles / per)
    parts = [env.partition(c[0], c[1]) for c, _ in env.PARTITION]
    assert parts == [(256, 1, 256), (257, 2, 129), (512, 2, 256), (513, 3, 171)]
    assert [plan_of(c)[3] for c, _ in env.PARTITION] == [256, 129, 256, 171]
    B, T = env.PARTITION[1][0][:2]
    assert B * T == 2049 and B * T - 256 * env.TOK == 1          # the last tile holds one token
    scalars = [env.extras_of(c) for c, _ in env.SCALARS]
    assert scalars == [{"rms_norm_eps": 1e-2}, {"pos_emb_base": 100.0}, {"zero_sequence": 1}]
    assert [(c[0], c[1], c[3], c[7]) for c, _ in env.RELU] == [(2, 9, 1, "relu"), (2, 9, 512, "relu")]
    assert [env.partition(c[0], c[1])[0] for c in env.ABI_CASES] == [24, 257, 24, 257]
    assert (5 * 37) % env.TOK != 0 and [c[8] for c in env.ABI_CASES] == ["scalar", "scalar", "features", "features"]
    assert [(c[2], c[1], c[6], c[5], p) for c, p in env.DROPOUT] == [((64, 4, 1), 65, False, "positional", 0.5),
                                                                    ((36, 6, 3), 129, True, "rotary", 0.9)]


def test_the_non_default_scalars_reach_the_kernel_config():
    base = config_of(env.BASE)
    eps, div, zero = (config_of(c) for c, _ in env.SCALARS)
    assert abs(base.rms_norm_eps - 1e-5) < 1e-12 and abs(eps.rms_norm_eps - 1e-2) < 1e-9
    hd = 6
    assert [div.div_term[i] for i in range(hd // 2)] == [float(v) for v in TR._frequencies(hd, 100.0)]
    assert [base.div_term[i] for i in range(hd // 2)] == [float(v) for v in TR._frequencies(hd, 10e4)]
    assert zero.scalar_input == 0 and base.scalar_input == 1
    x = env.inputs(env.SCALARS[2][0])[1]
    assert x.shape == (3, 17, 36) and (x[1] == 0).all() and (x[0] != 0).all() and (x[2] != 0).all()
    assert [config_of(c).final_emb_dimension for c, _ in env.FINAL] == [1, 2, 35, 36, 128]


def test_the_peaked_net_is_peaked():
    net, x, _, _ = env.inputs(env.PEAKED)
    plain = env.inputs(env.BASE)[0]
    H, KV, hd = 6, 3, 6
    for a, b in zip(net.layers, plain.layers):
        wa, wb = a.self_attn.qkv_proj.weight, b.self_attn.qkv_proj.weight
        assert torch.equal(wa[:(H + KV) * hd], 3.0 * wb[:(H + KV) * hd]) and torch.equal(wa[(H + KV) * hd:],
                                                                                         wb[(H + KV) * hd:])
    peaks = env.max_score(net, x, env.PEAKED)
    print("peaked attention, fp64 max|S| per layer:", peaks)
    assert len(peaks) == 2 and all(env.PEAKED_SCORES[0] <= s <= env.PEAKED_SCORES[1] for s in peaks)
    assert max(env.max_score(plain, x, env.BASE)) < 10


def test_repeated_batches_are_a_weighted_sum_of_their_distinct_rows():
    case = env.vary(B=40, T=5, heads=(12, 6, 6), I=4)
    net, x, wts, n = env.inputs(case)
    assert n == 17 and torch.equal(x[17:34], x[:17]) and torch.equal(wts[34:], wts[:6])
    out, grad, mag = env.per_sequence(net, x, wts, case, n)
    all_out, all_grad, all_mag = env.per_sequence(net, x, wts, case)
    whole = O.reference(net.state_dict(), x, wts, env.kwargs_of(case))
    assert torch.equal(out, all_out) and (out - whole[0]).abs().max() <= 1e-12 * out.abs().max()
    assert (grad - all_grad).abs().max() <= 1e-12 * mag.max() and (mag - all_mag).abs().max() <= 1e-12 * mag.max()
    assert (grad - whole[1]).abs().max() <= 1e-12 * mag.max()
    assert (mag >= grad.abs() - 1e-12 * mag.max()).all()


# ---- the eager formula alone meets the bound -------------------------------------------------------------------------
def cpu_routes(case):
    """(net, x, wts, distinct, {route: (out, flat gradient)}) in fp32 on the CPU: the module's eager route, which
    also stands in for the kernels"""
    net, x, wts, n = env.inputs(case)
    net.zero_grad()
    out = net(x)
    (out * wts).sum().backward()
    got = {"eager": (out.detach(), O.flat_grad(net).clone())}
    got["kernel"] = got["eager"]
    return net, x, wts, n, got


SMALL = [c for c in env.ALL_CASES if c[1] <= 129 and c[0] <= env.DISTINCT]


@pytest.mark.parametrize("case", SMALL, ids=[env.case_id(c) for c in SMALL])
def test_the_eager_route_alone_passes_every_slot(case):
    """the bound is one the reference computation meets: finite, non-zero figures in every live slot"""
    net, x, wts, n, got = cpu_routes(case)
    out, grad, mag = env.per_sequence(net, x, wts, case, n)
    others = []
    if case[7] == "relu":
        near, others = env.kink_references(net, x, wts, case, n)
        assert near <= 6
    check("tr_envelope_cpu", env.case_id(case), "forward", got["kernel"][0], got["eager"][0], out,
          [o[0] for o in others])
    figures = env.slot_check("tr_envelope_cpu", case, got["kernel"][1], got["eager"][1], grad, mag,
                             others=[o[1] for o in others])
    live = list(figures)[2 if case[8] == "features" else 0:]
    assert all(figures[s]["scale"] > 0 and figures[s]["eager_err"] < 1e-3 * figures[s]["scale"] for s in live)


@pytest.mark.parametrize("case", [c for c, _ in env.RELU], ids=[env.case_id(c) for c, _ in env.RELU])
def test_the_relu_cases_have_few_units_near_a_kink(case):
    net, x, _, _ = env.inputs(case)
    near, candidates = O.kink_candidates(net.state_dict(), x, env.kwargs_of(case))
    print(f"{env.case_id(case)}: {near} pre-activations within the margin of a kink")
    assert near <= 6 and len(candidates) == 2 ** near


# ---- the per-slot bound has teeth ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stand_in():
    """(stand-in kernel gradient, eager gradient, fp64 gradient, sum_b |g_b|) of the seeded-defect case"""
    net, x, wts, n, got = cpu_routes(env.SEEDED)
    _, ref, mag = env.per_sequence(net, x, wts, env.SEEDED, n)
    return got["kernel"][1], got["eager"][1], ref, mag


def test_the_unmodified_stand_in_passes_every_slot_and_the_figures_are_the_ones_written_down():
    kernel, eager, ref, mag = stand_in()
    figures = env.slot_check("tr_envelope_cpu_stand_in", env.SEEDED, kernel, eager, ref, mag)
    check("tr_envelope_cpu_stand_in", env.case_id(env.SEEDED), "param_grad", kernel, eager, ref)
    assert len(figures) == 9 * 3 + 5
    whole_bar = 4 * env.worst(eager, ref)
    bars = {name: f["bound"] for name, f in figures.items() if f["scale"] > 0}
    print(f"whole-vector bar {whole_bar:.3e}; slot bars {min(bars.values()):.3e} .. {max(bars.values()):.3e}")
    # the whole-vector bar is layer 0's; the last layer, the final norm and the aggregator bias sit 8 x and more below
    assert max(bars, key=bars.get).startswith("layers.0.") and max(bars.values()) == whole_bar
    late = [b for name, b in bars.items() if name.startswith(("layers.2.", "norm.", "aggregator."))]
    assert max(late) < whole_bar / 4 and bars["norm.weight"] < whole_bar / 8
    assert bars["aggregator.bias"] == 16 * env.ULP * figures["aggregator.bias"]["scale"] < whole_bar / 100


DEFECTS = [("aggregator.bias", 3e-5), ("layers.2.input_layernorm.weight", 5e-5)]


@pytest.mark.parametrize("slot,relative", DEFECTS, ids=[f"{s}-{r:.0e}" for s, r in DEFECTS])
def test_a_seeded_defect_passes_the_whole_vector_bound_and_fails_only_its_slot(slot, relative):
    kernel, eager, ref, mag = stand_in()
    lo, hi = {name: (a, b) for name, a, b in env.slot_table(env.sizes_of(env.SEEDED))}[slot]
    broken = kernel.clone()
    broken[lo:hi] *= 1 + relative
    defect = (broken - kernel).abs().max().item()
    whole_bar = 4 * env.worst(eager, ref)
    good = env.slot_figures(env.sizes_of(env.SEEDED), kernel, eager, ref, mag)[slot]
    print(f"{slot} x (1 + {relative:.0e}): defect {defect:.3e}, whole-vector bar {whole_bar:.3e}, "
          f"slot bar {good['bound']:.3e}")
    assert defect > 2 * good["bound"] + good["kernel_err"]
    assert defect + env.worst(kernel, ref) < whole_bar
    check("tr_envelope_cpu_defect", env.case_id(env.SEEDED), slot, broken, eager, ref)
    with pytest.raises(AssertionError) as e:
        env.slot_check("tr_envelope_cpu_defect", env.SEEDED, broken, eager, ref, mag, tag=f"{slot}x{relative:.0e}")
    assert list(e.value.args[0][1]) == [slot], e.value.args[0][1]


def test_swapped_gate_and_up_rows_fail_exactly_those_two_slots():
    kernel, eager, ref, mag = stand_in()
    table = {name: (a, b) for name, a, b in env.slot_table(env.sizes_of(env.SEEDED))}
    gate, up = (table[f"layers.1.ffn.gate_up_proj.weight.{part}"] for part in ("gate", "up"))
    assert gate[1] == up[0] and gate[1] - gate[0] == up[1] - up[0]
    broken = kernel.clone()
    broken[gate[0]:gate[1]], broken[up[0]:up[1]] = kernel[up[0]:up[1]], kernel[gate[0]:gate[1]]
    with pytest.raises(AssertionError) as e:
        env.slot_check("tr_envelope_cpu_defect", env.SEEDED, broken, eager, ref, mag, tag="gate_up_swapped")
    assert list(e.value.args[0][1]) == ["layers.1.ffn.gate_up_proj.weight.gate", "layers.1.ffn.gate_up_proj.weight.up"]


def test_a_leak_into_the_scalar_projection_of_a_features_input_fails():
    kernel, eager, ref, mag = stand_in()
    broken = kernel.clone()
    broken[3] = 1e-30
    with pytest.raises(AssertionError) as e:
        env.slot_check("tr_envelope_cpu_defect", env.SEEDED, broken, eager, ref, mag, tag="scalar_projection_leak")
    assert len(e.value.args[0][1]) == 2 and all("scalar_projection.weight" in k for k in e.value.args[0][1])
