"""The kernel route of ResNetEmbedding1D on the device against the fp64 oracle (tests/resnet_embedding_oracle.py).

Bound, for the trunk output, the module output and the flat parameter gradient: the kernel route's worst error against
the oracle is at most max(4 x the eager fp32 route's worst error on the same device and inputs, 16 * 2^-24 * max|ref|).
Measured figures go to the parity artifact (tests/parity_log.py).  `test_parity` and the recorded 1D cases hold the
gradient to the same bound once more per parameter tensor, with the scale of tests/resnet_envelope.py (`slot_check`).

Kinks.  A ReLU net's gradient jumps where an activation's input crosses 0, and an fp32 route may land on the other side
of one that the oracle sees within rounding of 0.  The rows that `near_kink_rows` returns -- decided by the fp64 oracle
alone, before either route runs -- get grad_out = 0, so their contribution to every parameter gradient is exactly zero
on every route; they still run and still count in the output parity.  No case may zero more than one third of its rows
(asserted); SEEDS holds the seed of every case whose first seed does (checked on the host: none does at present).

Cases: a pairwise-covering set over the plan's edges (rows around the 16-row tile and the MFMA tile, widths that are
and are not multiples of 16, the envelope's ends, with and without the initial Linear), plus fixed cases: the defaults,
more row tiles than workgroups with a partial last tile for each row-tile size (16: not reachable, 4096 rows fill the
grid exactly; 32: 10 000 rows; 64: 16 500 rows, which also takes the split weight-gradient path), 64 blocks, and every
recorded 1D ReLU case.
"""

import copy
import functools
import itertools
import os

import pytest
import torch
from torch import nn

from sbi_amd import _lib
from sbi_amd.neural_nets import ResNetEmbedding1D
from sbi_amd.neural_nets.embedding_nets import resnet as RN
from tests import parity_log
from tests import resnet_embedding_oracle as O

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 33, 65)
C_INTERNAL = (1, 16, 17, 50, 128)
C_HIDDEN = (4, 17, 64, 128)
N_BLOCKS = (1, 2, 3, 20)
C_IN = ("id", 1, 7, 128)
FACTORS = [ROWS, C_INTERNAL, C_HIDDEN, N_BLOCKS, C_IN]


def pairwise(factors):
    """greedy pairwise-covering subset of the product of `factors` (deterministic)."""
    product = list(itertools.product(*factors))
    pairs = [{(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))} for c in product]
    todo = set().union(*pairs)
    chosen = []
    while todo:
        k = max(range(len(product)), key=lambda i: len(pairs[i] & todo))
        chosen.append(product[k])
        todo -= pairs[k]
    return chosen


CASES = pairwise(FACTORS)
DEFAULTS = (40, 128, 128, 20, 10)
FIXED = [
    DEFAULTS,                    # the defaults (head 1000 wide, c_out 8)
    (3000, 17, 20, 2, 3),        # 188 row tiles of 16, the last one partial
    (10000, 17, 20, 2, 3),       # 313 row tiles of 32 on 256 workgroups, the last one partial; 10 row splits
    (16500, 17, 20, 2, 3),       # 258 row tiles of 64 on 256 workgroups, the last one partial; 17 row splits
    (33, 16, 16, 64, "id"),      # the deepest trunk of the envelope
]
# the seed of every case whose seed 0 puts more than one third of its rows within the margin of a kink
SEEDS = {}


def case_id(c):
    return "-".join(str(v) for v in c)


def kwargs_of(case):
    rows, ci, ch, nb, cin = case
    kw = dict(c_in=ci if cin == "id" else cin, c_out=5, n_blocks=nb, c_internal=ci, c_hidden_final=16,
              construct_mapping_kwargs={"c_hidden": ch})
    if case == DEFAULTS:
        kw.update(c_out=8, c_hidden_final=1000)
    return kw


def make(kwargs):
    return ResNetEmbedding1D(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in kwargs.items()})


def spread(net, seed):
    """every parameter moved by 0.05 randn, as the golden tool does"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return net


@functools.lru_cache(maxsize=None)
def draw(case):
    """(net, x, wts with the near-kink rows zeroed, those rows, the oracle's (trunk, out, grad))"""
    seed = SEEDS.get(case_id(case), 0)
    kw = kwargs_of(case)
    torch.manual_seed(seed)
    net = spread(make(kw), seed)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(case[0], kw["c_in"], generator=g) * 1.3 + 0.2
    wts = torch.randn(case[0], kw["c_out"], generator=g)
    near = O.near_kink_rows(net.state_dict(), x, {})
    wts[near] = 0
    return net, x, wts, near, O.reference(net.state_dict(), x, wts, {})


def worst(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


def check(test, config, what, kernel, eager, ref):
    """the bound of the module docstring for one quantity; prints and records before it asserts"""
    e_k, e_e = worst(kernel, ref), worst(eager, ref)
    scale = ref.abs().max().item()
    bound = max(4 * e_e, 16 * 2.0**-24 * scale)
    print(f"{test}[{config}] {what}: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e} bound {bound:.3e}")
    parity_log.record(test, f"{config}:{what}", kernel_err=e_k, eager_err=e_e, max_ref=scale,
                      ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= bound, (what, e_k, bound)


def both_routes(net):
    """(kernel-route module on the device, eager twin with the same weights)"""
    net = copy.deepcopy(net).cuda()
    twin = copy.deepcopy(net)
    twin.force_eager = True
    return net, twin


def run_both(net, twin, x, wts):
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        xd = x.cuda()
        assert m.kernel_route(xd)[0] == (name == "kernel"), m.kernel_route(xd)
        m.zero_grad()
        with torch.no_grad():
            trunk = m.trunk(xd)
        out = m(xd)
        (out * wts.cuda()).sum().backward()
        got[name] = (trunk, out, O.flat_grad(m))
    return got


def parity(test, config, net, x, wts, ref, kwargs=None):
    """`check` for the trunk, the output and the whole flat gradient; with the constructor's `kwargs` also the per-slot
    bound of tests/resnet_envelope.py for the gradient (its scale from the oracle's operands)"""
    from tests import resnet_envelope as env

    got = run_both(*both_routes(net), x, wts)
    for i, what in enumerate(("trunk", "forward", "param_grad")):
        check(test, config, what, got["kernel"][i], got["eager"][i], ref[i])
    if kwargs is not None:
        sd = net.state_dict()
        scale = env.scale_of(sd, O.reference_with_operands(sd, x, wts, {})[3])
        env.slot_check(test, (config, env.sizes_of_kwargs(kwargs)), got["kernel"][2], got["eager"][2], ref[2], scale)


# ---- parity -----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_every_pair():
    every = set()
    for c in itertools.product(*FACTORS):
        every.update((i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c)))
    covered = {(i, c[i], j, c[j]) for c in CASES for i in range(len(c)) for j in range(i + 1, len(c))}
    assert every <= covered, sorted(every - covered, key=str)[:5]
    assert all({c[i] for c in CASES} == set(f) for i, f in enumerate(FACTORS))
    assert len(CASES) <= 60
    tiles = set()
    for c in CASES + FIXED:
        rc, tile, lds, splits = RN.plan(make(kwargs_of(c)).kernel_config(), c[0])
        assert rc == 0, c
        tiles.add((tile, splits > 1))
    # the row tile of every pairwise case is 16, so 15 / 16 / 17 are the tile size and its neighbours
    assert tiles == {(16, False), (16, True), (32, True), (64, True)}
    assert -(-10000 // 32) > 256 and 10000 % 32 and -(-16500 // 64) > 256 and 16500 % 64 and 3000 % 16


@pytest.mark.parametrize("case", CASES + FIXED, ids=case_id)
def test_parity(case):
    net, x, wts, near, ref = draw(case)
    print(f"resnet_parity[{case_id(case)}] rows within the margin of a kink: {len(near)} of {case[0]}")
    assert 3 * len(near) <= case[0], (len(near), case[0])
    parity("resnet_parity", case_id(case), net, x, wts, ref, kwargs_of(case))


GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "resnet_embedding_reference.pt"),
                    weights_only=False)
RELU_1D = sorted(n for n, c in GOLDEN["cases"].items() if c["class"] == "1D" and "activation" not in c["kwargs"])


@pytest.mark.parametrize("name", RELU_1D)
def test_the_recorded_1d_cases_on_the_kernel_route(name):
    c = GOLDEN["cases"][name]
    net = make(c["kwargs"])
    net.load_state_dict(c["state_dict"], strict=True)
    near = O.near_kink_rows(c["state_dict"], c["x"], {})
    assert 3 * len(near) <= c["x"].shape[0]
    wts = c["wts"].clone()
    wts[near] = 0
    parity("resnet_golden", name, net, c["x"], wts, O.reference(c["state_dict"], c["x"], wts, {}), c["kwargs"])
    if not near:        # the recording itself, within the reference's own fp32 error (tests/test_resnet_embedding_cpu.py)
        kernel = both_routes(net)[0]
        out = kernel(c["x"].cuda())
        assert (out.cpu() - c["out"]).abs().max() <= 1024 * 2.0**-24 * c["out"].abs().max()


# ---- bitwise conditions -----------------------------------------------------------------------------------------------
BITWISE = dict(c_in=10, c_out=6, n_blocks=3, c_internal=50, c_hidden_final=24, construct_mapping_kwargs={"c_hidden": 17})


@functools.lru_cache(maxsize=None)
def bitwise_net():
    torch.manual_seed(9)
    return spread(make(BITWISE), 9).cuda()


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch_size():
    net = bitwise_net()
    x = (torch.randn(200, 10, generator=torch.Generator().manual_seed(11)) * 1.3).cuda()
    with torch.no_grad():
        assert net.kernel_route(x)[0]
        trunk = net.trunk(x)
        assert torch.isfinite(trunk).all() and trunk.abs().max() > 0
        alone = net.trunk(x[57:58])[0]
        for place in (0, 100, 199):
            moved = x.clone()
            moved[place] = x[57]
            assert torch.equal(net.trunk(moved)[place], alone), place
        assert torch.equal(net.trunk(x)[57], alone)
        assert torch.equal(torch.cat([net.trunk(x[:77]), net.trunk(x[77:])]), trunk)
        # the other row tiles run the same chain: 5000 rows take 32-row tiles, 17 000 rows 64-row tiles
        for rows in (5000, 17000):
            big = x.repeat(rows // 200, 1)
            assert RN.plan(net.kernel_config(), rows)[1] == (32 if rows == 5000 else 64)
            assert torch.equal(net.trunk(big)[-200:], trunk)


def test_two_backward_calls_give_identical_gradients():
    net = bitwise_net()
    for rows in (200, 5000):
        g = torch.Generator().manual_seed(12)
        x, wts = torch.randn(rows, 10, generator=g).cuda(), torch.randn(rows, 6, generator=g).cuda()
        grads = []
        for _ in range(2):
            net.zero_grad()
            (net(x) * wts).sum().backward()
            grads.append(O.flat_grad(net).clone())
        assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0


# ---- routing ------------------------------------------------------------------------------------------------------------
def test_the_forced_route_launches_no_resnet_kernel(monkeypatch):
    x = torch.randn(5, 10, generator=torch.Generator().manual_seed(16)).cuda()
    net, twin = both_routes(bitwise_net())
    want = net(x)
    lib = _lib.load()

    def refuse(*args):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(lib, "sbi_amd_resnet_forward", refuse)
    monkeypatch.setattr(lib, "sbi_amd_resnet_backward", refuse)
    got = twin(x)
    got.sum().backward()
    assert torch.isfinite(O.flat_grad(twin)).all()
    assert (got - want).abs().max() <= 1e-4 * (1 + want.abs().max())
    with pytest.raises(AssertionError, match="about to be launched"):
        net(x)


def test_what_the_kernels_do_not_take_runs_eager_and_gives_the_eager_numbers():
    g = torch.Generator().manual_seed(24)
    x = torch.randn(5, 10, generator=g).cuda()
    net, twin = both_routes(bitwise_net())
    # an input that requires grad: d/dx exists on the eager route only
    xd = x.clone().requires_grad_(True)
    assert net.kernel_route(xd) == (False, "input requires grad (the kernel backward has no d/dx)")
    out = net(xd)
    out.sum().backward()
    assert torch.equal(out, twin(x)) and torch.isfinite(xd.grad).all() and xd.grad.abs().max() > 0
    with torch.no_grad():
        assert net.kernel_route(xd)[0]
    double = copy.deepcopy(net).double()
    assert double.kernel_route(x.double()) == (False, "input is not float32")
    assert double.kernel_route(x) == (False, "parameters are not float32 on the input's device")
    small = dict(c_in=10, c_out=4, n_blocks=2, c_internal=16, c_hidden_final=8)
    wide_stash = dict(c_in=128, c_out=4, n_blocks=64, c_internal=128, c_hidden_final=8,
                      construct_mapping_kwargs={"c_hidden": 16})
    for kw, rows, reason in (
            (dict(small, activation=nn.Tanh), 5, "activation is not nn.ReLU"),
            (dict(small, construct_mapping=lambda a, b, activation: nn.Sequential(nn.Linear(a, b), activation()),
                  construct_mapping_kwargs={}), 5, "a custom construct_mapping (or kwargs beyond c_hidden) runs eager"),
            (dict(small, c_internal=129), 5, RN.plan_reason(_lib.E_UNSUPPORTED)),
            (dict(small, construct_mapping_kwargs={"c_hidden": 129}), 5, RN.plan_reason(_lib.E_UNSUPPORTED)),
            (dict(small, c_in=129), 5, RN.plan_reason(_lib.E_UNSUPPORTED)),
            (small, 65536, "a call that needs gradients with 65536 >= 65536 rows: eager torch measured faster there "
                           "(profiles/resnet_embed_bench.json)"),
            (wide_stash, 32768, None)):
        torch.manual_seed(28)
        other = make(kw).cuda()
        xo = torch.randn(rows, kw["c_in"], generator=g).cuda()
        took, why = other.kernel_route(xo)
        if reason is None:
            nbytes = RN.workspace_bytes(other.kernel_config(), rows, True)
            assert nbytes > RN.MAX_WORKSPACE_BYTES
            reason = why
            assert why.startswith(f"workspace of {nbytes} bytes passes MAX_WORKSPACE_BYTES = {1 << 30}")
            with torch.no_grad():
                assert other.kernel_route(xo) == (True, "kernel")      # without a stash the call fits
        assert (took, why) == (False, reason)
        if rows == 65536:       # the measured thresholds, one per kind of call; one row fewer takes the kernels
            with torch.no_grad():
                assert other.kernel_route(xo)[1].startswith("a forward-only call with 65536 >= 65536 rows")
            assert (RN.MAX_ROWS_TRAINING, RN.MAX_ROWS_FORWARD) == (65536, 65536)
            assert other.kernel_route(xo[:-1]) == (True, "kernel")
        forced = copy.deepcopy(other)
        forced.force_eager = True
        out = other(xo)
        out.sum().backward()
        assert torch.equal(out, forced(xo)) and torch.isfinite(O.flat_grad(other)).all()


def test_the_next_forward_uses_the_new_weights():
    torch.manual_seed(19)
    host = spread(make(BITWISE), 19)
    x = torch.randn(17, 10, generator=torch.Generator().manual_seed(20))
    with torch.no_grad():
        want = host(x)
    close = lambda a, b: (a.cpu() - b.cpu()).abs().max() <= 1e-4 * (1 + b.abs().max())     # noqa: E731
    net = copy.deepcopy(host).to("cuda")
    xd = x.cuda()
    assert net.kernel_route(xd) == (True, "kernel")
    with torch.no_grad():
        assert close(net(xd), want)
    fresh = make(BITWISE).cuda()
    fresh.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(fresh(xd), net(xd))
    opt = torch.optim.Adam(net.parameters(), lr=0.05)
    net(xd).sum().backward()
    opt.step()
    eager = copy.deepcopy(net)
    eager.force_eager = True
    with torch.no_grad():
        after = net(xd)
        assert not close(after, want) and close(after, eager(xd))


def test_double_backward_differentiates_the_eager_formula():
    net, twin = both_routes(bitwise_net())
    x = torch.randn(6, 10, generator=torch.Generator().manual_seed(22)).cuda()
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        assert m.kernel_route(x)[0] == (name == "kernel")
        params = list(m.parameters())
        first = torch.autograd.grad(m(x).square().sum(), params, create_graph=True)
        penalty = sum((g ** 2).sum() for g in first)
        second = torch.autograd.grad(penalty, params, allow_unused=True)
        got[name] = torch.cat([(g if g is not None else torch.zeros_like(q)).reshape(-1)
                               for g, q in zip(second, params)])
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    assert (got["kernel"] - got["eager"]).abs().max() <= 1e-3 * got["eager"].abs().max()


# ---- through the NSF builder -------------------------------------------------------------------------------------------
NSF_EMB = dict(c_in=10, c_out=8, n_blocks=3, c_internal=32, c_hidden_final=32, construct_mapping_kwargs={"c_hidden": 32})


def test_gradients_through_build_nsf_match_the_eager_route():
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    torch.manual_seed(20)
    theta = torch.randn(256, 2)
    x = theta @ torch.randn(2, 10) + 0.3 * torch.randn(256, 10)
    torch.manual_seed(21)
    est = build_nsf(theta, x, embedding_net=spread(make(NSF_EMB), 20)).to("cuda")
    emb = est.embedding_net[-1]
    assert isinstance(emb, ResNetEmbedding1D)
    seen = {}

    def keep(module, args, output):
        # the rows the oracle sees within the margin of a kink get no gradient, on both routes alike
        seen["x"] = args[0].detach()
        near = O.near_kink_rows(module.state_dict(), seen["x"], {})
        live = torch.ones(output.shape[0], 1, device=output.device)
        live[near] = 0
        seen["near"] = near
        if output.requires_grad:
            output.register_hook(lambda g: seen.__setitem__("g", (g * live).detach()) or g * live)

    emb.register_forward_hook(keep)
    got, ref = {}, {}
    for name in ("kernel", "eager"):
        emb.force_eager = name == "eager"
        est.zero_grad()
        seen.clear()
        est.loss(theta.cuda(), x.cuda()).mean().backward()
        assert seen["x"].shape == x.shape and 3 * len(seen["near"]) <= 256
        assert emb.kernel_route(seen["x"])[0] == (name == "kernel"), emb.kernel_route(seen["x"])
        got[name] = O.flat_grad(emb)
        ref[name] = O.reference(emb.state_dict(), seen["x"], seen["g"], {})[2]
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    e_k, e_e = worst(got["kernel"], ref["kernel"]), worst(got["eager"], ref["eager"])
    scale = ref["kernel"].abs().max().item()
    print(f"build_nsf resnet embedding grads: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e}")
    parity_log.record("resnet_through_build_nsf", "linear_gaussian", kernel_err=e_k, eager_err=e_e, max_ref=scale,
                      ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= max(4 * e_e, 16 * 2.0**-24 * scale)
