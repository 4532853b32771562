"""SpectralConvEmbedding on the sc_embed HIP kernels: parity with the fp64 oracle (tests/sc_embedding_oracle.py) over a
pairwise-covering set of sizes and grids with n_points on the kernels' edges, the recorded cases of the real sbi class,
the bitwise conditions the fixed orders give, routing, and the module in front of a flow.

Parity bound (output and flat parameter gradient, the bound of tests/test_embedding_nets_gpu.py): the kernel's worst
error against the fp64 oracle is at most 4 x the eager fp32 route's worst error on the same device and inputs, with the
floor 16 * 2^-24 * max|ref|.  Measured figures go to the parity artifact (tests/parity_log.py).

n_points of a case: the assertion's limit modes == n_points // 2 + 1 on an even and an odd grid; 15, 16, 17, 63, 65
(a padded MFMA row tile, exactly one, one + 1, four - 1, four + 1); and the edge of the split of the sums over the
points, a multiple of 4 * parts, and its neighbours.  Combinations the plan refuses (modes > n_points // 2 + 1, or an
LDS image beyond 160 KiB: 32 channels fit with one mode only, since every gradient accumulator lives in LDS) are
not cases: they run eager and there is nothing to compare.

Of the three fixed cases, (1, 1, 4000) on the equispaced grid at the defaults is beyond the LDS limit (the longest
equispaced grid the plan takes at the defaults is 1041 points): it runs eager on both sides, its route is printed and
recorded, and the longest equispaced grid is a case of its own next to the longest grid with positions."""
import copy
import functools
import itertools
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import SpectralConvEmbedding
from sbi_amd.neural_nets.embedding_nets import sc_embedding as S
from tests import parity_log
from tests import sc_embedding_oracle as O

pytestmark = pytest.mark.gpu

BATCHES, IN_CHANNELS, WIDTHS, OUT_CHANNELS = (1, 3, 40), (1, 3), (1, 5, 16, 17, 32), (1, 3)
MODES, LAYERS, GRIDS = (1, 10, 16, 17), (1, 3), ("equispaced", "shared", "per_sample")
EDGES = ("2(M-1)", "2M-1", 15, 16, 17, 63, 65, "split-1", "split", "split+1")
FACTORS = [BATCHES, IN_CHANNELS, WIDTHS, OUT_CHANNELS, MODES, LAYERS, GRIDS, EDGES]
LONGEST = {"equispaced": 1041, "shared": 666}       # at the defaults (include/sbi_amd_sc.h)


@functools.lru_cache(maxsize=None)
def parts_of(cin, width, cout, modes, layers):
    """the number of ranges the plan cuts the points into: a function of (modes, conv_channels)"""
    return S.plan((cin, modes, cout, width, layers), 256, 1, False)[1]


def points_of(case):
    _, cin, width, cout, modes, layers, _, edge = case
    if not isinstance(edge, str):
        return edge
    if edge == "2(M-1)":
        return max(2, 2 * (modes - 1))
    if edge == "2M-1":
        return 2 * modes - 1
    step = 4 * parts_of(cin, width, cout, modes, layers)
    split = step * (2 * modes // step + 2)                # the first edges are below the assertion's limit
    return split + {"split-1": -1, "split": 0, "split+1": 1}[edge]


def dims_of(case):
    _, cin, width, cout, modes, layers, _, _ = case
    return (cin, modes, cout, width, layers)


@functools.lru_cache(maxsize=None)
def planned(case):
    return S.plan(dims_of(case), points_of(case), case[0], case[6] != "equispaced")[0] == 0


def pairwise(factors, allowed=lambda case: True, stride=1):
    """greedy pairwise-covering subset of (every stride-th element of) the product of `factors` (deterministic)."""
    product = [c for c in itertools.product(*factors) if allowed(c)][::stride]
    pairs = [{(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))} for c in product]
    todo = set().union(*pairs)
    chosen = []
    while todo:
        k = max(range(len(product)), key=lambda i: len(pairs[i] & todo))
        chosen.append(product[k])
        todo -= pairs[k]
    return chosen


# (B, in_channels, conv_channels, out_channels, modes, num_layers, grid, edge); test_the_cases_cover_every_pair checks
# that no pair is lost
CASES = pairwise(FACTORS, planned)
FIXED = [
    (600, 1, 5, 1, 10, 3, "equispaced", 64),              # more samples than workgroups
    (1, 1, 5, 1, 10, 3, "equispaced", 4000),              # beyond the LDS limit: eager on both sides (see above)
    (1, 1, 5, 1, 10, 3, "equispaced", LONGEST["equispaced"]),
    (2, 1, 5, 1, 10, 3, "shared", LONGEST["shared"]),     # the longest grid with positions
]


def case_id(c):
    return "-".join(str(v) for v in c)


def spread(net, seed):
    """every parameter moved by 0.2 randn, as the golden tool does"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g, dtype=p.dtype) * (2 ** 0.5 if p.is_complex() else 1.0))
    return net


def make_input(batch, cin, n, grid, g):
    values = torch.randn(batch, cin, n, generator=g) * 1.3 + 0.2
    if grid == "equispaced":
        return values
    if grid == "shared":
        pos = torch.sort(torch.rand(n, generator=g))[0].repeat(batch, cin, 1)
    else:
        pos = (3 * torch.rand(batch, 1, n, generator=g) - 1).repeat(1, cin, 1)       # unsorted, in [-1, 2)
    return torch.stack([values, pos], dim=1)


def parity_inputs(case, seed=0):
    batch, cin, width, cout, modes, layers, grid, _ = case
    torch.manual_seed(seed)
    net = spread(SpectralConvEmbedding(cin, modes=modes, out_channels=cout, conv_channels=width, num_layers=layers),
                 seed)
    g = torch.Generator().manual_seed(1000 + seed)
    x = make_input(batch, cin, points_of(case), grid, g)
    wts = torch.randn(batch, 2 * modes * cout, generator=g)
    return net, x, wts


def worst(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


def check(test, config, what, kernel, eager, ref):
    """the bound of the module docstring for one quantity; prints and records before it asserts"""
    e_k, e_e, scale = worst(kernel, ref), worst(eager, ref), ref.abs().max().item()
    bound = max(4 * e_e, 16 * 2.0**-24 * scale)
    print(f"{test}[{config}] {what}: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e} bound {bound:.3e}")
    parity_log.record(test, f"{config}:{what}", kernel_err=e_k, eager_err=e_e, max_ref=scale,
                      ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= bound, (what, e_k, bound)


def both_routes(net):
    """(kernel-route module on the device, eager twin with the same weights)"""
    net = net.cuda()
    twin = copy.deepcopy(net)
    twin.force_eager = True
    return net, twin


def run_both(net, twin, x, wts, kernel=True):
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        xd = x.cuda()
        assert m.kernel_route(xd)[0] == (name == "kernel" and kernel), m.kernel_route(xd)
        m.zero_grad()
        out = m(xd)
        (out * wts.cuda()).sum().backward()
        got[name] = (out, O.flat_grad(m))
    return got


# ---- parity -----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_every_pair():
    every = set()
    for c in itertools.product(*FACTORS):
        if planned(c):
            every.update((i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c)))
    covered = {(i, c[i], j, c[j]) for c in CASES for i in range(len(c)) for j in range(i + 1, len(c))}
    assert every <= covered, sorted(every - covered, key=str)[:5]
    # every value of every factor is in a case, and no case is long
    assert all({c[i] for c in CASES} == set(f) for i, f in enumerate(FACTORS))
    assert max(points_of(c) for c in CASES) <= 300
    # the split edges are edges: the range length changes between `split` and `split+1`
    for c in CASES:
        if c[7] == "split":
            n, parts = points_of(c), parts_of(*c[1:6])
            assert n % (4 * parts) == 0 and n >= 2 * (c[4] - 1)
    # the fixed cases are what their comments say
    assert [S.plan(dims_of(c), points_of(c), c[0], c[6] != "equispaced")[0] for c in FIXED] == [0, _lib.E_LDS, 0, 0]
    for grid, n in LONGEST.items():
        assert S.plan((1, 10, 1, 5, 3), n + 1, 1, grid != "equispaced")[0] == _lib.E_LDS


@pytest.mark.parametrize("case", CASES + FIXED, ids=case_id)
def test_parity(case):
    config = case_id(case)
    net, x, wts = parity_inputs(case)
    accepted = planned(case)
    got = run_both(*both_routes(net), x, wts, kernel=accepted)
    if not accepted:
        route = net.cuda().kernel_route(x.cuda())
        print(f"sc_parity[{config}] runs eager: {route[1]}")
        parity_log.record("sc_parity", f"{config}:route", kernel=0.0, reason=route[1])
    ref = O.reference(net.state_dict(), x, wts)
    for i, what in enumerate(("forward", "param_grad")):
        check("sc_parity", config, what, got["kernel"][i], got["eager"][i], ref[i])


GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "sc_embedding_reference.pt"), weights_only=False)


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_the_recorded_cases_on_the_kernel_route(name):
    """the recording of the real class is the reference"""
    case = GOLDEN["cases"][name]
    net, twin = both_routes(O.golden_net(SpectralConvEmbedding, case))
    assert net.kernel_route(case["x"].cuda()) == (True, "kernel")
    got = run_both(net, twin, case["x"], case["wts"])
    assert got["kernel"][1].numel() == case["grad_flat"].numel()
    assert all(p.grad.dtype == p.dtype for p in net.parameters())
    for i, (what, ref) in enumerate((("forward", case["out"]), ("param_grad", case["grad_flat"]))):
        check("sc_golden", name, what, got["kernel"][i], got["eager"][i], ref.double())


# ---- bitwise conditions -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bitwise_net(small=True):
    torch.manual_seed(9)
    kw = dict(in_channels=3, modes=6, out_channels=2, conv_channels=17, num_layers=2) if small else dict(in_channels=1)
    return spread(SpectralConvEmbedding(**kw), 9).cuda()


# (small net, B, n_points, grid): a small module; the defaults; more samples than workgroups
BITWISE = ((True, 70, 37, "per_sample"), (False, 5, 200, "equispaced"), (True, 600, 21, "equispaced"),
           (False, 600, 64, "shared"))


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch_size():
    for small, B, n, grid in BITWISE:
        net = bitwise_net(small)
        x = make_input(B, net.in_channels, n, grid, torch.Generator().manual_seed(11)).cuda()
        with torch.no_grad():
            out = net(x)
            assert net.kernel_route(x)[0] and torch.isfinite(out).all() and out.abs().max() > 0
            for i in (0, 2, B // 2, B - 1):
                assert torch.equal(net(x[i:i + 1])[0], out[i]), i
            assert torch.equal(net(x[1:4]), out[1:4])


def test_two_backward_calls_give_identical_gradients():
    for small, B, n, grid in BITWISE:
        net = bitwise_net(small)
        g = torch.Generator().manual_seed(12)
        x = make_input(B, net.in_channels, n, grid, g).cuda()
        wts = torch.randn(B, 2 * net.modes * net.out_channels, generator=g).cuda()
        grads = []
        for _ in range(2):
            net.zero_grad()
            (net(x) * wts).sum().backward()
            grads.append(O.flat_grad(net).clone())
        assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0


@pytest.mark.parametrize("where", ["value", "position"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_value_or_position_stays_in_its_own_row(bad, where):
    net = bitwise_net()
    # sample 8 shares its workgroup with sample 520: the LDS image is rebuilt for every sample
    x = make_input(600, 3, 21, "per_sample", torch.Generator().manual_seed(15))
    holed = x.clone()
    if where == "value":
        holed[8, 0, 1, 13] = bad
    else:
        holed[8, 1, :, 13] = bad
    keep = [i for i in range(600) if i != 8]
    with torch.no_grad():
        out, out_bad = net(x.cuda()), net(holed.cuda())
    assert net.kernel_route(holed.cuda())[0]
    assert torch.isfinite(out).all() and torch.equal(out_bad[keep], out[keep])
    assert not torch.isfinite(out_bad[8]).any()           # every mode sees every point
    # the gradient: the non-finite sample reaches it, and nothing stays behind for the next call
    wts = torch.randn(600, out.shape[1], generator=torch.Generator().manual_seed(16)).cuda()
    grads = []
    for inp in (x, holed, x):
        net.zero_grad()
        (net(inp.cuda()) * wts).sum().backward()
        grads.append(O.flat_grad(net).clone())
    assert torch.isfinite(grads[0]).all() and not torch.isfinite(grads[1]).all() and torch.equal(grads[0], grads[2])


# ---- routing and launch counts ----------------------------------------------------------------------------------------
def test_the_forced_route_launches_no_sc_kernel(monkeypatch):
    x = make_input(17, 3, 37, "shared", torch.Generator().manual_seed(16)).cuda()
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    want = net(x)
    lib = _lib.load()

    def refuse(*args):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(lib, "sbi_amd_sc_forward", refuse)
    monkeypatch.setattr(lib, "sbi_amd_sc_backward", refuse)
    got = twin(x)
    got.sum().backward()
    assert torch.isfinite(O.flat_grad(twin)).all()
    assert (got - want).abs().max() <= 1e-4 * (1 + want.abs().max())
    with pytest.raises(AssertionError, match="about to be launched"):
        net(x)


def test_the_kernel_route_calls_forward_and_backward_once_per_module_call(monkeypatch):
    lib = _lib.load()
    calls = {"forward": 0, "backward": 0}
    fwd, bwd = lib.sbi_amd_sc_forward, lib.sbi_amd_sc_backward

    def count_forward(*args):
        calls["forward"] += 1
        return fwd(*args)

    def count_backward(*args):
        calls["backward"] += 1
        return bwd(*args)

    monkeypatch.setattr(lib, "sbi_amd_sc_forward", count_forward)
    monkeypatch.setattr(lib, "sbi_amd_sc_backward", count_backward)
    for i, (n, layers) in enumerate(((64, 1), (500, 3), (300, 8))):
        net, twin = both_routes(SpectralConvEmbedding(1, num_layers=layers, modes=10 if layers < 8 else 4))
        x = torch.randn(4, 1, n, device="cuda")
        net(x).sum().backward()
        assert calls == {"forward": 2 * i + 1, "backward": i + 1}
        with torch.no_grad():
            net(x)
        assert calls == {"forward": 2 * i + 2, "backward": i + 1}
    twin(x).sum().backward()
    assert calls == {"forward": 6, "backward": 3}


def test_what_the_kernels_do_not_take_runs_eager_and_gives_the_eager_numbers():
    g = torch.Generator().manual_seed(24)
    x = make_input(5, 3, 37, "shared", g).cuda()
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    # an input that requires grad: d/dx exists on the eager route only
    xd = x.clone().requires_grad_(True)
    assert net.kernel_route(xd) == (False, "input requires grad (the kernel backward has no d/dx)")
    out = net(xd)
    out.sum().backward()
    assert torch.equal(out, twin(x)) and torch.isfinite(xd.grad).all() and xd.grad.abs().max() > 0
    with torch.no_grad():
        assert net.kernel_route(xd)[0]          # nothing to differentiate: the kernels take it
    # host tensors and fp64
    host = copy.deepcopy(net).cpu()
    assert host.kernel_route(x.cpu()) == (False, "input is not on a ROCm device")
    assert (host(x.cpu()) - twin(x).cpu()).abs().max() <= 1e-5 * (1 + twin(x).abs().max())
    assert net.kernel_route(x.cpu()) == (False, "input is not on a ROCm device")
    double = copy.deepcopy(net).double()
    assert double.fc0.weight.dtype == torch.float64       # (nn.Module.double() leaves the complex weights complex64)
    assert double.kernel_route(x.double()) == (False, "input is not float32")
    forced = copy.deepcopy(double)
    forced.force_eager = True
    assert torch.equal(double(x.double()), forced(x.double()))
    assert (double(x.double()) - twin(x)).abs().max() <= 1e-5 * (1 + twin(x).abs().max())
    assert double.kernel_route(x) == (False, "parameters are not float32 / complex64 on the input's device")
    # beyond the LDS limit, and beyond the envelope
    for kw, n, reason in ((dict(), 2000, S.plan_reason(_lib.E_LDS)),
                          (dict(modes=65, num_layers=1, conv_channels=2), 200, S.plan_reason(_lib.E_UNSUPPORTED))):
        torch.manual_seed(28)
        big = SpectralConvEmbedding(1, **kw).cuda()
        xl = torch.randn(2, 1, n, generator=g).cuda()
        assert big.kernel_route(xl) == (False, reason)
        forced = copy.deepcopy(big)
        forced.force_eager = True
        out = big(xl)
        out.sum().backward()
        assert torch.equal(out, forced(xl)) and torch.isfinite(O.flat_grad(big)).all()


# ---- module level -----------------------------------------------------------------------------------------------------
def test_the_next_forward_uses_the_new_weights():
    torch.manual_seed(19)
    host = spread(SpectralConvEmbedding(1), 19)
    x = torch.randn(17, 1, 64, generator=torch.Generator().manual_seed(20))
    with torch.no_grad():
        want = host(x)
    close = lambda a, b: (a.cpu() - b.cpu()).abs().max() <= 1e-4 * (1 + b.abs().max())     # noqa: E731
    net = copy.deepcopy(host).to("cuda")
    xd = x.cuda()
    assert net.kernel_route(xd) == (True, "kernel")
    with torch.no_grad():
        assert close(net(xd), want)
    fresh = SpectralConvEmbedding(1).cuda()
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
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    x = make_input(6, 3, 37, "per_sample", torch.Generator().manual_seed(22)).cuda()
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        assert m.kernel_route(x)[0] == (name == "kernel")
        params = list(m.parameters())
        first = torch.autograd.grad(m(x).square().sum(), params, create_graph=True)
        penalty = sum((g.abs() ** 2).sum() for g in first)
        second = torch.autograd.grad(penalty, params, allow_unused=True)
        got[name] = torch.cat([(torch.view_as_real(g) if g.is_complex() else g).reshape(-1)
                               for g in second if g is not None])
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    assert got["kernel"].shape == got["eager"].shape
    # the same formula differentiated twice, once from the kernels' outputs: fp32 rounding apart
    assert (got["kernel"] - got["eager"]).abs().max() <= 1e-3 * got["eager"].abs().max()


def nsf_estimator(seed=20):
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    torch.manual_seed(seed)
    n, T = 256, 48
    theta = torch.randn(n, 2)
    grid = torch.linspace(0, 1, T)
    x = theta[:, :1] * torch.sin(6 * grid) + theta[:, 1:] * torch.cos(6 * grid) + 0.3 * torch.randn(n, T)
    torch.manual_seed(seed + 1)
    return theta, x[:, None], build_nsf(theta, x[:, None], embedding_net=spread(SpectralConvEmbedding(1), seed))


def test_gradients_through_build_nsf_match_the_eager_route():
    theta, x, est = nsf_estimator()
    est = est.to("cuda")
    emb = est.embedding_net[-1]
    assert isinstance(emb, SpectralConvEmbedding)
    seen = {}

    def keep(module, args, output):
        seen["x"] = args[0].detach()
        if output.requires_grad:
            output.register_hook(lambda g: seen.__setitem__("g", g.detach()))

    emb.register_forward_hook(keep)
    got, ref = {}, {}
    for name in ("kernel", "eager"):
        emb.force_eager = name == "eager"
        est.zero_grad()
        seen.clear()
        est.loss(theta.cuda(), x.cuda()).mean().backward()
        assert emb.kernel_route(seen["x"])[0] == (name == "kernel"), emb.kernel_route(seen["x"])
        got[name] = O.flat_grad(emb)
        # fp64 oracle of the embedding alone, driven by the gradient the flow handed back in THIS run
        ref[name] = O.reference(emb.state_dict(), seen["x"], seen["g"])[1]
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    e_k, e_e = worst(got["kernel"], ref["kernel"]), worst(got["eager"], ref["eager"])
    scale = ref["kernel"].abs().max().item()
    print(f"build_nsf sc embedding grads: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e}")
    parity_log.record("sc_through_build_nsf", "256-48", kernel_err=e_k, eager_err=e_e, max_ref=scale,
                      ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= max(4 * e_e, 16 * 2.0**-24 * scale)
