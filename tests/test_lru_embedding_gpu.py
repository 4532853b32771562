"""LRUEmbedding on the lru_embed HIP kernels: parity with the fp64 oracle (tests/lru_embedding_oracle.py) over a
pairwise-covering set of sizes, the recorded cases of the real sbi class, the bitwise conditions the fixed orders give,
routing, and the module in front of a flow.

Parity bound (features and flat real-view parameter gradient, the bound of tests/test_embedding_nets_gpu.py): the
kernel's worst error against the fp64 oracle is at most 4 x the eager fp32 route's worst error on the same device and
inputs, with the floor 16 * 2^-24 * max|ref|.  test_parity holds its gradient to the same bound once more in every
parameter slot on its own (tests/lru_envelope.py, `slot_check`).  Measured figures go to the parity artifact
(tests/parity_log.py)."""
import copy
import functools
import itertools
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import LRUEmbedding
from sbi_amd.neural_nets.embedding_nets import lru as L
from tests import lru_embedding_oracle as O
from tests import lru_envelope, parity_log

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 15, 16, 17, 33, 64, 65)      # one step, either side of a 16-step tile, several tiles
BATCHES, INPUT_DIMS, HIDDEN, STATES = (1, 17, 70), (1, 3), (8, 40, 72), (3, 20, 33)
AGGREGATIONS = ("mean", "last_step")


def pairwise(factors, allowed=lambda case: True):
    """greedy pairwise-covering subset of the product of `factors` (deterministic)."""
    product = [c for c in itertools.product(*factors) if allowed(c)]
    pairs = [{(i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c))} for c in product]
    todo = set().union(*pairs)
    chosen = []
    while todo:
        k = max(range(len(product)), key=lambda i: len(pairs[i] & todo))
        chosen.append(product[k])
        todo -= pairs[k]
    return chosen


# (T, B, input_dim, hidden_dim, state_dim, bidirectional, num_blocks, aggregation)
CASES = pairwise([STEPS, BATCHES, INPUT_DIMS, HIDDEN, STATES, (True, False), (1, 2, 3), AGGREGATIONS])
CASES.append((16, 600, 1, 8, 3, True, 1, "mean"))        # a launch has at most 512 workgroups: more than one pass
CASES.append((1000, 3, 1, 40, 20, True, 2, "mean"))      # default sizes: the carried state crosses 63 tiles


def case_id(c):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def make_net(case):
    _, _, input_dim, hidden, state, bidir, blocks, agg = case
    return LRUEmbedding(input_dim, 5, state_dim=state, hidden_dim=hidden, num_blocks=blocks, bidirectional=bidir,
                        aggregate_fcn=agg)


def spread(net, seed):
    """every parameter moved by 0.2 randn (complex noise for B and C), as the golden tool does"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            noise = torch.randn(p.shape, generator=g)
            if p.is_complex():
                noise = torch.complex(noise, torch.randn(p.shape, generator=g))
            p.add_(0.2 * noise)
    return net


def parity_inputs(case, seed=0):
    torch.manual_seed(seed)
    net = spread(make_net(case), seed)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(case[1], case[0], case[2], generator=g) * 1.3 + 0.2
    wts = torch.randn(case[1], case[3], generator=g)
    return net, x, wts


def oracle(net, x, wts):
    """fp64 (features, flat gradient of sum(wts * features) over the kernel parameters)"""
    d = net.dims
    _, features, grad = O.reference(net.state_dict(), x, wts, d[2], bool(d[4]), AGGREGATIONS[d[5]], through="features")
    return features, grad


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


def kernel_grad(net):
    return L.flat_image([p.grad for p in net.kernel_parameters()])


def both_routes(net):
    """(kernel-route module on the device, eager twin with the same weights)"""
    net = net.cuda()
    twin = copy.deepcopy(net)
    twin.force_eager = True
    return net, twin


def run_both(net, twin, x, wts):
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        xd = x.cuda()
        assert m.kernel_route(xd)[0] == (name == "kernel"), m.kernel_route(xd)
        m.zero_grad()
        out = m.features(xd)
        (out * wts.cuda()).sum().backward()
        got[name] = (out, kernel_grad(m))
    return got


# ---- parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity(case):
    config = case_id(case)
    net, x, wts = parity_inputs(case)
    ref = oracle(net, x, wts)
    got = run_both(*both_routes(net), x, wts)
    for i, what in enumerate(("forward", "param_grad")):
        check("lru_parity", config, what, got["kernel"][i], got["eager"][i], ref[i])
    if case[1] <= max(BATCHES):
        # the gradient slot by slot (tests/lru_envelope.py); the 600 distinct sequences of the grid-wrap case would be
        # 600 oracle calls, it keeps the whole-vector bound alone
        _, _, per_seq_abs = lru_envelope.per_sequence(net, x, wts)
        lru_envelope.slot_check("lru_parity_slots", case, got["kernel"][1], got["eager"][1], ref[1], per_seq_abs)


GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "lru_embedding_reference.pt"), weights_only=False)
KERNEL_CASES = sorted(n for n, c in GOLDEN["cases"].items() if not c["kwargs"].get("apply_input_normalization"))


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_the_recorded_cases_on_the_kernel_route(name):
    """the recording of the real class is the reference: features, and the gradient of the recorded loss through the
    (fp32) output layer"""
    case = GOLDEN["cases"][name]
    net = LRUEmbedding(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    net, twin = both_routes(net)
    got = {}
    for key, m in (("kernel", net), ("eager", twin)):
        xd = case["x"].cuda()
        assert m.kernel_route(xd)[0] == (key == "kernel")
        m.zero_grad()
        features = m.features(xd)
        out = m.output_layer(features)
        (out * case["wts"].cuda()).sum().backward()
        got[key] = (features, L.flat_image([p.grad for p in m.parameters()]), out)
    n = case["grad_flat"].numel()
    assert got["kernel"][1].numel() == n
    for i, (what, ref) in enumerate((("forward", case["features"]), ("param_grad", case["grad_flat"]),
                                     ("out", case["out"]))):
        check("lru_golden", name, what, got["kernel"][i], got["eager"][i], ref.double())


def test_the_layer_norm_case_runs_eager_and_matches_the_recording():
    case = GOLDEN["cases"]["layer_norm"]
    net = LRUEmbedding(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    net = net.cuda()
    assert net.kernel_route(case["x"].cuda()) == (False, "apply_input_normalization (no layer norm in the kernels)")
    with torch.no_grad():
        out = net(case["x"].cuda())
    assert (out.cpu() - case["out"]).abs().max() <= 1e-5 * (1 + case["out"].abs().max())


# ---- bitwise conditions -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bitwise_net(input_dim=3, **kw):
    torch.manual_seed(9)
    return spread(LRUEmbedding(input_dim, 5, **kw), 9).cuda()


SMALL = dict(state_dim=3, hidden_dim=8, num_blocks=1)


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch_size():
    for net, B, T in ((bitwise_net(), 70, 37), (bitwise_net(1, **SMALL), 600, 16)):
        x = torch.randn(B, T, net.dims[0], generator=torch.Generator().manual_seed(11)).cuda()
        with torch.no_grad():
            out = net.features(x)
            assert net.kernel_route(x)[0] and torch.isfinite(out).all() and out.abs().max() > 0
            for i in (0, 5, 37, B - 1):
                assert torch.equal(net.features(x[i:i + 1])[0], out[i]), i
            assert torch.equal(net.features(x[30:47]), out[30:47])


def test_two_backward_calls_give_identical_gradients():
    for net, B, T in ((bitwise_net(), 70, 37), (bitwise_net(1, **SMALL), 600, 16)):
        g = torch.Generator().manual_seed(12)
        x = torch.randn(B, T, net.dims[0], generator=g).cuda()
        wts = torch.randn(B, net.dims[1], generator=g).cuda()
        grads = []
        for _ in range(2):
            net.zero_grad()
            (net.features(x) * wts).sum().backward()
            grads.append(kernel_grad(net).clone())
        assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0


def test_loop_and_scan_modules_give_identical_bits():
    loop = bitwise_net()
    scan = LRUEmbedding(3, 5, mode="scan").cuda()
    scan.load_state_dict(loop.state_dict(), strict=True)
    g = torch.Generator().manual_seed(13)
    x, wts = torch.randn(17, 37, 3, generator=g).cuda(), torch.randn(17, 40, generator=g).cuda()
    got = []
    for m in (loop, scan):
        assert m.kernel_route(x) == (True, "kernel")
        m.zero_grad()
        out = m.features(x)
        (out * wts).sum().backward()
        got.append((out.detach(), kernel_grad(m).clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_step_stays_in_its_own_row(bad):
    net = bitwise_net()
    x = torch.randn(17, 37, 3, generator=torch.Generator().manual_seed(15))
    holed = x.clone()
    holed[8, 20, 1] = bad
    keep = [i for i in range(17) if i != 8]
    with torch.no_grad():
        out, out_bad = net.features(x.cuda()), net.features(holed.cuda())
    assert torch.equal(out_bad[keep], out[keep]) and torch.isfinite(out).all()
    assert not torch.isfinite(out_bad[8]).all()


# ---- routing and launch counts ----------------------------------------------------------------------------------------
def test_the_forced_route_launches_no_lru_kernel(monkeypatch):
    x = torch.randn(17, 20, 3, generator=torch.Generator().manual_seed(16)).cuda()
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    want = net(x)

    def refuse(*args):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(L._LRUEmbedFn, "apply", refuse)
    got = twin(x)
    got.sum().backward()
    assert torch.isfinite(kernel_grad(twin)).all()
    assert (got - want).abs().max() <= 1e-4 * (1 + want.abs().max())
    with pytest.raises(AssertionError, match="about to be launched"):
        net(x)


def test_the_kernel_route_calls_forward_once_per_module_forward_whatever_T(monkeypatch):
    lib = _lib.load()
    calls = {"forward": 0, "backward": 0}
    fwd, bwd = lib.sbi_amd_lru_forward, lib.sbi_amd_lru_backward

    def count_forward(*args):
        calls["forward"] += 1
        return fwd(*args)

    def count_backward(*args):
        calls["backward"] += 1
        return bwd(*args)

    monkeypatch.setattr(lib, "sbi_amd_lru_forward", count_forward)
    monkeypatch.setattr(lib, "sbi_amd_lru_backward", count_backward)
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    for n, T in enumerate((5, 200)):
        x = torch.randn(4, T, 3, device="cuda")
        net(x).sum().backward()
        assert calls == {"forward": 2 * n + 1, "backward": n + 1}
        with torch.no_grad():
            net(x)
        assert calls == {"forward": 2 * n + 2, "backward": n + 1}
    twin(x).sum().backward()
    assert calls == {"forward": 4, "backward": 2}


def test_what_the_kernels_do_not_take_runs_eager_and_gives_the_eager_numbers():
    g = torch.Generator().manual_seed(24)
    x = torch.randn(5, 20, 3, generator=g).cuda()
    # an input that requires grad: d/dx exists on the eager route only
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    xd = x.clone().requires_grad_(True)
    assert net.kernel_route(xd) == (False, "input requires grad (the kernel backward has no d/dx)")
    out = net(xd)
    out.sum().backward()
    assert torch.equal(out, twin(x)) and torch.isfinite(xd.grad).all() and xd.grad.abs().max() > 0
    with torch.no_grad():
        assert net.kernel_route(xd)[0]          # nothing to differentiate: the kernels take it
    # layer norm, dropout in training mode
    torch.manual_seed(25)
    norm = spread(LRUEmbedding(3, 5, apply_input_normalization=True), 25).cuda()
    assert norm.kernel_route(x) == (False, "apply_input_normalization (no layer norm in the kernels)")
    forced = copy.deepcopy(norm)
    forced.force_eager = True
    assert torch.equal(norm(x), forced(x))
    drop = spread(LRUEmbedding(3, 5, dropout=0.5), 26).cuda()
    assert drop.kernel_route(x) == (False, "dropout in training mode (no dropout in the kernels)")
    torch.manual_seed(27)
    a = drop(x)
    forced = copy.deepcopy(drop)
    forced.force_eager = True
    torch.manual_seed(27)
    assert torch.equal(a, forced(x))
    assert drop.eval().kernel_route(x) == (True, "kernel")
    # a block too wide for the LDS
    wide = spread(LRUEmbedding(3, 5, state_dim=64, hidden_dim=128, num_blocks=1), 28).cuda()
    assert wide.kernel_route(x) == (False, "one block's weights plus the time tiles exceed 160 KiB of LDS")
    forced = copy.deepcopy(wide)
    forced.force_eager = True
    out = wide(x)
    out.sum().backward()
    assert torch.equal(out, forced(x)) and torch.isfinite(kernel_grad(wide)).all()


# ---- module level -----------------------------------------------------------------------------------------------------
def test_the_next_forward_uses_the_new_weights():
    torch.manual_seed(19)
    host = spread(LRUEmbedding(3, 5), 19)
    x = torch.randn(17, 20, 3, generator=torch.Generator().manual_seed(20))
    with torch.no_grad():
        want = host(x)
    close = lambda a, b: (a.cpu() - b.cpu()).abs().max() <= 1e-4 * (1 + b.abs().max())     # noqa: E731
    net = copy.deepcopy(host).to("cuda")
    xd = x.cuda()
    assert net.kernel_route(xd) == (True, "kernel")
    with torch.no_grad():
        assert close(net(xd), want)
    fresh = LRUEmbedding(3, 5).cuda()
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
    net, twin = both_routes(copy.deepcopy(bitwise_net(1, **SMALL)))
    x = torch.randn(6, 9, 1, generator=torch.Generator().manual_seed(22)).cuda()
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        assert m.kernel_route(x)[0] == (name == "kernel")
        params = m.kernel_parameters()
        first = torch.autograd.grad(m.features(x).square().sum(), params, create_graph=True)
        penalty = sum(torch.view_as_real(g).square().sum() if g.is_complex() else g.square().sum() for g in first)
        got[name] = L.flat_image([g for g in torch.autograd.grad(penalty, params, allow_unused=True) if g is not None])
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    # the same formula differentiated twice, once from the kernels' outputs: fp32 rounding apart
    assert (got["kernel"] - got["eager"]).abs().max() <= 1e-3 * got["eager"].abs().max()


def nsf_estimator(seed=20):
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    torch.manual_seed(seed)
    n, T = 256, 24
    theta = torch.randn(n, 2)
    grid = torch.linspace(0, 1, T)
    x = (theta[:, :1] * torch.sin(6 * grid) + theta[:, 1:] * torch.cos(6 * grid) + 0.3 * torch.randn(n, T))[..., None]
    torch.manual_seed(seed + 1)
    return theta, x, build_nsf(theta, x, embedding_net=spread(LRUEmbedding(1, 8), seed))


def test_gradients_through_build_nsf_match_the_eager_route():
    theta, x, est = nsf_estimator()
    est = est.to("cuda")
    lru = est.embedding_net[-1]
    assert isinstance(lru, LRUEmbedding)
    seen = {}

    def keep_input(module, args):
        seen["x"] = args[0].detach()

    def keep_feature_gradient(module, args):
        if args[0].requires_grad:
            args[0].register_hook(lambda g: seen.__setitem__("g", g.detach()))

    lru.register_forward_pre_hook(keep_input)
    lru.output_layer.register_forward_pre_hook(keep_feature_gradient)
    got, ref = {}, {}
    for name in ("kernel", "eager"):
        lru.force_eager = name == "eager"
        est.zero_grad()
        seen.clear()
        est.loss(theta.cuda(), x.cuda()).mean().backward()
        assert lru.kernel_route(seen["x"])[0] == (name == "kernel"), lru.kernel_route(seen["x"])
        got[name] = kernel_grad(lru)
        # fp64 oracle of the recurrent stack alone, driven by the gradient the output layer handed back in THIS run
        ref[name] = oracle(lru, seen["x"], seen["g"])[1]
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    e_k, e_e = worst(got["kernel"], ref["kernel"]), worst(got["eager"], ref["eager"])
    scale = ref["kernel"].abs().max().item()
    print(f"build_nsf lru grads: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e}")
    parity_log.record("lru_through_build_nsf", "256-24x1", kernel_err=e_k, eager_err=e_e, max_ref=scale,
                      ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= max(4 * e_e, 16 * 2.0**-24 * scale)
