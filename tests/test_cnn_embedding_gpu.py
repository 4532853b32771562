"""CNNEmbedding on the cnn_embed HIP kernels: parity with the fp64 oracle (tests/cnn_embedding_oracle.py) over a
pairwise-covering set of shapes, the recorded cases of the real sbi class, the bitwise conditions the fixed orders
give, and the module in front of a flow.

Parity bound (features and flat parameter gradient, the bound of tests/test_embedding_nets_gpu.py): the kernel's worst
error against the fp64 oracle is at most 4 x the eager fp32 route's worst error on the same inputs, with the floor
16 * 2^-24 * max|ref|.  Measured ratios go to the parity artifact (tests/parity_log.py).

Every parity case is well separated (the oracle's docstring): its seed is the first one of a CPU search
(`python -m tests.test_cnn_embedding_gpu` prints them) and is hard-coded in SEEDS; the tests assert the condition."""
import copy
import itertools
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import CNNEmbedding
from sbi_amd.neural_nets.embedding_nets import cnn as C
from tests import cnn_embedding_oracle as O
from tests import parity_log

pytestmark = pytest.mark.gpu

SHAPES = ((12,), (13,), (33,), (12, 12), (13, 12), (9, 17))
IN_CHANNELS, OUT_CHANNELS = (1, 3), ((6, 12), (5, 17), (16,), (4, 4, 4))
KERNELS, POOLS, BATCHES = (3, 5), (2, 3), (1, 17, 70)


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


# combinations whose map shrinks to 0 are dropped.  Edges inside the cover: an odd extent whose last column the pool
# drops (13, 33, 9 x 17), a final map of extent 1 ((12, 12) with 5 / 2), a channel count crossing 16, one-, two- and
# three-layer stacks.
CASES = pairwise([SHAPES, IN_CHANNELS, OUT_CHANNELS, KERNELS, POOLS, BATCHES],
                 allowed=lambda c: O.sizes(c[0], c[2], c[3], c[4]) is not None)
# a launch has at most 512 workgroups: a batch larger than one pass of the grid, at the smallest shape
CASES.append(((12,), 1, (6, 12), 3, 2, 600))


def case_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


# first well separated seed of every case (CPU search, see the module docstring)
SEEDS = {
    "12-1-6x12-3-2-1": 0,
    "12-3-16-5-3-17": 0,
    "13-1-5x17-3-3-70": 0,
    "33-3-4x4x4-5-2-70": 0,
    "12x12-1-5x17-5-2-17": 0,
    "12x12-3-6x12-3-3-1": 0,
    "33-1-4x4x4-3-3-17": 0,
    "13x12-1-16-3-2-1": 0,
    "13-3-6x12-5-2-1": 0,
    "9x17-3-5x17-3-2-1": 0,
    "9x17-1-16-5-3-70": 1,
    "13x12-3-6x12-3-3-17": 0,
    "13x12-1-6x12-5-2-70": 2,
    "12-1-5x17-3-2-70": 0,
    "12-1-4x4x4-3-2-1": 0,
    "13-1-16-3-2-17": 0,
    "33-1-6x12-3-2-1": 0,
    "12x12-1-16-3-2-70": 0,
    "9x17-1-6x12-3-2-17": 0,
    "13-1-4x4x4-3-2-1": 0,
    "33-1-5x17-3-2-1": 0,
    "33-1-16-3-2-1": 0,
    "12x12-1-4x4x4-3-2-1": 0,
    "13x12-1-5x17-3-2-1": 0,
    "13x12-1-4x4x4-3-2-1": 0,
    "9x17-1-4x4x4-3-2-1": 0,
    "12-1-6x12-3-2-600": 0,
}


def make_net(case):
    shape, cin, couts, k, pk, _ = case
    return CNNEmbedding(shape, in_channels=cin, out_channels_per_layer=list(couts), num_conv_layers=len(couts),
                        kernel_size=k, pool_kernel_size=pk)


def spread(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # away from the small default init: every layer matters
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
    return net


def parity_inputs(case, seed):
    """(net on the host, x (B, C, spatial...), wts (B, F)) of a case under a seed"""
    torch.manual_seed(seed)
    net = spread(make_net(case), seed)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(case[5], *net.input_shape, generator=g) * 1.3 + 0.2
    wts = torch.randn(case[5], net.linear_subnet.dims[0], generator=g)
    return net, x, wts


def find_seed(case, floor=1.0):
    for seed in range(10000):
        net, x, _ = parity_inputs(case, seed)
        report = []
        O.cnn_forward([p.detach().double() for p in net.conv_parameters()], x.double(), case[4], report)
        if report[0] >= floor:
            return seed
    raise RuntimeError(case)


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


def conv_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.conv_parameters()])


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
        got[name] = (out, conv_grad(m))
    return got


# ---- parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_parity(case):
    config = case_id(case)
    net, x, wts = parity_inputs(case, SEEDS[config])
    ref_out, ref_grad, separation, _ = O.cnn_reference(net.conv_parameters(), x, wts, case[4])
    assert separation >= 1.0, separation
    got = run_both(*both_routes(net), x, wts)
    for i, (what, ref) in enumerate((("forward", ref_out), ("param_grad", ref_grad))):
        check("cnn_parity", config, what, got["kernel"][i], got["eager"][i], ref)


GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "cnn_embedding_reference.pt"), weights_only=False)


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_the_recorded_cases_on_the_kernel_route(name):
    case = GOLDEN["cases"][name]
    net = CNNEmbedding(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    net, twin = both_routes(net)
    x = case["x"]
    # d loss / d features of the recorded loss, through the (eager fp32) head at the recorded features
    f = case["features"].clone().requires_grad_(True)
    (copy.deepcopy(twin.linear_subnet).cpu().net(f) * case["wts"]).sum().backward()
    ref_out, ref_grad, separation, _ = O.cnn_reference(net.conv_parameters(), x, f.grad, net.dims[5])
    assert separation >= 1.0, separation
    got = run_both(net, twin, x, f.grad)
    for i, (what, ref) in enumerate((("forward", ref_out), ("param_grad", ref_grad))):
        check("cnn_golden", name, what, got["kernel"][i], got["eager"][i], ref)
    close = lambda a, b: bool(((a.cpu() - b).abs() <= 1e-5 * (1 + b.abs())).all())     # noqa: E731
    n = ref_grad.numel()
    assert close(got["kernel"][0], case["features"]) and close(got["kernel"][1], case["grad_flat"][:n])
    with torch.no_grad():
        assert close(net(x.cuda()), case["out"])


# ---- bitwise conditions -----------------------------------------------------------------------------------------------
def bitwise_net(shape=(13, 12), cin=3):
    return spread(CNNEmbedding(shape, in_channels=cin, kernel_size=3), 9).cuda()


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch_size():
    for net, B in ((bitwise_net(), 70), (spread(CNNEmbedding((33,)), 10).cuda(), 600)):
        x = torch.randn(B, *net.input_shape, generator=torch.Generator().manual_seed(11)).cuda()
        with torch.no_grad():
            out = net.features(x)
            assert net.kernel_route(x)[0] and torch.isfinite(out).all() and out.abs().max() > 0
            for i in (0, 5, 37, B - 1):
                assert torch.equal(net.features(x[i:i + 1])[0], out[i]), i
            assert torch.equal(net.features(x[30:47]), out[30:47])


def test_two_backward_calls_give_identical_gradients():
    for net, B in ((bitwise_net(), 70), (spread(CNNEmbedding((33,)), 10).cuda(), 600)):
        g = torch.Generator().manual_seed(12)
        x = torch.randn(B, *net.input_shape, generator=g).cuda()
        wts = torch.randn(B, net.linear_subnet.dims[0], generator=g).cuda()
        grads = []
        for _ in range(2):
            net.zero_grad()
            (net.features(x) * wts).sum().backward()
            grads.append(conv_grad(net).clone())
        assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0


def test_the_three_input_layouts_give_identical_bits():
    net = spread(CNNEmbedding((13, 12)), 13).cuda()
    x = torch.randn(17, 13, 12, generator=torch.Generator().manual_seed(14)).cuda()
    with torch.no_grad():
        a, b, c = net(x), net(x.reshape(17, 1, 13, 12)), net(x.reshape(17, 156))
    assert net.kernel_route(x)[0] and torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError, match="Expected flat or channel-first input"):
        net(x.reshape(17, 12, 13))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_pixel_stays_in_its_own_row(bad):
    net = bitwise_net()
    g = torch.Generator().manual_seed(15)
    x = torch.randn(17, 3, 13, 12, generator=g)
    holed = x.clone()
    holed[8, 1, 6, 5] = bad
    keep = [i for i in range(17) if i != 8]
    with torch.no_grad():
        out, out_bad = net.features(x.cuda()), net.features(holed.cuda())
    assert torch.equal(out_bad[keep], out[keep]) and torch.isfinite(out).all()
    assert not torch.isfinite(out_bad[8]).all()


# ---- launch counts ----------------------------------------------------------------------------------------------------
def test_the_forced_route_launches_no_cnn_kernel(monkeypatch):
    from sbi_amd.neural_nets.embedding_nets import fully_connected

    x = torch.randn(17, 1, 13, 12, generator=torch.Generator().manual_seed(16)).cuda()
    net, twin = both_routes(spread(CNNEmbedding((13, 12)), 17))
    assert not twin.linear_subnet.force_eager          # the flag sits on the CNN module alone
    assert net.linear_subnet.kernel_route(torch.zeros(17, net.linear_subnet.dims[0], device="cuda"))[0]
    want = net(x)

    def refuse(*args):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(C._CNNEmbedFn, "apply", refuse)
    monkeypatch.setattr(fully_connected._FCEmbedFn, "apply", refuse)
    got = twin(x)
    got.sum().backward()
    assert torch.isfinite(conv_grad(twin)).all()
    assert (got - want).abs().max() <= 1e-4 * (1 + want.abs().max())
    with pytest.raises(AssertionError, match="about to be launched"):
        net(x)


def test_the_kernel_route_calls_forward_once_per_module_forward(monkeypatch):
    lib = _lib.load()
    calls = {"forward": 0, "backward": 0}
    fwd, bwd = lib.sbi_amd_cnn_forward, lib.sbi_amd_cnn_backward

    def count_forward(*args):
        calls["forward"] += 1
        return fwd(*args)

    def count_backward(*args):
        calls["backward"] += 1
        return bwd(*args)

    monkeypatch.setattr(lib, "sbi_amd_cnn_forward", count_forward)
    monkeypatch.setattr(lib, "sbi_amd_cnn_backward", count_backward)
    net, twin = both_routes(spread(CNNEmbedding((13, 12)), 18))
    x = torch.randn(17, 13, 12, device="cuda")
    net(x).sum().backward()
    assert calls == {"forward": 1, "backward": 1}
    with torch.no_grad():
        net(x)
    assert calls == {"forward": 2, "backward": 1}
    twin(x).sum().backward()
    assert calls == {"forward": 2, "backward": 1}


# ---- module level -----------------------------------------------------------------------------------------------------
def test_the_next_forward_uses_the_new_weights():
    host = spread(CNNEmbedding((13, 12)), 19)
    x = torch.randn(17, 13, 12, generator=torch.Generator().manual_seed(20))
    with torch.no_grad():
        want = host(x)
    close = lambda a, b: (a.cpu() - b.cpu()).abs().max() <= 1e-4 * (1 + b.abs().max())     # noqa: E731
    net = copy.deepcopy(host).to("cuda")
    xd = x.cuda()
    assert net.kernel_route(xd) == (True, "kernel")
    with torch.no_grad():
        assert close(net(xd), want)
    fresh = CNNEmbedding((13, 12)).cuda()
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
    net, twin = both_routes(spread(CNNEmbedding((13, 12), in_channels=3, kernel_size=3), 21))
    x = torch.randn(17, 3, 13, 12, generator=torch.Generator().manual_seed(22)).cuda()
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        assert m.kernel_route(x)[0] == (name == "kernel")
        params = m.conv_parameters()
        first = torch.autograd.grad(m.features(x).square().sum(), params, create_graph=True)
        penalty = sum(g.square().sum() for g in first)
        got[name] = torch.cat([g.reshape(-1) for g in torch.autograd.grad(penalty, params, allow_unused=True)
                               if g is not None])
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    # the same formula differentiated twice, once from the kernels' outputs: fp32 rounding apart
    assert (got["kernel"] - got["eager"]).abs().max() <= 1e-3 * got["eager"].abs().max()


def test_an_input_that_requires_grad_takes_the_eager_route():
    net = spread(CNNEmbedding((13,), in_channels=3, kernel_size=3), 23).cuda()
    g = torch.Generator().manual_seed(24)
    x, wts = torch.randn(5, 3, 13, generator=g), torch.randn(5, net.linear_subnet.dims[0], generator=g)
    xd = x.cuda().requires_grad_(True)
    assert net.kernel_route(xd) == (False, "input requires grad (the kernel backward has no d/dx)")
    (net.features(xd) * wts.cuda()).sum().backward()
    _, _, _, ref_dx = O.cnn_reference(net.conv_parameters(), x, wts, 2, want_dx=True)
    assert worst(xd.grad, ref_dx) <= 1e-5 * (1 + ref_dx.abs().max().item())
    with torch.no_grad():
        assert net.kernel_route(xd)[0]          # nothing to differentiate: the kernels take it


def test_an_input_too_long_for_the_lds_falls_back_to_eager():
    n = 100
    while O.lds_bytes((n + 1,), 1, (6, 12), 5, 2) <= 160 * 1024:
        n += 1
    net, twin = both_routes(spread(CNNEmbedding((n + 1,)), 25))
    x = torch.randn(3, n + 1, generator=torch.Generator().manual_seed(26)).cuda()
    assert net.kernel_route(x.reshape(3, 1, -1)) == (False, "weights plus one sample's maps exceed 160 KiB of LDS")
    out = net(x)
    out.sum().backward()
    assert torch.equal(out, twin(x)) and torch.isfinite(conv_grad(net)).all()
    fits = CNNEmbedding((n,)).cuda()             # the longest input that is resident runs on the kernels
    xf = x[:, :n].contiguous()
    assert fits.kernel_route(xf) == (True, "kernel")
    with torch.no_grad():
        fits_twin = copy.deepcopy(fits)
        fits_twin.force_eager = True
        a, b = fits.features(xf), fits_twin.features(xf)
    assert (a - b).abs().max() <= 1e-5 * (1 + b.abs().max())


def test_a_batch_above_1024_is_left_to_eager():
    net, twin = both_routes(spread(CNNEmbedding((12,)), 27))
    x = torch.randn(1025, 12, generator=torch.Generator().manual_seed(28)).cuda()
    assert net.kernel_route(x[:1024]) == (True, "kernel")
    assert net.kernel_route(x) == (False, "batch above 1024: eager torch measured faster there")
    with torch.no_grad():
        out = net.features(x)
        assert torch.equal(out, twin.features(x))
        assert (net.features(x[:1024]) - out[:1024]).abs().max() <= 1e-5 * (1 + out.abs().max())


NSF_SEED = 20


def nsf_inputs(seed):
    torch.manual_seed(seed)
    n = 256
    theta = torch.randn(n, 2)
    grid = torch.linspace(0, 1, 12)
    x = (theta[:, :1, None] * torch.sin(6 * grid)[None, :, None] + theta[:, 1:, None] * torch.cos(6 * grid)[None, None, :]
         + 0.3 * torch.randn(n, 12, 12))
    return theta, x


def nsf_estimator(seed):
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    theta, x = nsf_inputs(seed)
    torch.manual_seed(seed + 1)
    return theta, x, build_nsf(theta, x, embedding_net=spread(CNNEmbedding((12, 12)), seed))


def find_nsf_seed(floor=2.0):
    """host side: the standardized x in front of the stack; a margin of 2 leaves room for the device's own rounding"""
    for seed in range(1000):
        theta, x, est = nsf_estimator(seed)
        with torch.no_grad():
            z = est.embedding_net[:-1](x).reshape(256, 1, 12, 12)
        report = []
        O.cnn_forward([p.detach().double() for p in est.embedding_net[-1].conv_parameters()], z.double(), 2, report)
        if report[0] >= floor:
            return seed
    raise RuntimeError("no well separated seed")


def test_gradients_through_build_nsf_match_the_eager_route():
    theta, x, est = nsf_estimator(NSF_SEED)
    est = est.to("cuda")
    cnn = est.embedding_net[-1]
    assert isinstance(cnn, CNNEmbedding)
    seen = {}

    def keep_input(module, args):
        seen["x"] = args[0].detach()

    def keep_feature_gradient(module, args):
        if args[0].requires_grad:
            args[0].register_hook(lambda g: seen.__setitem__("g", g.detach()))

    cnn.register_forward_pre_hook(keep_input)
    cnn.linear_subnet.register_forward_pre_hook(keep_feature_gradient)
    cnn.linear_subnet.net.register_forward_pre_hook(keep_feature_gradient)     # the forced route calls the Sequential
    got, ref = {}, {}
    for name in ("kernel", "eager"):
        cnn.force_eager = name == "eager"
        est.zero_grad()
        seen.clear()
        est.loss(theta.cuda(), x.cuda()).mean().backward()
        assert cnn.kernel_route(seen["x"])[0] == (name == "kernel"), cnn.kernel_route(seen["x"])
        got[name] = conv_grad(cnn)
        # fp64 oracle of the convolution stack alone, driven by the gradient the head handed back in THIS run
        _, ref[name], separation, _ = O.cnn_reference(cnn.conv_parameters(), seen["x"].cpu().reshape(256, 1, 12, 12),
                                                      seen["g"].cpu(), 2)
        assert separation >= 1.0, separation
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    e_k, e_e = worst(got["kernel"], ref["kernel"]), worst(got["eager"], ref["eager"])
    scale = ref["kernel"].abs().max().item()
    print(f"build_nsf cnn grads: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e}")
    parity_log.record("cnn_through_build_nsf", "256-12x12", kernel_err=e_k, eager_err=e_e, max_ref=scale,
                      ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= max(4 * e_e, 16 * 2.0**-24 * scale)


if __name__ == "__main__":      # the CPU seed search
    for c in CASES:
        print(f'    "{case_id(c)}": {find_seed(c)},', flush=True)
    print("NSF_SEED =", find_nsf_seed())
