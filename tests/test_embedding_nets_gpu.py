"""FCEmbedding / PermutationInvariantEmbedding on the embed HIP kernels: parity with the fp64 oracle
(tests/embedding_oracle.py) over a pairwise-covering set of shapes, the bitwise conditions the pooled sum's fixed order
gives, and the module in front of a flow.

Parity bound (every quantity: forward, parameter gradient, d/dx): the kernel's worst error against the fp64 oracle is
at most 4 x the eager fp32 route's worst error on the same inputs, with the floor 16 * 2^-24 * max|ref| (an eager error
of exactly 0 must not fail a correct kernel).  Measured ratios go to the parity artifact (tests/parity_log.py)."""
import copy
import itertools

import pytest
import torch

from sbi_amd.neural_nets import FCEmbedding, PermutationInvariantEmbedding
from tests import embedding_oracle as O
from tests import parity_log

pytestmark = pytest.mark.gpu

IN_DIMS, HIDDENS, OUT_DIMS, LAYERS, BATCHES = (1, 3, 17), (16, 50, 100), (1, 20, 33), (2, 4), (1, 17, 333)
TRIALS, COUNTS, AGGS = (1, 15, 16, 17, 33), ("full", "random", "single", "none"), ("sum", "mean")


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


def fits(D, H, E, L):
    """the documented LDS image of this net stays within 160 KiB (tests/embedding_oracle.py restates it)"""
    return O.lds_bytes(D, H, E, L) <= 160 * 1024


# every pair of levels is covered by a shape the kernels take; the one corner that cannot be resident (hidden 100 in 4
# layers with the widest input AND output) is the fallback test below
FC_CASES = pairwise([IN_DIMS, HIDDENS, OUT_DIMS, LAYERS, BATCHES], allowed=lambda c: fits(*c[:4]))
PI_CASES = pairwise([IN_DIMS, HIDDENS, OUT_DIMS, LAYERS, BATCHES, TRIALS, COUNTS, AGGS],
                    allowed=lambda c: not (c[6] == "none" and c[7] == "mean") and fits(*c[:4])
                    and fits(c[2] + 1, c[1], c[2], c[3]))
# the half-chunk path (16-row tiles: hidden 100 in 4 layers) at more than the 1-wide input and output the cover gives it
FC_CASES.append((3, 100, 20, 4, 17))
PI_CASES.append((3, 100, 15, 4, 17, 17, "random", "mean"))


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


def flat_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


def spread(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # away from the small default init: every layer matters
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
    return net


def both_routes(net):
    """(kernel-route module on the device, eager twin with the same weights)"""
    net = net.cuda()
    twin = copy.deepcopy(net)
    twin.force_eager = True
    return net, twin


def make_x(B, T, D, counts, seed):
    """(B, T, D) with valid trials at random positions; one partly-NaN entry in a valid trial when D > 1"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, D, generator=g) * 1.3 + 0.2
    if counts == "full":
        n = [T] * B
    else:
        n = torch.randint(1, T + 1, (B,), generator=g).tolist()
        if counts == "single":
            n[B // 2] = 1
        if counts == "none":
            n[B // 2] = 0
    for b in range(B):
        drop = torch.randperm(T, generator=g)[n[b]:]
        x[b, drop] = float("nan")
    if D > 1 and counts != "full":
        b = 0 if n[0] > 0 else B - 1
        t = int(torch.nonzero(~torch.isnan(x[b, :, 0]))[0]) if n[b] > 0 else None
        if t is not None:
            x[b, t, 1] = float("nan")
    return x


# ---- parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fc_parity(case):
    D, H, E, L, B = case
    config = "-".join(map(str, case))
    net, twin = both_routes(spread(FCEmbedding(D, E, L, H), 1))
    g = torch.Generator().manual_seed(2)
    x, wts = torch.randn(B, D, generator=g) * 1.5, torch.randn(B, E, generator=g)
    ref_out, ref_grads, ref_dx = O.fc_reference(list(net.parameters()), x, wts, want_dx=True)
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        xd = x.cuda().requires_grad_(True)
        assert m.kernel_route(xd)[0] == (name == "kernel"), m.kernel_route(xd)
        out = m(xd)
        (out * wts.cuda()).sum().backward()
        got[name] = (out, flat_grad(m), xd.grad)
    ref = (ref_out, torch.cat([g_.reshape(-1) for g_ in ref_grads]), ref_dx)
    for i, what in enumerate(("forward", "param_grad", "dx")):
        check("fc_parity", config, what, got["kernel"][i], got["eager"][i], ref[i])


@pytest.mark.parametrize("case", PI_CASES, ids=lambda c: "-".join(map(str, c)))
def test_perminv_parity(case):
    D, H, E, L, B, T, counts, agg = case
    config = "-".join(map(str, case))
    net = PermutationInvariantEmbedding(FCEmbedding(D, E, L, H), E, aggregation_fn=agg, num_hiddens=H, num_layers=L,
                                        output_dim=E)
    net, twin = both_routes(spread(net, 3))
    x = make_x(B, T, D, counts, 4)
    wts = torch.randn(B, E, generator=torch.Generator().manual_seed(5))
    params = list(net.parameters())
    ref_out, ref_grads = O.perminv_reference(params[:2 * L], params[2 * L:], x, wts, agg == "mean")
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        assert m.kernel_route(x.cuda())[0] == (name == "kernel"), m.kernel_route(x.cuda())
        out = m(x.cuda())
        (out * wts.cuda()).sum().backward()
        got[name] = (out, flat_grad(m))
    ref = (ref_out, torch.cat([g_.reshape(-1) for g_ in ref_grads]))
    for i, what in enumerate(("forward", "param_grad")):
        check("perminv_parity", config, what, got["kernel"][i], got["eager"][i], ref[i])


def test_a_net_too_wide_for_the_lds_falls_back_to_eager():
    assert not fits(17, 100, 33, 4)
    net = PermutationInvariantEmbedding(FCEmbedding(17, 33, 4, 100), 33, num_hiddens=100, num_layers=4, output_dim=33)
    net, twin = both_routes(spread(net, 3))
    x = make_x(17, 15, 17, "random", 4).cuda()
    assert net.kernel_route(x) == (False, "trial_net: weight image plus row tiles exceed 160 KiB of LDS")
    out = net(x)
    out.sum().backward()
    assert torch.equal(out, twin(x)) and torch.isfinite(flat_grad(net)).all()
    fc = FCEmbedding(17, 33, 4, 100).cuda()
    assert fc.kernel_route(x) == (False, "weight image plus row tiles exceed 160 KiB of LDS")
    assert fc(x).shape == (17, 15, 33)


def test_permuting_the_valid_trials_stays_within_the_parity_bound():
    B, T, D, E = 17, 33, 3, 20
    net, twin = both_routes(spread(PermutationInvariantEmbedding(FCEmbedding(D, E), E, num_hiddens=50, output_dim=E), 6))
    x = make_x(B, T, D, "random", 7)
    g = torch.Generator().manual_seed(8)
    xp = torch.stack([row[torch.randperm(T, generator=g)] for row in x])
    params = list(net.parameters())
    with torch.no_grad():
        ref = O.perminv_forward([p.detach().double().cpu() for p in params[:4]],
                                [p.detach().double().cpu() for p in params[4:]], x.double(), False)
        a, b, e = net(x.cuda()), net(xp.cuda()), twin(x.cuda())
    check("perminv_permuted", "17-33-3", "forward", a, e, ref)
    check("perminv_permuted", "17-33-3", "forward_permuted", b, e, ref)
    assert not torch.equal(a, b)        # a different association: close, not bitwise


# ---- bitwise conditions -----------------------------------------------------------------------------------------------
def bitwise_net(agg="sum"):
    net = PermutationInvariantEmbedding(FCEmbedding(3, 20, 2, 50), 20, aggregation_fn=agg, num_hiddens=50, output_dim=20)
    return spread(net, 9).cuda()


def test_a_row_does_not_depend_on_its_place_in_the_batch():
    net = bitwise_net()
    x = make_x(333, 17, 3, "random", 10).cuda()
    with torch.no_grad():
        out = net(x)
        for i in (0, 5, 166, 332):
            assert torch.equal(net(x[i:i + 1])[0], out[i]), i
        assert torch.equal(net(x[100:117]), out[100:117])


@pytest.mark.parametrize("agg", AGGS)
def test_a_row_does_not_depend_on_trailing_padding(agg):
    net = bitwise_net(agg)
    T = 15
    x = make_x(5, T, 3, "random", 11)
    with torch.no_grad():
        out = net(x.cuda())
        for extra in (1, 16, 40):
            grown = torch.cat([x, torch.full((5, extra, 3), float("nan"))], dim=1).cuda()
            assert torch.equal(net(grown), out), extra


def test_two_backward_calls_give_identical_gradients():
    net = bitwise_net("mean")
    x = make_x(333, 33, 3, "random", 12).cuda()
    wts = torch.randn(333, 20, device="cuda")
    grads = []
    for _ in range(2):
        net.zero_grad()
        (net(x) * wts).sum().backward()
        grads.append(flat_grad(net).clone())
    assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all()
    fc = spread(FCEmbedding(17, 33, 4, 100), 13).cuda()
    xf = torch.randn(333, 17, device="cuda")
    wf = torch.randn(333, 33, device="cuda")
    grads = []
    for _ in range(2):
        fc.zero_grad()
        xg = xf.clone().requires_grad_(True)
        (fc(xg) * wf).sum().backward()
        grads.append(torch.cat([flat_grad(fc), xg.grad.reshape(-1)]).clone())
    assert torch.equal(grads[0], grads[1])


def test_an_all_nan_element_under_mean_leaves_the_other_rows_alone():
    net = bitwise_net("mean")
    x = make_x(17, 16, 3, "random", 14)
    holed = x.clone()
    holed[8] = float("nan")
    with torch.no_grad():
        out, out_h = net(x.cuda()), net(holed.cuda())
    keep = [i for i in range(17) if i != 8]
    assert torch.isnan(out_h[8]).all() and torch.isfinite(out).all()
    assert torch.equal(out_h[keep], out[keep])


def test_an_element_without_a_valid_trial_under_sum_is_the_head_at_zero():
    net = bitwise_net("sum")
    x = make_x(17, 16, 3, "none", 15).cuda()
    with torch.no_grad():
        out = net(x)
        zero = net.fc_subnet(torch.zeros(1, 21, device="cuda"))
    assert net.fc_subnet.kernel_route(torch.zeros(1, 21, device="cuda"))[0]
    assert torch.equal(out[8], zero[0])


# ---- module level -----------------------------------------------------------------------------------------------------
def test_gradients_through_build_nsf_match_the_eager_route():
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    torch.manual_seed(0)
    n, T, D, E = 256, 8, 2, 12
    theta = torch.randn(n, 2)
    x = theta[:, None, :] + 0.5 * torch.randn(n, T, D)
    counts = torch.randint(1, T + 1, (n,))
    for b in range(n):
        x[b, counts[b]:] = float("nan")
    emb = PermutationInvariantEmbedding(FCEmbedding(D, E, 2, 32), E, num_hiddens=32, output_dim=10)
    torch.manual_seed(1)
    est = build_nsf(theta, x, embedding_net=emb).to("cuda")
    pi = est.embedding_net[-1]
    assert isinstance(pi, PermutationInvariantEmbedding)
    seen = {}

    def keep_input(module, args):
        seen["x"] = args[0].detach()

    def keep_output_gradient(module, args, out):
        if out.requires_grad:
            out.register_hook(lambda g: seen.__setitem__("g", g.detach()))

    pi.register_forward_pre_hook(keep_input)
    pi.register_forward_hook(keep_output_gradient)
    got, ref = {}, {}
    for name in ("kernel", "eager"):
        pi.force_eager = name == "eager"
        est.zero_grad()
        est.loss(theta.cuda(), x.cuda()).mean().backward()
        assert pi.kernel_route(seen["x"])[0] == (name == "kernel"), pi.kernel_route(seen["x"])
        got[name] = flat_grad(pi)
        params = list(pi.parameters())
        # fp64 oracle of the embedding alone, driven by the gradient the flow kernels handed back in THIS run
        _, grads = O.perminv_reference(params[:4], params[4:], seen["x"].cpu(), seen["g"].cpu(), False)
        ref[name] = torch.cat([g_.reshape(-1) for g_ in grads])
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    e_k, e_e = worst(got["kernel"], ref["kernel"]), worst(got["eager"], ref["eager"])
    scale = ref["kernel"].abs().max().item()
    print(f"build_nsf embedding grads: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e}")
    parity_log.record("embed_through_build_nsf", "256-8-2", kernel_err=e_k, eager_err=e_e, max_ref=scale)
    assert e_k <= max(4 * e_e, 16 * 2.0**-24 * scale)


def test_the_next_forward_uses_the_new_weights():
    x = make_x(17, 15, 3, "random", 16)
    host = spread(PermutationInvariantEmbedding(FCEmbedding(3, 20), 20, num_hiddens=50), 17)
    with torch.no_grad():
        want = host(x)
    close = lambda a, b: (a.cpu() - b.cpu()).abs().max() <= 1e-4 * (1 + b.abs().max())     # noqa: E731
    net = copy.deepcopy(host).to("cuda")                                # .to()
    xd = x.cuda()
    assert net.kernel_route(xd) == (True, "kernel")
    with torch.no_grad():
        assert close(net(xd), want)
    twin = copy.deepcopy(net)                                           # deepcopy: its own weights
    with torch.no_grad():
        for p in twin.parameters():
            p.mul_(1.5)
        assert not close(twin(xd), want) and close(net(xd), want)
    fresh = PermutationInvariantEmbedding(FCEmbedding(3, 20), 20, num_hiddens=50).cuda()
    fresh.load_state_dict(twin.state_dict(), strict=True)               # load_state_dict
    with torch.no_grad():
        assert torch.equal(fresh(xd), twin(xd))
    opt = torch.optim.Adam(net.parameters(), lr=0.05)                   # in-place optimizer update
    net(xd).sum().backward()
    opt.step()
    eager = copy.deepcopy(net)
    eager.force_eager = True
    with torch.no_grad():
        after = net(xd)
        assert not close(after, want) and close(after, eager(xd))
    fc = FCEmbedding(3).cuda()
    assert fc.kernel_route(xd)[0] and fc(xd).shape == (17, 15, 20)      # leading dimensions are kept


def test_double_backward_differentiates_the_eager_formula():
    x = make_x(17, 15, 3, "random", 18).cuda()
    net, twin = both_routes(spread(PermutationInvariantEmbedding(FCEmbedding(3, 20), 20, num_hiddens=50), 19))
    fc, fc_twin = both_routes(spread(FCEmbedding(3, 20, 3, 16), 20))
    xf = torch.randn(33, 3, device="cuda")
    got = {}
    for name, m, f in (("kernel", net, fc), ("eager", twin, fc_twin)):
        second = []
        for module, inp in ((m, x), (f, xf.clone().requires_grad_(True))):
            assert module.kernel_route(inp)[0] == (name == "kernel")
            params = list(module.parameters())
            first = torch.autograd.grad(module(inp).square().sum(), params, create_graph=True)
            penalty = sum(g.square().sum() for g in first)
            second.append(torch.cat([g.reshape(-1) for g in torch.autograd.grad(penalty, params, allow_unused=True)
                                     if g is not None]))
        got[name] = torch.cat(second)
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    # the same formula differentiated twice, once from the kernels' outputs: fp32 rounding apart
    assert (got["kernel"] - got["eager"]).abs().max() <= 1e-3 * got["eager"].abs().max()


def test_the_forced_route_launches_no_embed_kernel(monkeypatch):
    from sbi_amd.neural_nets.embedding_nets import fully_connected, permutation_invariant

    x = make_x(17, 15, 3, "random", 21).cuda()
    net, twin = both_routes(spread(PermutationInvariantEmbedding(FCEmbedding(3, 20), 20, num_hiddens=50), 22))
    assert not twin.trial_net.force_eager and not twin.fc_subnet.force_eager     # the flag sits on the pooled net alone
    want = net(x)

    def refuse(*args):
        raise AssertionError("an embed kernel was about to be launched")

    monkeypatch.setattr(fully_connected._FCEmbedFn, "apply", refuse)
    monkeypatch.setattr(permutation_invariant._PermInvFn, "apply", refuse)
    got = twin(x)
    got.sum().backward()
    assert torch.isfinite(flat_grad(twin)).all()
    assert (got - want).abs().max() <= 1e-4 * (1 + want.abs().max()) and not torch.equal(got, want)
    with pytest.raises(AssertionError, match="about to be launched"):
        net(x)
    fc, fc_twin = both_routes(FCEmbedding(3))
    assert fc_twin(x).shape == (17, 15, 20)
    with pytest.raises(AssertionError, match="about to be launched"):
        fc(x)


def test_inf_entries_are_passed_on_by_both_routes():
    x = make_x(17, 15, 3, "full", 23)
    bad = x.clone()
    bad[4, 2, 0] = float("inf")
    net, twin = both_routes(spread(PermutationInvariantEmbedding(FCEmbedding(3, 20), 20, num_hiddens=50), 24))
    keep = [i for i in range(17) if i != 4]
    with torch.no_grad():
        for m in (net, twin):
            out, out_bad = m(x.cuda()), m(bad.cuda())
            assert torch.equal(out_bad[keep], out[keep])
            assert not torch.isfinite(out_bad[4]).all() or not torch.equal(out_bad[4], out[4])
        clamped = torch.nan_to_num(bad).cuda()
        assert torch.isfinite(net(clamped)).all()
