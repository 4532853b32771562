"""TransformerEmbedding on the tr_embed HIP kernels: parity with the fp64 oracle (tests/transformer_embedding_oracle.py)
over a pairwise-covering set of sizes with T on the query / key tile edges, the recorded series cases of the real sbi
class, dropout (keep rate, keying, parity with the exported masks, seeding), the bitwise conditions the fixed orders
give, routing, and the module in front of a flow.

Parity bound (output and flat parameter gradient, the bound of tests/test_embedding_nets_gpu.py): the kernel's worst
error against the fp64 oracle is at most 4 x the eager fp32 route's worst error on the same device and inputs, with the
floor 16 * 2^-24 * max|ref|.  Measured figures go to the parity artifact (tests/parity_log.py).

Relu cases.  The gradient jumps where a gate pre-activation crosses 0.  Each route's gradient is compared with the
fp64 gradient on its own side of every kink: the oracle lists the units whose fp64 pre-activation lies within
64 * 2^-24 * max|gate| of 0 (`kink_candidates`) and every assignment of sides that differs from fp64's at those units
only; a route's error is its distance to the nearest of these gradients.  A route on the other side of a kink anywhere
else matches none of them and fails the bound."""
import copy
import functools
import itertools
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import TransformerEmbedding
from sbi_amd.neural_nets.embedding_nets import transformer as TR
from tests import parity_log
from tests import transformer_embedding_oracle as O
from tests import transformer_envelope as env

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 40)
STEPS = (1, 2, 15, 16, 17, 31, 33, 65)
HEADS = ((12, 6, 6), (16, 1, 1), (36, 6, 3), (64, 4, 1), (72, 4, 4), (128, 2, 2))       # (F, heads, kv heads)
INTER, LAYERS = (4, 17, 64), (1, 3)
POS, CAUSAL, ACT, INPUT = ("rotary", "positional", "none"), (True, False), ("gelu", "relu"), ("scalar", "features")
FACTORS = [BATCHES, STEPS, HEADS, INTER, LAYERS, POS, CAUSAL, ACT, INPUT]


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
DEFAULT_HEADS = (96, 12, 12)
FIXED = [
    (600, 16, (36, 6, 3), 17, 1, "rotary", True, "gelu", "scalar"),          # more sequences than workgroups
    (4, 100, DEFAULT_HEADS, 256, 4, "rotary", True, "gelu", "scalar"),       # the defaults at F = 96
    (1, 1024, (24, 12, 12), 256, 4, "rotary", True, "gelu", "scalar"),       # a long sequence at F = 24
    # the longest sequence of the envelope: both attention-backward kernels need 128 KiB of dynamic LDS, far above
    # the default limit, so each one's limit has to be raised
    (1, 4096, (4, 1, 1), 4, 1, "rotary", True, "gelu", "scalar"),
]


def case_id(c):
    return "-".join("x".join(str(u) for u in v) if isinstance(v, tuple) else str(v) for v in c)


def kwargs_of(case):
    _, _, (F, H, KV), inter, layers, pos, causal, act, _ = case
    return dict(feature_space_dim=F, num_attention_heads=H, num_key_value_heads=KV, intermediate_size=inter,
                num_hidden_layers=layers, pos_emb=pos, is_causal=causal, mlp_activation=act)


def spread(net, seed):
    """every parameter moved by 0.2 randn, as the golden tool does"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
    return net


def draw(case, seed):
    B, T, (F, _, _) = case[0], case[1], case[2]
    torch.manual_seed(seed)
    net = spread(TransformerEmbedding(**kwargs_of(case)), seed).eval()
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(*((B, T) if case[8] == "scalar" else (B, T, F)), generator=g) * 1.3 + 0.2
    wts = torch.randn(B, F // 2, generator=g)
    return net, x, wts


def parity_inputs(case):
    return draw(case, 0)


def worst(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


def check(test, config, what, kernel, eager, ref, others=()):
    """the bound of the module docstring for one quantity; prints and records before it asserts.  `others`: the
    reference on the other sides of the kinks that lie within the margin; each route is held against its nearest"""
    e_k = min(worst(kernel, r) for r in (ref, *others))
    e_e = min(worst(eager, r) for r in (ref, *others))
    scale = ref.abs().max().item()
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


def run_both(net, twin, x, wts):
    got = {}
    for name, m in (("kernel", net), ("eager", twin)):
        xd = x.cuda()
        assert m.kernel_route(xd)[0] == (name == "kernel"), m.kernel_route(xd)
        m.zero_grad()
        out = m(xd)
        (out * wts.cuda()).sum().backward()
        got[name] = (out, O.flat_grad(m))
    return got


# ---- parity -----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_every_pair():
    every = set()
    for c in itertools.product(*FACTORS):
        every.update((i, c[i], j, c[j]) for i in range(len(c)) for j in range(i + 1, len(c)))
    covered = {(i, c[i], j, c[j]) for c in CASES for i in range(len(c)) for j in range(i + 1, len(c))}
    assert every <= covered, sorted(every - covered, key=str)[:5]
    assert all({c[i] for c in CASES} == set(f) for i, f in enumerate(FACTORS))
    assert len(CASES) <= 80
    assert sorted({F // H for F, H, _ in HEADS}) == [2, 6, 16, 18, 64]
    # every case, the fixed ones too, is inside the plan
    for c in CASES + FIXED:
        net = TransformerEmbedding(**kwargs_of(c))
        assert TR.plan(net.kernel_config(c[8] == "scalar"), c[0], c[1])[0] == 0, c
    assert -(-600 * 16 // 8) > 256            # more tiles than weight-gradient workgroups
    long = TransformerEmbedding(**kwargs_of(FIXED[3]))
    assert TR.plan(long.kernel_config(True), 1, 4096)[1][4] == 4 * 4 * (2 * 4096 + 2 * 4) > 64 * 1024


@pytest.mark.parametrize("case", CASES + FIXED, ids=case_id)
def test_parity(case):
    """Output and flat gradient under the whole-quantity bound, then the gradient slot by slot.  Nearest its slot bound
    on the MI355X: (1, 2, (16, 1, 1), 17, 3, positional, every key, relu, features), layer 0: k rows 2.674e-07 against
    the 16-ulp floor 2.778e-07 (scale 0.291), q rows 1.421e-07 against 1.687e-07 (4 x eager)."""
    config = case_id(case)
    net, x, wts = parity_inputs(case)
    got = run_both(*both_routes(net), x, wts)
    ref = O.reference(net.state_dict(), x, wts, kwargs_of(case))
    others = []
    if case[7] == "relu":
        near, candidates = O.kink_candidates(net.state_dict(), x, kwargs_of(case))
        print(f"tr_parity[{config}] pre-activations within the margin of a kink: {near}")
        others = [O.reference(net.state_dict(), x, wts, kwargs_of(case), positive=c) for c in candidates[1:]]
    for i, what in enumerate(("forward", "param_grad")):
        check("tr_parity", config, what, got["kernel"][i], got["eager"][i], ref[i], [o[i] for o in others])
    # ... and the gradient slot by slot (tests/transformer_envelope.py)
    env.slot_check("tr_parity", case, got["kernel"][1], got["eager"][1], ref[1],
                   env.per_sequence(net, x, wts, case)[2], others=[o[1] for o in others])


GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "transformer_embedding_reference.pt"),
                    weights_only=False)
SERIES = sorted(n for n, c in GOLDEN["cases"].items()
                if not O.full_config(c["kwargs"])["vit"] and O.full_config(c["kwargs"])["ffn"] == "mlp"
                and c["attention_mask"] is None)


@pytest.mark.parametrize("name", SERIES)
def test_the_recorded_series_cases_on_the_kernel_route(name):
    """the recording of the real class is the reference"""
    case = GOLDEN["cases"][name]
    net, twin = both_routes(O.golden_net(TransformerEmbedding, case))
    assert net.kernel_route(case["x"].cuda()) == (True, "kernel")
    got = run_both(net, twin, case["x"], case["wts"])
    assert got["kernel"][1].numel() == case["grad_flat"].numel()
    for i, (what, ref) in enumerate((("forward", case["out"]), ("param_grad", case["grad_flat"]))):
        check("tr_golden", name, what, got["kernel"][i], got["eager"][i], ref.double())
    # ... and the gradient slot by slot against the fp64 oracle on the recorded weights and inputs
    state, kw, rows = case["state_dict"], case["kwargs"], range(case["x"].shape[0])
    sides = [None]
    if O.full_config(kw)["mlp_activation"] == "relu":
        sides = O.kink_candidates(state, case["x"], kw)[1]

    def oracle(positive):
        return [O.reference(state, case["x"][b:b + 1], case["wts"][b:b + 1], kw,
                            positive=None if positive is None else [m[b:b + 1] for m in positive])[1] for b in rows]

    per_seq = oracle(sides[0])
    env.slot_check("tr_golden", (name, env.sizes_of_kwargs(kw), "scalar" if case["x"].ndim == 2 else "features"),
                   got["kernel"][1], got["eager"][1], sum(per_seq), sum(g.abs() for g in per_seq),
                   others=[sum(oracle(c)) for c in sides[1:]])


# ---- dropout ----------------------------------------------------------------------------------------------------------
DROP = dict(feature_space_dim=36, num_attention_heads=6, num_key_value_heads=3, intermediate_size=17,
            num_hidden_layers=2)


def dropout_net(p, seed=5):
    torch.manual_seed(seed)
    net = spread(TransformerEmbedding(**dict(DROP, attention_dropout=p)), seed).cuda().train()
    net.dropout_seed = 1234567890123
    return net


def masks_of(net, B, T):
    p = net.config["attention_dropout"]
    return [TR.dropout_mask(net.kernel_config(True), B, T, p, net.dropout_seed, l, "cuda")
            for l in range(net.config["num_hidden_layers"])]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_the_keep_rate_of_the_exported_masks(p):
    net = dropout_net(p)
    for mask in masks_of(net, 4, 33):
        n = mask.numel()
        assert mask.shape == (4, 6, 33, 33) and n == 4 * 6 * 33 * 33
        rate = mask.float().mean().item()
        sd = (p * (1 - p) / n) ** 0.5
        print(f"keep rate at p={p}: {rate:.5f} (1 - p = {1 - p}, 5 sd = {5 * sd:.5f})")
        assert abs(rate - (1 - p)) <= 5 * sd


def test_the_mask_is_keyed_by_element_not_by_shape():
    net = dropout_net(0.5)
    small, big = masks_of(net, 2, 17), masks_of(net, 4, 33)
    for l in range(2):
        assert torch.equal(small[l], big[l][:2, :, :17, :17])
    assert not torch.equal(big[0], big[1])
    assert not torch.equal(big[0][:, 0], big[0][:, 1]) and not torch.equal(big[0][0], big[0][1])
    net.dropout_seed += 1
    assert not torch.equal(masks_of(net, 4, 33)[0], big[0])


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_parity_with_the_exported_masks(p):
    """forward and backward use the masks the mask kernel exports: the eager formula and the oracle are fed them"""
    net = dropout_net(p)
    g = torch.Generator().manual_seed(7)
    x, wts = (torch.randn(4, 33, generator=g) * 1.3 + 0.2).cuda(), torch.randn(4, 18, generator=g).cuda()
    assert net.kernel_route(x) == (True, "kernel")
    out = net(x)
    (out * wts).sum().backward()
    grad = O.flat_grad(net).clone()
    keep = masks_of(net, 4, 33)
    params = [q.detach().clone().requires_grad_(True) for q in net.parameters()]
    eager = TR.tr_functional(x, params, dict(net.config, head_dim=6), keep)
    eager_grad = torch.cat([t.reshape(-1) for t in torch.autograd.grad((eager * wts).sum(), params)])
    ref = O.reference(net.state_dict(), x, wts, dict(DROP, attention_dropout=p), keep_masks=keep)
    check("tr_dropout", f"p{p}", "forward", out, eager, ref[0])
    check("tr_dropout", f"p{p}", "param_grad", grad, eager_grad, ref[1])
    net.eval()
    with torch.no_grad():
        assert (net(x) - out).abs().max() > 1e-3          # the masks did something


def test_seeding():
    net = dropout_net(0.5)
    net.dropout_seed = None
    x = torch.randn(4, 33, generator=torch.Generator().manual_seed(8)).cuda()
    with torch.no_grad():
        a, b = net(x), net(x)
        assert not torch.equal(a, b)
        torch.manual_seed(77)
        c = net(x)
        torch.manual_seed(77)
        d = net(x)
    assert torch.equal(c, d) and torch.isfinite(c).all()


# ---- bitwise conditions -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bitwise_net():
    torch.manual_seed(9)
    return spread(TransformerEmbedding(**DROP), 9).cuda().eval()


def test_a_row_does_not_depend_on_its_place_in_the_batch_or_on_the_batch_size():
    net = bitwise_net()
    for B, T in ((70, 19), (600, 16)):
        x = (torch.randn(B, T, generator=torch.Generator().manual_seed(11)) * 1.3).cuda()
        with torch.no_grad():
            out = net(x)
            assert net.kernel_route(x)[0] and torch.isfinite(out).all() and out.abs().max() > 0
            for i in (0, 2, B // 2, B - 1):
                assert torch.equal(net(x[i:i + 1])[0], out[i]), i
            assert torch.equal(net(x[1:4]), out[1:4])


def test_two_backward_calls_give_identical_gradients():
    net = bitwise_net()
    for B, T in ((70, 19), (600, 16)):
        g = torch.Generator().manual_seed(12)
        x, wts = torch.randn(B, T, generator=g).cuda(), torch.randn(B, 18, generator=g).cuda()
        grads = []
        for _ in range(2):
            net.zero_grad()
            (net(x) * wts).sum().backward()
            grads.append(O.flat_grad(net).clone())
        assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all() and grads[0].abs().max() > 0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_value_stays_in_its_own_row(bad):
    net = bitwise_net()
    x = torch.randn(70, 19, generator=torch.Generator().manual_seed(15))
    holed = x.clone()
    holed[8, 4] = bad           # sequence 8 shares token tiles with sequences 7 and 9 (19 is no multiple of the tile)
    keep = [i for i in range(70) if i != 8]
    with torch.no_grad():
        out, out_bad = net(x.cuda()), net(holed.cuda())
    assert torch.isfinite(out).all() and torch.equal(out_bad[keep], out[keep])
    assert not torch.isfinite(out_bad[8]).any()
    wts = torch.randn(70, 18, generator=torch.Generator().manual_seed(16)).cuda()
    grads = []
    for inp in (x, holed, x):
        net.zero_grad()
        (net(inp.cuda()) * wts).sum().backward()
        grads.append(O.flat_grad(net).clone())
    assert torch.isfinite(grads[0]).all() and not torch.isfinite(grads[1]).all() and torch.equal(grads[0], grads[2])


# ---- routing and launch counts ----------------------------------------------------------------------------------------
def test_the_forced_route_launches_no_tr_kernel(monkeypatch):
    x = torch.randn(5, 19, generator=torch.Generator().manual_seed(16)).cuda()
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    want = net(x)
    lib = _lib.load()

    def refuse(*args):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(lib, "sbi_amd_tr_forward", refuse)
    monkeypatch.setattr(lib, "sbi_amd_tr_backward", refuse)
    got = twin(x)
    got.sum().backward()
    assert torch.isfinite(O.flat_grad(twin)).all()
    assert (got - want).abs().max() <= 1e-4 * (1 + want.abs().max())
    with pytest.raises(AssertionError, match="about to be launched"):
        net(x)


def test_the_kernel_route_calls_forward_and_backward_once_per_module_call(monkeypatch):
    lib = _lib.load()
    calls = {"forward": 0, "backward": 0}
    fwd, bwd = lib.sbi_amd_tr_forward, lib.sbi_amd_tr_backward

    def count_forward(*args):
        calls["forward"] += 1
        return fwd(*args)

    def count_backward(*args):
        calls["backward"] += 1
        return bwd(*args)

    monkeypatch.setattr(lib, "sbi_amd_tr_forward", count_forward)
    monkeypatch.setattr(lib, "sbi_amd_tr_backward", count_backward)
    for i, (T, layers) in enumerate(((16, 1), (50, 3), (30, 8))):
        net, twin = both_routes(TransformerEmbedding(**dict(DROP, num_hidden_layers=layers)))
        x = torch.randn(4, T, device="cuda")
        net(x).sum().backward()             # training mode, attention_dropout 0.5
        assert calls == {"forward": 2 * i + 1, "backward": i + 1}
        with torch.no_grad():
            net(x)
        assert calls == {"forward": 2 * i + 2, "backward": i + 1}
    twin(x).sum().backward()
    assert calls == {"forward": 6, "backward": 3}


def test_what_the_kernels_do_not_take_runs_eager_and_gives_the_eager_numbers():
    g = torch.Generator().manual_seed(24)
    x = torch.randn(5, 19, generator=g).cuda()
    net, twin = both_routes(copy.deepcopy(bitwise_net()))
    # an input that requires grad: d/dx exists on the eager route only
    xd = x.clone().requires_grad_(True)
    assert net.kernel_route(xd) == (False, "input requires grad (the kernel backward has no d/dx)")
    out = net(xd)
    out.sum().backward()
    assert torch.equal(out, twin(x)) and torch.isfinite(xd.grad).all() and xd.grad.abs().max() > 0
    with torch.no_grad():
        assert net.kernel_route(xd)[0]
    # a mask, position ids, fp64
    am = torch.ones(5, 19, device="cuda")
    am[1, :4] = 0
    assert not net.kernel_route(x, attention_mask=am)[0]
    assert torch.equal(net(x, attention_mask=am), twin(x, attention_mask=am))
    assert not torch.equal(net(x, attention_mask=am)[1], twin(x)[1])
    ids = torch.arange(19, device="cuda") + 3
    assert not net.kernel_route(x, position_ids=ids)[0]
    assert torch.equal(net(x, position_ids=ids), twin(x, position_ids=ids))
    double = copy.deepcopy(net).double()
    assert double.kernel_route(x.double()) == (False, "input is not float32")
    assert (double(x.double()) - twin(x)).abs().max() <= 1e-4 * (1 + twin(x).abs().max())
    assert double.kernel_route(x) == (False, "parameters are not float32 on the input's device")
    # MoE, ViT, F = 132, T = 4097
    small = dict(feature_space_dim=24, intermediate_size=8, num_hidden_layers=1)
    for kw, shape, reason in (
            (dict(small, ffn="moe", num_local_experts=3, num_experts_per_tok=2), (3, 9), 'ffn="moe" runs eager'),
            (dict(small, vit=True, image_size=8, patch_size=4, num_channels=1, vit_dropout=0.0), (3, 1, 8, 8),
             "vit=True runs eager"),
            (dict(small, feature_space_dim=132, num_attention_heads=6, num_key_value_heads=6), (3, 9),
             TR.plan_reason(_lib.E_UNSUPPORTED)),
            (dict(small, num_attention_heads=2, num_key_value_heads=2), (1, 4097),
             TR.plan_reason(_lib.E_UNSUPPORTED))):
        torch.manual_seed(28)
        other = TransformerEmbedding(**kw).cuda().eval()
        xo = torch.randn(*shape, generator=g).cuda()
        assert other.kernel_route(xo) == (False, reason)
        forced = copy.deepcopy(other)
        forced.force_eager = True
        out = other(xo)
        out.sum().backward()
        assert torch.equal(out, forced(xo)) and torch.isfinite(O.flat_grad(other)).all()


# ---- module level -----------------------------------------------------------------------------------------------------
def test_the_next_forward_uses_the_new_weights():
    torch.manual_seed(19)
    host = spread(TransformerEmbedding(**DROP), 19).eval()
    x = torch.randn(17, 20, generator=torch.Generator().manual_seed(20))
    with torch.no_grad():
        want = host(x)
    close = lambda a, b: (a.cpu() - b.cpu()).abs().max() <= 1e-4 * (1 + b.abs().max())     # noqa: E731
    net = copy.deepcopy(host).to("cuda")
    xd = x.cuda()
    assert net.kernel_route(xd) == (True, "kernel")
    with torch.no_grad():
        assert close(net(xd), want)
    fresh = TransformerEmbedding(**DROP).cuda().eval()
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
    x = torch.randn(6, 19, generator=torch.Generator().manual_seed(22)).cuda()
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


def nsf_estimator(features, seed=20):
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    torch.manual_seed(seed)
    n, T = 256, 32
    theta = torch.randn(n, 2)
    grid = torch.linspace(0, 1, T)
    x = theta[:, :1] * torch.sin(6 * grid) + theta[:, 1:] * torch.cos(6 * grid) + 0.3 * torch.randn(n, T)
    kw = dict(DROP, attention_dropout=0.0)
    if features:
        x = x[:, :, None] * torch.linspace(0.5, 1.5, 36)
    torch.manual_seed(seed + 1)
    return theta, x, build_nsf(theta, x, embedding_net=spread(TransformerEmbedding(**kw), seed))


@pytest.mark.parametrize("features", [False, True], ids=["series", "features"])
def test_gradients_through_build_nsf_match_the_eager_route(features):
    theta, x, est = nsf_estimator(features)
    est = est.to("cuda")
    emb = est.embedding_net[-1]
    assert isinstance(emb, TransformerEmbedding)
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
        assert seen["x"].shape[1:] == x.shape[1:]
        assert emb.kernel_route(seen["x"])[0] == (name == "kernel"), emb.kernel_route(seen["x"])
        got[name] = O.flat_grad(emb)
        ref[name] = O.reference(emb.state_dict(), seen["x"], seen["g"], dict(DROP, attention_dropout=0.0))[1]
    assert torch.isfinite(got["kernel"]).all() and got["kernel"].abs().max() > 0
    e_k, e_e = worst(got["kernel"], ref["kernel"]), worst(got["eager"], ref["eager"])
    scale = ref["kernel"].abs().max().item()
    print(f"build_nsf transformer embedding grads: kernel {e_k:.3e} eager {e_e:.3e} max|ref| {scale:.3e}")
    parity_log.record("tr_through_build_nsf", "features" if features else "series", kernel_err=e_k, eager_err=e_e,
                      max_ref=scale, ratio=e_k / e_e if e_e > 0 else float("inf") if e_k > 0 else 0.0)
    assert e_k <= max(4 * e_e, 16 * 2.0**-24 * scale)
