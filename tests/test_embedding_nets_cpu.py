"""FCEmbedding / PermutationInvariantEmbedding without a GPU: the eager route against the recorded outputs of the real
sbi classes (tests/golden/embedding_reference.pt, tools/make_golden_embedding.py), state_dict interchange, the count
semantics, the routing reasons and the host-side answers of include/sbi_amd_embed.h."""
import copy
import ctypes
import os
import re

import pytest
import torch
from torch import nn

from sbi_amd import _lib
from sbi_amd.neural_nets import FCEmbedding, PermutationInvariantEmbedding
from sbi_amd.neural_nets.embedding_nets.permutation_invariant import masks_nan_trials
from tests import embedding_oracle as O
from tests.embedding_oracle import lds_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = torch.load(os.path.join(ROOT, "tests", "golden", "embedding_reference.pt"))


def row_parity(got, ref):
    """the project's row parity: |d| <= 1e-5 (1 + |ref|)"""
    got, ref = got.double(), ref.double()
    return bool(((got - ref).abs() <= 1e-5 * (1 + ref.abs())).all())


def flat_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


def perminv_from(case, agg):
    net = PermutationInvariantEmbedding(FCEmbedding(**case["trial_kwargs"]), aggregation_fn=agg, **case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    return net


# ---- the eager route against the real classes ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN["fc"]))
def test_fc_eager_matches_the_reference(name):
    case = GOLDEN["fc"][name]
    net = FCEmbedding(**case["kwargs"])
    assert list(net.state_dict()) == list(case["state_dict"])
    net.load_state_dict(case["state_dict"], strict=True)
    out = net(case["x"])
    assert row_parity(out, case["out"])
    (out * case["wts"]).sum().backward()
    assert row_parity(flat_grad(net), case["grad_flat"])


@pytest.mark.parametrize("agg", ["sum", "mean"])
@pytest.mark.parametrize("name", sorted(GOLDEN["perminv"]))
def test_perminv_eager_matches_the_reference_where_the_counts_agree(name, agg):
    case = GOLDEN["perminv"][name]
    net = perminv_from(case, agg)
    assert list(net.state_dict()) == list(case["state_dict"])
    assert all(k.startswith(("trial_net.net.", "fc_subnet.net.")) for k in net.state_dict())
    out = net(case["x"])
    assert row_parity(out, case[agg]["out"])
    (out * case[agg]["wts"]).sum().backward()
    assert row_parity(flat_grad(net), case[agg]["grad_flat"])
    # and the fp64 oracle says the same on these inputs
    n_t = 2 * case["trial_kwargs"]["num_layers"]
    params = list(net.parameters())
    ref, _ = O.perminv_reference(params[:n_t], params[n_t:], case["x"], case[agg]["wts"], agg == "mean")
    assert row_parity(case[agg]["out"], ref)


def test_state_dict_keys_follow_the_reference_layout():
    assert list(FCEmbedding(3).state_dict()) == ["net.0.weight", "net.0.bias", "net.3.weight", "net.3.bias"]
    assert list(FCEmbedding(3, num_layers=4).state_dict()) == [
        f"net.{i}.{w}" for i in (0, 3, 6, 9) for w in ("weight", "bias")]
    ln = FCEmbedding(3, num_layers=3, enable_layer_norm=True)
    assert [k for k in ln.state_dict() if k.startswith(("net.1.", "net.4."))] == [
        "net.1.weight", "net.1.bias", "net.4.weight", "net.4.bias"]
    assert isinstance(ln.net[-1], nn.ReLU) and isinstance(ln.net[-2], nn.Linear)
    assert FCEmbedding(3, activation=nn.Tanh)(torch.randn(4, 3)).abs().max() <= 1     # the last activation is applied


def test_signatures_defaults_and_assertion_message():
    import inspect

    fc = inspect.signature(FCEmbedding.__init__).parameters
    assert [(k, v.default) for k, v in fc.items()][1:] == [
        ("input_dim", inspect.Parameter.empty), ("output_dim", 20), ("num_layers", 2), ("num_hiddens", 50),
        ("enable_layer_norm", False), ("activation", nn.ReLU)]
    pi = inspect.signature(PermutationInvariantEmbedding.__init__).parameters
    assert [(k, v.default) for k, v in pi.items()][1:] == [
        ("trial_net", inspect.Parameter.empty), ("trial_net_output_dim", inspect.Parameter.empty),
        ("aggregation_fn", "sum"), ("num_hiddens", 100), ("num_layers", 2), ("output_dim", 20), ("aggregation_dim", 1)]
    with pytest.raises(AssertionError, match=re.escape("aggregation_fn must be 'mean' or 'sum'.")):
        PermutationInvariantEmbedding(FCEmbedding(2), 20, aggregation_fn="max")


# ---- count semantics --------------------------------------------------------------------------------------------------
def test_count_is_per_element_where_sbi_reads_another_elements():
    torch.manual_seed(3)
    B, T, D = 4, 5, 3
    counts = [5, 1, 3, 2]
    x = torch.randn(B, T, D)
    for b, n in enumerate(counts):
        x[b, n:] = float("nan")
    sbi_counts = T - torch.isnan(x).sum(dim=1).reshape(-1)[:B]       # the reference's expression
    assert sbi_counts.tolist() != counts                              # this input is a departing one
    for agg in ("sum", "mean"):
        net = PermutationInvariantEmbedding(FCEmbedding(D, output_dim=6, num_hiddens=12), 6, aggregation_fn=agg,
                                            num_hiddens=10, output_dim=4)
        wts = torch.randn(B, 4)
        out = net(x)
        (out * wts).sum().backward()
        params = list(net.parameters())
        ref, gref = O.perminv_reference(params[:4], params[4:], x, wts, agg == "mean")
        assert row_parity(out, ref)
        assert row_parity(flat_grad(net), torch.cat([g.reshape(-1) for g in gref]))


def test_partly_nan_trial_counts_and_reads_zero():
    net = PermutationInvariantEmbedding(FCEmbedding(2, output_dim=3, num_hiddens=8), 3, num_hiddens=8, output_dim=2)
    x = torch.tensor([[[1.0, float("nan")], [float("nan"), float("nan")]]])
    same = torch.tensor([[[1.0, 0.0]]])
    assert torch.equal(net(x), net(same))


def test_element_without_a_valid_trial():
    torch.manual_seed(5)
    x = torch.randn(3, 4, 2)
    x[1] = float("nan")
    trial = FCEmbedding(2, output_dim=3, num_hiddens=8)
    s = PermutationInvariantEmbedding(trial, 3, aggregation_fn="sum", num_hiddens=8, output_dim=2)
    out = s(x)
    assert torch.equal(out[1], s.fc_subnet(torch.zeros(1, 4))[0])
    m = PermutationInvariantEmbedding(trial, 3, aggregation_fn="mean", num_hiddens=8, output_dim=2)
    out = m(x)
    assert torch.isnan(out[1]).all() and torch.isfinite(out[[0, 2]]).all()
    assert torch.equal(out[[0, 2]], m(x[[0, 2]]))


# ---- routing ----------------------------------------------------------------------------------------------------------
def test_kernel_route_reasons():
    x = torch.randn(4, 3)
    assert FCEmbedding(3).kernel_route(x) == (False, "input is not on a ROCm device")
    assert FCEmbedding(3).kernel_route(x.double()) == (False, "input is not float32")
    assert FCEmbedding(3, activation=nn.Tanh).kernel_route(x) == (False, "activation is not nn.ReLU")
    assert FCEmbedding(3, enable_layer_norm=True).kernel_route(x) == (False, "layer norm is enabled")
    forced = FCEmbedding(3)
    forced.force_eager = True
    assert forced.kernel_route(x) == (False, "force_eager is set")
    assert not FCEmbedding.force_eager

    x3 = torch.randn(2, 5, 3)
    mk = lambda trial, **kw: PermutationInvariantEmbedding(trial, 20, **kw)     # noqa: E731
    assert mk(FCEmbedding(3)).kernel_route(x3) == (False, "input is not on a ROCm device")
    assert mk(nn.Sequential(nn.Linear(3, 20))).kernel_route(x3) == (False, "trial_net is not sbi_amd's FCEmbedding")
    assert mk(FCEmbedding(3, activation=nn.ELU)).kernel_route(x3) == (False, "trial_net: activation is not nn.ReLU")
    assert mk(FCEmbedding(3, enable_layer_norm=True)).kernel_route(x3) == (False, "trial_net: layer norm is enabled")
    assert mk(FCEmbedding(3), aggregation_dim=2).kernel_route(x3) == (False, "aggregation_dim is not 1")
    assert mk(FCEmbedding(3, output_dim=7)).kernel_route(x3) == (
        False, "trial_net_output_dim does not match the trial_net")
    assert mk(FCEmbedding(3)).kernel_route(x3.double()) == (False, "input is not float32")
    # every fallback still computes
    assert mk(nn.Sequential(nn.Linear(3, 20)))(x3).shape == (2, 20)
    assert mk(FCEmbedding(3, activation=nn.ELU))(x3).shape == (2, 20)


def test_weights_follow_deepcopy_load_state_dict_and_optimizer_steps():
    torch.manual_seed(2)
    x = torch.randn(3, 4, 2)
    net = PermutationInvariantEmbedding(FCEmbedding(2, output_dim=3, num_hiddens=8), 3, num_hiddens=8, output_dim=2)
    twin = copy.deepcopy(net)
    assert torch.equal(twin(x), net(x))
    opt = torch.optim.Adam(net.parameters(), lr=0.1)
    net(x).sum().backward()
    opt.step()
    assert not torch.equal(twin(x), net(x))
    twin.load_state_dict(net.state_dict(), strict=True)
    assert torch.equal(twin(x), net(x))


def test_nan_x_o_is_let_through_for_this_embedding_only():
    from sbi_amd.inference.posteriors.direct_posterior import DirectPosterior
    from sbi_amd.neural_nets.net_builders.flow import Standardize

    class Est:
        def __init__(self, emb):
            self.embedding_net = emb

    pi = PermutationInvariantEmbedding(FCEmbedding(2), 20)
    assert masks_nan_trials(Est(pi))
    assert masks_nan_trials(Est(nn.Sequential(Standardize(torch.zeros(2), torch.ones(2)), pi)))
    assert not masks_nan_trials(Est(nn.Sequential(Standardize(torch.zeros(2), torch.ones(2)), FCEmbedding(2))))
    assert not masks_nan_trials(Est(None)) and not masks_nan_trials(Est(nn.Identity()))
    post = DirectPosterior.__new__(DirectPosterior)
    nan_x, inf_x = torch.tensor([[1.0, float("nan")]]), torch.tensor([[1.0, float("inf")]])
    assert not post._x_is_acceptable(nan_x) and not post._x_is_acceptable(inf_x)
    post._allow_nan_x = True
    assert post._x_is_acceptable(nan_x) and not post._x_is_acceptable(inf_x)


# ---- host side of the C ABI -------------------------------------------------------------------------------------------
def cfg(in_dim=3, hidden=50, out_dim=20, num_layers=2):
    return _lib.FCEmbedConfigC(in_dim, hidden, out_dim, num_layers)


def plan(c, B=10, T=1):
    waves, lds = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = _lib.load().sbi_amd_embed_plan(ctypes.byref(c) if c is not None else None, B, T, ctypes.byref(waves),
                                        ctypes.byref(lds))
    return rc, waves.value, lds.value


def test_param_count_and_offsets():
    lib = _lib.load()
    for kw in (dict(), dict(in_dim=17, hidden=32, out_dim=7, num_layers=3), dict(in_dim=64, hidden=128, out_dim=64,
                                                                               num_layers=4)):
        c = cfg(**kw)
        net = FCEmbedding(c.in_dim, c.out_dim, c.num_layers, c.hidden)
        offs = (ctypes.c_int64 * (2 * c.num_layers))()
        assert lib.sbi_amd_embed_param_count(ctypes.byref(c), offs) == sum(p.numel() for p in net.parameters())
        want, at = [], 0
        for p in net.parameters():
            want.append(at)
            at += p.numel()
        assert list(offs) == want
        assert lib.sbi_amd_embed_param_count(ctypes.byref(c), None) == at


def test_plan_envelope_edges():
    assert plan(cfg()) == (0, 8, lds_bytes(3, 50, 20, 2))
    for kw, bad in ((dict(in_dim=64), dict(in_dim=65)), (dict(hidden=128), dict(hidden=129)),
                    (dict(out_dim=64), dict(out_dim=65)), (dict(num_layers=2), dict(num_layers=1)),
                    (dict(num_layers=4), dict(num_layers=5))):
        assert plan(cfg(**kw))[0] == 0, kw
        assert plan(cfg(**bad))[0] == _lib.E_UNSUPPORTED, bad
        assert _lib.load().sbi_amd_embed_param_count(ctypes.byref(cfg(**bad)), None) == _lib.E_UNSUPPORTED
    assert plan(cfg(), B=3, T=65535)[0] == 0
    assert plan(cfg(), B=3, T=65536)[0] == _lib.E_UNSUPPORTED
    assert plan(cfg(), B=2**31 // 65535 + 1, T=65535)[0] == _lib.E_UNSUPPORTED      # rows past 2^31
    for kw in (dict(in_dim=0), dict(hidden=0), dict(out_dim=0), dict(num_layers=0)):
        assert plan(cfg(**kw))[0] == _lib.E_BADARG, kw
    assert plan(cfg(), B=0)[0] == _lib.E_BADARG and plan(cfg(), T=0)[0] == _lib.E_BADARG
    assert plan(None)[0] == _lib.E_BADARG
    assert _lib.load().sbi_amd_embed_param_count(None, None) == _lib.E_BADARG
    assert _lib.load().sbi_amd_embed_workspace_bytes(None, 10) == _lib.E_BADARG
    assert _lib.load().sbi_amd_embed_workspace_bytes(ctypes.byref(cfg()), 0) == _lib.E_BADARG


@pytest.mark.parametrize("L", [2, 3, 4])
def test_first_shape_that_exceeds_the_lds(L):
    """in_dim = out_dim = 64: walk hidden upwards; the plan says E_LDS exactly when the documented image passes 160 KiB"""
    first = next((h for h in range(1, 129) if lds_bytes(64, h, 64, L) > 160 * 1024), None)
    assert (first is None) == (L == 2)
    for h in ([128] if first is None else [first - 1, first, 128]):
        rc, waves, lds = plan(cfg(64, h, 64, L))
        if first is not None and h >= first:
            assert rc == _lib.E_LDS
            # the parameter count is still answered: it does not depend on the LDS budget
            assert _lib.load().sbi_amd_embed_param_count(ctypes.byref(cfg(64, h, 64, L)), None) == sum(
                p.numel() for p in FCEmbedding(64, 64, L, h).parameters())
        else:
            assert (rc, waves, lds) == (0, 8, lds_bytes(64, h, 64, L))
    # the half-chunk band below E_LDS: 100 hidden units in 4 layers fit only with 16-row tiles
    assert 4 * (lds_bytes(1, 100, 1, 4) // 4) == lds_bytes(1, 100, 1, 4) <= 160 * 1024 < lds_bytes(1, 100, 1, 4) + 4 * 16 * (
        2 * 20 + 3 * 116)
    assert plan(cfg(1, 100, 1, 4)) == (0, 8, lds_bytes(1, 100, 1, 4))


def test_workspace_is_a_function_of_the_shape():
    lib = _lib.load()
    c = cfg()
    P = 3 * 50 + 50 + 50 * 20 + 20
    assert lib.sbi_amd_embed_workspace_bytes(ctypes.byref(c), 1) == 4 * P
    assert lib.sbi_amd_embed_workspace_bytes(ctypes.byref(c), 33) == 2 * 4 * P
    assert lib.sbi_amd_embed_workspace_bytes(ctypes.byref(c), 10**6) == 512 * 4 * P


def test_exported_symbols_equal_the_header():
    text = open(os.path.join(ROOT, "include", "sbi_amd_embed.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sbi_amd_\w+)\s*\(", text))
    assert declared == set(_lib.exported_symbols_embed()) and len(declared) == 7
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert not set(_lib.exported_symbols_embed()) & set(_lib.exported_symbols())


# ---- the eager route is eager all the way down; Inf is not masked ------------------------------------------------------
def test_the_eager_route_never_enters_the_sub_nets_own_routing(monkeypatch):
    net = PermutationInvariantEmbedding(FCEmbedding(2, output_dim=3, num_hiddens=8), 3, num_hiddens=8, output_dim=2)
    x = torch.randn(3, 4, 2)
    want = net(x)

    def refuse(self, x):
        raise AssertionError("the eager route went through FCEmbedding.forward (which may pick the kernels)")

    monkeypatch.setattr(FCEmbedding, "forward", refuse)
    net.force_eager = True
    got = net(x)
    got.sum().backward()
    assert torch.equal(got, want) and all(p.grad is not None for p in net.parameters())


def test_inf_entries_are_passed_on_not_clamped():
    torch.manual_seed(7)
    net = PermutationInvariantEmbedding(FCEmbedding(2, output_dim=3, num_hiddens=8), 3, num_hiddens=8, output_dim=2)
    with torch.no_grad():      # every first-layer unit sees the first input coordinate
        net.trial_net.net[0].weight[:, 0] = net.trial_net.net[0].weight[:, 0].abs() + 0.1
    x = torch.randn(3, 4, 2)
    bad = x.clone()
    bad[1, 2, 0] = float("inf")
    clamped = torch.nan_to_num(bad, nan=0.0)          # what sbi feeds its trial net
    out = net(bad)
    assert torch.equal(out[[0, 2]], net(x)[[0, 2]])
    assert torch.isfinite(net.trial_net(clamped)).all()
    assert not torch.isfinite(net.trial_net(bad[1])).all()                  # the Inf reaches the trial net as it is
    assert not torch.isfinite(out[1]).all() and torch.isfinite(net(clamped)).all()
