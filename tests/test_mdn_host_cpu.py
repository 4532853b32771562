"""Host side of the mixture-density-network estimator without a GPU: config, factory and refusal behaviour, the flat
parameter layout against the restatement's parameter shapes (C ABI size / offset queries included), the state-dict
round trip in the reference's keys, the initialisation constants, the out-of-envelope and multi-round refusals."""
import math
import os
import re
import warnings

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import MDNConfig, likelihood_nn, posterior_nn
from sbi_amd.neural_nets.estimators.mdn import MDNHyper, MixtureDensityEstimator, MoG
from sbi_amd.neural_nets.net_builders.mdn import build_mdn
from tests.mdn_oracle import MDNOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mdn_reference.pt")


def _data(D=3, C=4, n=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=g) * 1.5 + 0.3, torch.randn(n, C, generator=g) * 0.7 - 0.2


def test_config_and_factory_build_the_estimator():
    theta, x = _data()
    assert (MDNConfig().hidden_features, MDNConfig().num_components) == (50, 10)
    est = MDNConfig(hidden_features=16, num_components=4).build(theta, x)
    assert isinstance(est, MixtureDensityEstimator)
    assert est.input_shape == (3,) and est.condition_shape == (4,)
    h = est.net.hyper
    assert (h.D, h.C, h.hidden_features, h.num_components, h.epsilon) == (3, 4, 16, 4, 1e-4)
    est2 = posterior_nn("mdn", hidden_features=16, num_components=4)(theta, x)
    assert est2.net.hyper == h
    assert posterior_nn("mdn")(theta, x).net.hyper.num_components == 10
    with pytest.warns(UserWarning, match="Unknown kwargs"):
        build = posterior_nn("mdn", num_transforms_typo=3)
    assert isinstance(build(theta, x), MixtureDensityEstimator)
    with pytest.raises(ValueError):
        MDNConfig(z_score_input="nonsense")
    with pytest.raises(ValueError):
        MDNConfig(num_components=0)


def test_z_scoring_buffers_are_the_reference_s():
    theta, x = _data()
    est = build_mdn(theta, x, hidden_features=8, num_components=2)
    z = est.net.zstats
    assert torch.allclose(z[:3], theta.mean(0)) and torch.allclose(z[3:6], theta.std(0))
    assert torch.allclose(z[6:10], x.mean(0)) and torch.allclose(z[10:], x.std(0))
    est = build_mdn(theta, x, z_score_x="none", z_score_y=None, hidden_features=8, num_components=2)
    assert torch.equal(est.net.zstats, torch.cat([torch.zeros(3), torch.ones(3), torch.zeros(4), torch.ones(4)]))
    assert "_transform_shift" not in est.state_dict() and "_embedding_net.0._mean" not in est.state_dict()


def test_refusals_by_name():
    theta, x = _data()
    with pytest.raises(NotImplementedError, match="transform_to_unconstrained"):
        build_mdn(theta, x, z_score_x="transform_to_unconstrained")
    with pytest.raises(NotImplementedError, match="transform_to_unconstrained"):
        posterior_nn("mdn", z_score_theta="transform_to_unconstrained")(theta, x)
    with pytest.raises(NotImplementedError, match="hidden_net"):
        build_mdn(theta, x, hidden_net=torch.nn.Linear(4, 50))
    with pytest.raises(NotImplementedError):
        likelihood_nn("mdn")
    with pytest.raises(NotImplementedError):
        posterior_nn("maf")(theta, x)
    with pytest.raises(NotImplementedError, match="MADE-MoG"):
        posterior_nn("made")(theta, x)
    with pytest.raises(NotImplementedError, match="mdn_snpe_a.*NPE-A"):
        posterior_nn("mdn_snpe_a")(theta, x)
    mog = MoG(torch.zeros(1, 2), torch.zeros(1, 2, 3), torch.eye(3).expand(1, 2, 3, 3), torch.eye(3).expand(1, 2, 3, 3))
    with pytest.raises(NotImplementedError, match="condition"):
        mog.condition(torch.zeros(1, 1))
    est = build_mdn(theta, x, hidden_features=8, num_components=2)
    with pytest.raises(NotImplementedError):
        est.inverse_transform(theta, x)
    emb = torch.nn.Linear(4, 5)
    with pytest.raises(NotImplementedError, match="embedding"):
        build_mdn(theta, x, embedding_net=emb)


@pytest.mark.parametrize("kw", [dict(D=17), dict(num_components=17), dict(hidden_features=65)],
                         ids=["D17", "K17", "H65"])
def test_out_of_envelope_configurations_are_refused(kw):
    theta, x = _data(D=kw.get("D", 3))
    with pytest.raises(RuntimeError, match="not supported by the HIP kernels"):
        build_mdn(theta, x, hidden_features=kw.get("hidden_features", 16), num_components=kw.get("num_components", 4))


@pytest.mark.parametrize("D,C,H,K", [(3, 4, 16, 4), (1, 4, 16, 3), (10, 10, 50, 10), (16, 12, 64, 16)])
def test_flat_layout_matches_the_restatement_and_the_c_abi(D, C, H, K):
    o = MDNOracle(D, C, H, K)
    h = MDNHyper(D, C, H, K)
    shapes = o.param_shapes()
    assert [("net." + k, s) for k, s in h.layer_entries()] == shapes
    assert h.param_count() == sum(math.prod(s) for _, s in shapes) == o.flat_params().numel()
    assert ("net._upper_layer.weight" in dict(shapes)) == (D > 1)
    lib = _lib.load()
    cfg = h.c_config()
    assert lib.sbi_amd_mdn_param_count(cfg) == h.param_count()
    off = 0
    for i in range(len(shapes) // 2):
        (_, ws), (_, bs) = shapes[2 * i], shapes[2 * i + 1]
        assert lib.sbi_amd_mdn_param_offset(cfg, i, 0) == off
        off += math.prod(ws)
        assert lib.sbi_amd_mdn_param_offset(cfg, i, 1) == off
        off += math.prod(bs)
    if D == 1:
        assert lib.sbi_amd_mdn_param_offset(cfg, 5, 0) == _lib.E_BADARG
    assert lib.sbi_amd_mdn_packed_floats(cfg) > h.param_count()
    U = D * (D - 1) // 2
    npad = 512
    planes = 8 + 1 + 2 * -(-K * D // 16) + -(-K * U // 16)
    assert lib.sbi_amd_mdn_train_workspace_floats(cfg, 300) == npad * 3 * 64 + npad * 16 * planes + h.param_count() + (
        -h.param_count() % 4)
    for bad in (_lib.MDNConfigC(17, C, H, K, 1e-4), _lib.MDNConfigC(D, C, H, 17, 1e-4), _lib.MDNConfigC(D, C, 65, K, 1e-4),
                _lib.MDNConfigC(D, 65, H, K, 1e-4)):
        assert lib.sbi_amd_mdn_param_count(bad) == _lib.E_UNSUPPORTED
    for bad in (_lib.MDNConfigC(0, C, H, K, 1e-4), _lib.MDNConfigC(D, 0, H, K, 1e-4), _lib.MDNConfigC(D, C, 0, K, 1e-4),
                _lib.MDNConfigC(D, C, H, 0, 1e-4)):
        assert lib.sbi_amd_mdn_param_count(bad) == _lib.E_UNSUPPORTED      # anything outside the envelope
    assert lib.sbi_amd_mdn_param_count(_lib.MDNConfigC(D, C, H, K, -1.0)) == _lib.E_BADARG
    assert lib.sbi_amd_mdn_param_count(None) == _lib.E_BADARG


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "sbi_amd_mdn.h")).read()
    declared = set(re.findall(r"\b(sbi_amd_mdn_[a-z_]+)\s*\(", text))
    assert declared == set(_lib.exported_symbols_mdn()) and len(declared) == 9
    assert not declared & set(_lib.exported_symbols())


@pytest.mark.parametrize("case", ["d3", "d1"])
def test_state_dict_round_trip_in_the_reference_keys(case):
    c = torch.load(GOLDEN)[case]
    est = build_mdn(c["theta"], c["x"], hidden_features=c["H"], num_components=c["K"])
    sd = est.state_dict()
    assert list(sd) == list(c["state_dict"])
    assert all(sd[k].shape == v.shape for k, v in c["state_dict"].items())
    # z-scoring statistics of the same batch: the same buffers as the reference computed
    for k in ("_transform_shift", "_transform_scale", "_embedding_net.0._mean", "_embedding_net.0._std"):
        assert torch.allclose(sd[k], c["state_dict"][k], atol=1e-6), k
    est.load_state_dict(c["state_dict"], strict=True)
    back = est.state_dict()
    assert all(torch.equal(back[k], v) for k, v in c["state_dict"].items())
    o = MDNOracle(c["D"], c["C"], c["H"], c["K"])
    o.load_state_dict(back, strict=True)
    assert torch.equal(o.flat_params(), est.net.flat_params.detach())
    # the kernels' own two-tensor form loads too
    est.net._native_state_dict = True
    try:
        native = est.state_dict()
    finally:
        est.net._native_state_dict = False
    assert set(native) == {"net.flat_params", "net.zstats"}
    est2 = build_mdn(c["theta"] * 2, c["x"] + 1, hidden_features=c["H"], num_components=c["K"])
    est2.load_state_dict(native)
    assert all(torch.equal(est2.state_dict()[k], v) for k, v in c["state_dict"].items())
    with pytest.raises(RuntimeError):
        bad = dict(c["state_dict"])
        bad["net._means_layer.weight"] = bad["net._means_layer.weight"][:-1]
        est.load_state_dict(bad)


def test_initialisation_constants():
    torch.manual_seed(0)
    theta, x = _data(D=4, C=3)
    eps = 1e-4
    sd = build_mdn(theta, x).state_dict()
    assert torch.allclose(sd["net._unconstrained_diagonal_layer.bias"],
                          torch.full((40,), math.log(math.exp(1 - eps) - 1)), atol=1e-7)
    assert (sd["net._upper_layer.bias"] == 0).all()
    for k in ("net._logits_layer.weight", "net._logits_layer.bias", "net._unconstrained_diagonal_layer.weight",
              "net._upper_layer.weight"):
        assert sd[k].abs().max() < 6 * eps and 0.5 * eps < sd[k].std() < 2 * eps, k
    bound = 1 / math.sqrt(50)           # torch's Linear default on the rest
    assert 0.5 * bound < sd["net._means_layer.weight"].abs().max() <= bound
    assert 0.5 * bound < sd["net._hidden_net.2.weight"].abs().max() <= bound


def test_multi_round_training_is_refused_naming_single_round_npe():
    from torch.distributions import MultivariateNormal

    from sbi_amd.inference import NPE

    prior = MultivariateNormal(torch.zeros(2), torch.eye(2))
    theta = prior.sample((300,))
    x = theta + 0.1 * torch.randn(300, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inf = NPE(prior=prior, density_estimator="mdn", show_progress_bars=False)
        assert isinstance(NPE(prior=prior, density_estimator=MDNConfig())._build_neural_net(theta, x),
                          MixtureDensityEstimator)
        inf.append_simulations(theta, x)
        inf._neural_net = inf._build_neural_net(theta, x)       # as after a first round
        inf.append_simulations(theta, x, proposal=prior.__class__(torch.zeros(2), 0.5 * torch.eye(2)))
        with pytest.raises(NotImplementedError, match="single-round NPE"):
            inf.train(max_num_epochs=1)
