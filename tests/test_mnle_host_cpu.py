"""Host side of MNLE without a GPU: builders, config validation, category inference and value <-> index mapping, the
reference's warnings and errors, the state_dict round trip into the eager restatement, every refusal by message, the
MNLE constructor paths, and that the refusals pinned elsewhere are unchanged."""
import warnings

import pytest
import torch
from torch import nn

from sbi_amd.neural_nets import MAFRQSConfig, MixedConfig, NSFConfig, likelihood_nn, posterior_nn
from sbi_amd.neural_nets.estimators.mixed_density_estimator import (MixedDensityEstimator, MNLEHyper,
                                                                    map_values_to_indices)
from sbi_amd.neural_nets.net_builders.mixed_nets import build_mnle, build_mnpe
from tests.mnle_oracle import MixedOracle


def data(n=200, values=((-1.0, 1.0), (0.0, 2.0, 5.0)), C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(n, C, generator=g)
    cols = []
    for vals in values:
        v = torch.tensor(vals)
        idx = torch.randint(0, len(vals), (n,), generator=g)
        idx[: len(vals)] = torch.arange(len(vals))
        cols.append(v[idx])
    x = torch.cat([torch.rand(n, 1, generator=g) + 0.2, torch.stack(cols, 1)], 1)
    return theta, x


def quiet_build(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return build_mnle(*a, **k)


def test_builder_infers_categories_and_keeps_the_reference_warnings():
    theta, x = data()
    with pytest.warns(UserWarning) as rec:
        est = build_mnle(x, theta)
    msgs = [str(w.message) for w in rec]
    assert any("continuous data in the first n-k columns" in m for m in msgs)
    assert any("Inferring num_categories from batch_x" in m for m in msgs)
    assert isinstance(est, MixedDensityEstimator)
    h = est.net.hyper
    assert h.num_categories == (2, 3) and h.C == 3 and h.tail_bound == 10.0
    assert (h.discrete_hidden, h.discrete_blocks, h.embedding, h.hidden, h.num_bins, h.num_transforms) == \
        (50, 2, 50, 50, 10, 5)
    assert est.input_shape == (3,) and est.condition_shape == (3,)
    assert torch.equal(est.net.lookup[0, :2], torch.tensor([-1.0, 1.0]))
    assert torch.equal(est.net.lookup[1, :3], torch.tensor([0.0, 2.0, 5.0]))
    with warnings.catch_warnings(record=True) as rec2:
        warnings.simplefilter("always")
        build_mnle(x, theta, num_categories_per_variable=torch.tensor([2, 3]))
    assert not any("Inferring" in str(w.message) for w in rec2)
    with pytest.raises(NotImplementedError, match="forward method is not implemented"):
        est.forward(x)


def test_widths_fall_back_as_in_the_reference():
    theta, x = data()
    est = quiet_build(x, theta, hidden_features=32, discrete_hidden_features=16, combined_embedding_features=24,
                      discrete_hidden_layers=1, num_transforms=2, num_bins=8, log_transform_x=True)
    h = est.net.hyper
    assert (h.discrete_hidden, h.discrete_blocks, h.embedding, h.hidden, h.num_bins, h.num_transforms) == \
        (16, 1, 24, 32, 8, 2)
    assert h.log_transform and est.log_transform_input
    cfg = MixedConfig(continuous=NSFConfig(tail_bound=10.0, hidden_features=40, num_transforms=3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = cfg.build(x, theta).net.hyper
    assert (h.discrete_hidden, h.embedding, h.hidden, h.num_transforms) == (40, 40, 40, 3)
    assert MixedConfig().continuous.tail_bound == 10.0


def test_value_index_mapping_and_the_unseen_value_error():
    theta, x = data()
    est = quiet_build(x, theta)
    vals = torch.tensor([[-1.0, 5.0], [1.0, 0.0], [1.0, 2.0]])
    assert map_values_to_indices(est.net, vals).tolist() == [[0, 2], [1, 0], [1, 1]]
    with pytest.raises(ValueError, match="Variable 1 contains values not seen during training"):
        map_values_to_indices(est.net, torch.tensor([[-1.0, 7.0]]))
    with pytest.raises(ValueError, match="Variable 0 contains values not seen during training"):
        map_values_to_indices(est.net, torch.tensor([[0.0, 2.0]]))          # between two seen values


def test_state_dict_round_trips_into_the_restatement():
    theta, x = data()
    est = quiet_build(x, theta, hidden_features=16, num_transforms=2, num_bins=4, hidden_layers_spline_context=2,
                      log_transform_x=True)
    sd = est.state_dict()
    for key in ("discrete_net.net.initial_layer.weight", "discrete_net.net.blocks.0.linear_layers.1.bias",
                "discrete_net.net.blocks.0.context_layer.weight", "discrete_net.net.mask",
                "discrete_net.net.initial_layer.degrees", "discrete_net.net.values_lookup",
                "continuous_net.net._embedding_net.0.weight",
                "continuous_net.net._transform._transforms.1.transform_net.spline_predictor.0.weight"):
        assert key in sd, key
    oracle = MixedOracle([2, 3], [torch.tensor([-1.0, 1.0]), torch.tensor([0.0, 2.0, 5.0])], 3, 16, 2, 16, 16, 4, 2,
                         2, 10.0, True)
    res = oracle.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(oracle.flat_params(), est.net.flat_params.detach())
    assert torch.equal(oracle.discrete_net.net.initial_layer.mask, est.net.hyper.made_mask("initial"))
    assert torch.equal(oracle.discrete_net.net.final_layer.mask, est.net.hyper.made_mask("final"))
    # and back: perturbed restatement weights load under the reference's names
    with torch.no_grad():
        for p in oracle.parameters():
            p.add_(0.1)
    est.load_state_dict(oracle.state_dict())
    assert torch.equal(oracle.flat_params(), est.net.flat_params.detach())
    lp = oracle.log_prob(x[:5], theta[:5])          # the loaded restatement evaluates
    assert lp.shape == (5,) and torch.isfinite(lp).all()
    n_small = sum(1 for k, _, _ in est.net.hyper.linears() if k.endswith("linear_layers.1"))
    assert n_small == 2


def test_fresh_blocks_start_near_the_identity():
    theta, x = data()
    est = quiet_build(x, theta)
    for key, off, n, shape in est.net._slices():
        if ".linear_layers.1." in key:
            assert est.net.flat_params[off: off + n].abs().max() <= 1e-3


@pytest.mark.parametrize("kwargs, match", [
    (dict(flow_model="maf"), "NSF only"),
    (dict(dropout_probability=0.1), "dropout_probability > 0"),
    (dict(combined_embedding_net=nn.Linear(5, 5)), "custom combined_embedding_net"),
    (dict(hidden_features=65), "envelope"),
    (dict(num_bins=7), "envelope"),
])
def test_builder_refusals_name_the_alternative(kwargs, match):
    theta, x = data()
    with pytest.raises(NotImplementedError, match=match):
        quiet_build(x, theta, **kwargs)


def test_data_shape_refusals():
    theta, x = data()
    two_cont = torch.cat([x[:, :1] + 0.123, x], 1)
    with pytest.raises(NotImplementedError, match="exactly one continuous column"):
        quiet_build(two_cont, theta)
    with pytest.raises(NotImplementedError, match="exactly one continuous column"):
        quiet_build(x[:, 1:], theta)                                    # no continuous column
    five = torch.cat([x, x[:, 1:], x[:, 1:2]], 1)
    with pytest.raises(NotImplementedError, match="1..4 discrete columns"):
        quiet_build(five, theta)
    many = x.clone()
    many[:, 2] = torch.arange(200) % 17
    with pytest.raises(NotImplementedError, match="at most 16 categories"):
        quiet_build(many, theta)
    wide = nn.Sequential(nn.Linear(3, 65))
    with pytest.raises(NotImplementedError, match="wider than 64"):
        quiet_build(x, theta, embedding_net=wide)
    with pytest.raises(NotImplementedError, match="MNPE"):
        build_mnpe(x, theta)


def test_mixed_config_validation():
    with pytest.raises(NotImplementedError, match="NSF only"):
        MixedConfig(continuous=MAFRQSConfig())
    with pytest.raises(NotImplementedError, match="dropout"):
        MixedConfig(dropout_probability=0.2)
    with pytest.raises(NotImplementedError, match="combined_embedding_net"):
        MixedConfig(combined_embedding_net=nn.Identity())
    with pytest.raises(ValueError, match="z_score_condition"):
        MixedConfig(z_score_condition="bogus")
    with pytest.raises(ValueError, match="replaced when its mixed condition is built"):
        MixedConfig(continuous=NSFConfig(z_score_condition="none"))
    with pytest.raises(ValueError, match="extra_kwargs"):
        MixedConfig(extra_kwargs={"a": 1})


def test_mnle_constructor_paths():
    from sbi_amd.inference import MNLE
    from sbi_amd.inference.potentials.likelihood_based_potential import (LikelihoodBasedPotential,
                                                                         MixedLikelihoodBasedPotential,
                                                                         mixed_likelihood_estimator_based_potential)

    theta, x = data()
    inf = MNLE()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert isinstance(inf._build_neural_net(theta, x), MixedDensityEstimator)
    with pytest.warns(FutureWarning, match="deprecated"):
        inf = MNLE(density_estimator="mnle")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert isinstance(inf._build_neural_net(theta, x), MixedDensityEstimator)
    with pytest.raises(ValueError, match="MNLE supports only the preconfigured 'mnle' density estimator"):
        MNLE(density_estimator="nsf")
    with pytest.raises(TypeError):
        MNLE(density_estimator=3)
    inf = MNLE(density_estimator=MixedConfig(log_transform_x=True))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = inf._build_neural_net(theta, x)
    assert est.log_transform_input
    for bad in ("vi", "importance"):
        with pytest.raises(NotImplementedError, match="'mcmc' or 'rejection'"):
            inf.build_posterior(density_estimator=est, sample_with=bad)
    assert issubclass(MixedLikelihoodBasedPotential, LikelihoodBasedPotential)
    prior = torch.distributions.Independent(torch.distributions.Normal(torch.zeros(3), torch.ones(3)), 1)
    with pytest.warns(DeprecationWarning):
        pot, _ = mixed_likelihood_estimator_based_potential(est, prior, None)
    assert type(pot) is LikelihoodBasedPotential
    with pytest.warns(DeprecationWarning):
        mixed = MixedLikelihoodBasedPotential(est, prior)
    with pytest.raises(NotImplementedError, match="condition_on_theta"):
        mixed.condition_on_theta()


def test_the_kernels_are_required():
    """No CPU fallback: a CPU tensor is an error, not a quiet eager evaluation."""
    theta, x = data()
    est = quiet_build(x, theta)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.log_prob(x[:4], theta[:4])


def test_pinned_refusals_are_unchanged():
    for model in ("maf", "mdn", "made", "maf_rqs", "zuko_nsf"):
        with pytest.raises(NotImplementedError, match="'nsf' likelihood estimator only"):
            likelihood_nn(model)
    with pytest.raises(NotImplementedError):
        posterior_nn("maf")(torch.randn(10, 2), torch.randn(10, 2))
    assert callable(likelihood_nn("mnle")) and callable(likelihood_nn("nsf"))


def test_hyper_layout_matches_the_library():
    """The Python flat layout and the library's param_offset agree (host-only entry points: no GPU needed)."""
    from sbi_amd import _lib

    lib = _lib.load()
    h = MNLEHyper(num_categories=(16, 2, 7, 16), C=64, discrete_hidden=64, discrete_blocks=4, embedding=64, hidden=64,
                  num_bins=16, num_transforms=8, context_layers=2)
    cfg = h.c_config()
    assert lib.sbi_amd_mnle_param_count(cfg) == h.param_count()
    off = 0
    for i, (_, o, n_in) in enumerate(h.linears()):
        assert lib.sbi_amd_mnle_param_offset(cfg, i, 0) == off
        assert lib.sbi_amd_mnle_param_offset(cfg, i, 1) == off + o * n_in
        off += o * n_in + o
    assert lib.sbi_amd_mnle_param_offset(cfg, len(h.linears()), 0) == _lib.E_BADARG
