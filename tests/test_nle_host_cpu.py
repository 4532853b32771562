"""NLE's host side without a GPU: the likelihood_nn factory's roles, the refusals, the potential's x_o handling and its
generic (expand, log_prob, sum over trials) evaluation on the CPU oracle, and the posterior's deepcopy / pickle."""
import pickle
from copy import deepcopy

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd.inference import NLE, NLE_A, SNLE
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
from sbi_amd.inference.potentials.likelihood_based_potential import (LikelihoodBasedPotential,
                                                                     likelihood_estimator_based_potential)
from sbi_amd.neural_nets import NSFConfig, ZukoNSFConfig, likelihood_nn
from sbi_amd.utils.torchutils import BoxUniform
from tests.oracle_adapter import OracleEstimator


def test_aliases():
    assert NLE is NLE_A and SNLE is NLE_A


@pytest.mark.parametrize("zx,zt", [("independent", "none"), ("none", "independent"), ("structured", "independent")])
def test_likelihood_nn_roles(zx, zt):
    """x is the flow input (z_score_x), theta the condition (z_score_theta): factory.py:244-315."""
    torch.manual_seed(0)
    theta = torch.randn(300, 3) * 2 + 1
    x = torch.randn(300, 5) * 0.5 - 2
    est = likelihood_nn("nsf", z_score_x=zx, z_score_theta=zt, hidden_features=20, num_transforms=2)(theta, x)
    assert tuple(est.input_shape) == (5,) and tuple(est.condition_shape) == (3,)
    h = est.net.hyper
    assert (h.D, h.C, h.hidden_features, h.num_transforms) == (5, 3, 20, 2)
    D, C = 5, 3
    z = est.net.zstats
    shift, scale, mean, std = z[:D], z[D:2 * D], z[2 * D:2 * D + C], z[2 * D + C:]
    if zx == "none":
        assert torch.equal(shift, torch.zeros(D)) and torch.equal(scale, torch.ones(D))
    else:
        assert not torch.equal(scale, torch.ones(D))       # the input (x) is z-scored
    if zt == "none":
        assert torch.equal(mean, torch.zeros(C)) and torch.equal(std, torch.ones(C))
    else:
        assert torch.allclose(mean, theta.mean(0), atol=1e-5)


@pytest.mark.parametrize("model", ["maf", "mdn", "made", "maf_rqs", "zuko_nsf", "zuko_maf"])
def test_likelihood_nn_refuses_other_models(model):
    with pytest.raises(NotImplementedError, match="nsf"):
        likelihood_nn(model)


def test_nle_refusals():
    prior = BoxUniform(-torch.ones(2), torch.ones(2))
    with pytest.raises(NotImplementedError, match="density_estimator='nsf'"):
        NLE(prior)
    with pytest.raises(NotImplementedError, match="nsf"):
        NLE(prior, density_estimator="maf")
    with pytest.raises(NotImplementedError, match="nsf"):
        NLE(prior, density_estimator=ZukoNSFConfig())
    inf = NLE(prior, density_estimator=NSFConfig(hidden_features=8, num_transforms=1))
    for kind in ("vi", "importance"):
        with pytest.raises(NotImplementedError, match="outside"):
            inf.build_posterior(sample_with=kind)


def test_nle_config_builds_the_likelihood_estimator():
    inf = NLE(density_estimator=NSFConfig(hidden_features=8, num_transforms=1))
    est = inf._build_neural_net(torch.randn(50, 2), torch.randn(50, 4))
    assert tuple(est.input_shape) == (4,) and tuple(est.condition_shape) == (2,)


def test_append_simulations_rounds_and_invalid_x():
    inf = NLE(density_estimator="nsf")
    theta, x = torch.randn(10, 2), torch.randn(10, 3)
    x[3, 0] = float("nan")
    inf.append_simulations(theta, x)                               # kept: exclude_invalid_x=False by default
    inf.append_simulations(theta, x, exclude_invalid_x=True, from_round=1)
    th, xx, masks = inf.get_simulations()
    assert th.shape[0] == 19 and inf._data_round_index == [0, 1]
    assert masks[:10].all() and not masks[10:].any()
    assert inf._input_condition(th, xx)[0] is xx


def _oracle_potential(num_trials=4, num_theta=6):
    torch.manual_seed(3)
    theta = torch.randn(200, 2)
    x = theta @ torch.randn(2, 3) + 0.3 * torch.randn(200, 3)
    est = OracleEstimator(x, theta, hidden_features=16, num_transforms=2)      # q(x | theta)
    prior = MultivariateNormal(torch.zeros(2), torch.eye(2))
    x_o = torch.randn(num_trials, 3)
    th = torch.randn(num_theta, 2)
    return est, prior, x_o, th


def test_set_x_defaults_to_iid():
    est, prior, x_o, _ = _oracle_potential()
    pot = LikelihoodBasedPotential(est, prior)
    pot.set_x(x_o)
    assert pot.x_is_iid is True
    pot.set_x(x_o, x_is_iid=False)
    assert pot.x_is_iid is False
    with pytest.raises(ValueError):
        LikelihoodBasedPotential(est, prior).x_o


def test_potential_is_the_loop_over_trials_plus_prior():
    est, prior, x_o, th = _oracle_potential()
    pot, transform = likelihood_estimator_based_potential(est, prior, x_o)
    assert pot.x_is_iid
    got = pot(th, track_gradients=False)
    with torch.no_grad():
        ref = torch.zeros(th.shape[0])
        for i in range(x_o.shape[0]):
            ref += est.log_prob(x_o[i : i + 1].expand(th.shape[0], -1).unsqueeze(0), condition=th)[0]
        ref += prior.log_prob(th)
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-5)
    # the non-iid branch: one (x_i, theta_i) pair per row
    pot.set_x(x_o[:3], x_is_iid=False)
    paired = pot(th[:3], track_gradients=False)
    with torch.no_grad():
        ref = est.log_prob(x_o[:3].unsqueeze(0), condition=th[:3])[0] + prior.log_prob(th[:3])
    assert torch.allclose(paired, ref)
    with pytest.raises(ValueError, match="Batch size mismatch"):
        pot(th, track_gradients=False)
    # the transform is mcmc_transform(prior): constrained -> unconstrained
    assert torch.allclose(transform.inv(transform(th)), th, atol=1e-5)


def test_potential_outside_a_box_prior_is_minus_inf():
    est, _, x_o, _ = _oracle_potential()
    prior = BoxUniform(-torch.ones(2), torch.ones(2))
    pot = LikelihoodBasedPotential(est, prior, x_o)
    v = pot(torch.tensor([[0.0, 0.0], [1.5, 0.0], [0.0, -3.0]]), track_gradients=False)
    assert torch.isfinite(v[0]) and torch.isneginf(v[1:]).all()


def test_posterior_survives_deepcopy_and_pickle():
    est, prior, x_o, th = _oracle_potential()
    pot, transform = likelihood_estimator_based_potential(est, prior, None)
    post = MCMCPosterior(pot, prior, transform, num_chains=4, device="cpu").set_default_x(x_o)
    for other in (deepcopy(post), pickle.loads(pickle.dumps(post))):
        assert torch.allclose(other.potential(th), post.potential(th))
