"""Importance sampling, SIR and truncated proposals on the device: `ImportanceSamplingPosterior` over an NLE (NSF)
and an NRE potential, its batched sampling under `run_sbc`, the device selection against the torch path on the same
candidates, and one TSNPE round (`get_density_thresholder` + `RestrictedPrior`) for the MDN and the affine MAF, which
have no other multi-round route.  Tiny nets, a few hundred simulations, at most three epochs: nothing here asserts
the quality of a fit."""
import functools
import warnings

import pytest
import torch

from sbi_amd.diagnostics import run_sbc
from sbi_amd.inference import NLE, NPE, NRE_B, ImportanceSamplingPosterior
from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential
from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential
from sbi_amd.neural_nets import MAFConfig, MDNConfig, NSFConfig, classifier_nn
from sbi_amd.samplers.importance import sampling_importance_resampling, sir_select
from sbi_amd.simulators.linear_gaussian import linear_gaussian
from sbi_amd.utils import BoxUniform, RestrictedPrior, get_density_thresholder
from sbi_amd.utils.sbiutils import within_support

pytestmark = pytest.mark.gpu

DIM = 2


def simulate(prior, n):
    theta = prior.sample((n,)).cpu()
    return theta, linear_gaussian(theta, -0.5 * torch.ones(DIM), 0.5 * torch.eye(DIM))


@functools.lru_cache(maxsize=None)
def trained(kind):
    torch.manual_seed(3)
    prior = BoxUniform(-2.0 * torch.ones(DIM), 2.0 * torch.ones(DIM), device="cuda")
    theta, x = simulate(prior, 400)
    if kind == "nle":
        inf = NLE(prior=prior, density_estimator=NSFConfig(hidden_features=16, num_transforms=2), device="cuda",
                  show_progress_bars=False)
    else:
        inf = NRE_B(prior=prior, classifier=classifier_nn("resnet", hidden_features=16, num_blocks=1), device="cuda",
                    show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = inf.append_simulations(theta, x).train(max_num_epochs=3, training_batch_size=100)
    build = likelihood_estimator_based_potential if kind == "nle" else ratio_estimator_based_potential
    potential_fn, transform = build(est, prior, None)
    post = ImportanceSamplingPosterior(potential_fn, prior, theta_transform=transform)
    return post.set_default_x(torch.zeros(1, DIM)), prior, theta, x


@pytest.mark.parametrize("kind", ["nle", "nre"])
def test_importance_posterior_samples_on_the_device(kind):
    post, prior, theta, x = trained(kind)
    torch.manual_seed(5)
    s = post.sample((500,))
    assert s.shape == (500, DIM) and s.is_cuda and torch.isfinite(s).all() and bool(within_support(prior, s).all())
    torch.manual_seed(5)
    assert torch.equal(post.sample((500,)), s)                        # reproducible under torch.manual_seed
    assert post.sample((2, 3), oversampling_factor=100).shape == (2, 3, DIM)          # the one-wave-per-row kernel
    th, lw = post.sample((64,), method="importance")
    assert th.shape == (64, DIM) and lw.shape == (64,) and lw.is_cuda
    lp = post.log_prob(s[:10], normalization_constant_params=dict(num_samples=2000))
    assert lp.shape == (10,) and torch.isfinite(lp).all()
    b = post.sample_batched((50,), x[:8].cuda())
    assert b.shape == (50, 8, DIM) and b.is_cuda and torch.isfinite(b).all() and bool(
        within_support(prior, b.reshape(-1, DIM)).all())
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="Batched sampling not implemented")      # no per-observation loop
        warnings.filterwarnings("ignore", message="Number of")
        ranks, dap = run_sbc(theta[:8], x[:8], post, num_posterior_samples=50, show_progress_bar=False)
    assert ranks.shape == (8, DIM) and torch.isfinite(dap).all()


@pytest.mark.parametrize("K", [32, 100])
def test_device_route_and_torch_path_pick_the_same_winners(K):
    """Same candidates, weights and uniforms through the kernel and through `_select_torch` on the host; rows within
    1e-5 (in cumulative weight, fp64) of a boundary are left out, at most 2 % of them."""
    post, prior, _, _ = trained("nle")
    B = 2000
    torch.manual_seed(8)
    post.potential_fn.set_x(post.default_x)
    theta = prior.sample((B * K,))
    log_p, log_q = post.potential_fn(theta).reshape(B, K), prior.log_prob(theta).reshape(B, K)
    cand, u = theta.reshape(B, K, DIM), torch.rand(B, device="cuda")
    dev = sir_select(log_p, log_q, cand, u)
    host = sir_select(log_p.cpu(), log_q.cpu(), cand.cpu(), u.cpu())
    c = torch.softmax((log_p.double() - log_q.double()).cpu(), -1).cumsum(-1)
    keep = ((c - u.cpu().double().unsqueeze(-1)).abs() >= 1e-5).all(-1)
    assert keep.float().mean() >= 0.98
    assert torch.equal(dev[1].cpu()[keep], host[1][keep])
    assert torch.equal(dev[0].cpu()[keep], host[0][keep])
    assert int(dev[2].item()) == int(host[2].item()) == 0


def test_the_loop_on_the_device_refills_after_dead_rows():
    proposal = BoxUniform(-torch.ones(DIM), torch.ones(DIM), device="cuda")

    def potential(theta):
        return torch.where(theta[:, 0] > 0, torch.zeros_like(theta[:, 0]), torch.full_like(theta[:, 0], -float("inf")))

    s = sampling_importance_resampling(potential, proposal, num_samples=3000, num_candidate_samples=1,
                                       max_sampling_batch_size=1000)
    assert s.shape == (3000, DIM) and s.is_cuda and (s[:, 0] > 0).all()


@pytest.mark.parametrize("config", [MDNConfig, MAFConfig])
def test_tsnpe_round_with_a_truncated_proposal(config):
    torch.manual_seed(4)
    prior = BoxUniform(-2.0 * torch.ones(DIM), 2.0 * torch.ones(DIM), device="cuda")
    theta, x = simulate(prior, 500)
    inf = NPE(prior=prior, density_estimator=config(), device="cuda", show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inf.append_simulations(theta, x).train(max_num_epochs=3, training_batch_size=100)
        posterior = inf.build_posterior().set_default_x(torch.zeros(1, DIM))
        accept = get_density_thresholder(posterior, 1e-4, 20_000)
        restricted = RestrictedPrior(prior, accept, posterior, "rejection", device="cuda")
        theta2 = restricted.sample((300,), print_rejected_frac=False)
        assert theta2.shape == (300, DIM) and bool(accept(theta2).all()) and bool(within_support(prior, theta2).all())
        assert accept(theta2).dtype == torch.bool
        x2 = linear_gaussian(theta2.cpu(), -0.5 * torch.ones(DIM), 0.5 * torch.eye(DIM))
        inf.append_simulations(theta2.cpu(), x2, proposal=restricted)
        assert inf._data_round_index == [0, 0]                          # truncation: still the first-round loss
        inf.train(max_num_epochs=2, training_batch_size=100, force_first_round_loss=True)
        assert torch.isfinite(inf.build_posterior().set_default_x(torch.zeros(1, DIM)).sample((10,))).all()
        if config is MDNConfig:
            sir = restricted.sample((120,), sample_with="sir", oversampling_factor=64)
            assert sir.shape == (120, DIM) and torch.isfinite(sir).all()
            lp = restricted.log_prob(theta2[:5], prior_acceptance_params=dict(num_rejection_samples=500))
            assert torch.isfinite(lp).all()
