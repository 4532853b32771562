"""The affine MAF end to end: NPE on the linear-Gaussian task (sizes and C2ST threshold of the maf_rqs end-to-end
test in tests/test_maf_gpu.py), NLE with MCMC and with rejection on iid trials (task, sizes and acceptance criterion
of tests/test_nle_gpu.py::test_c2st_nle_on_linear_gaussian), and the batched / SBC / MAP surfaces."""
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd.inference import NLE, NPE
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential
from sbi_amd.neural_nets import MAFConfig
from sbi_amd.neural_nets.estimators.maf_affine_flow import MAFFlow
from sbi_amd.simulators.linear_gaussian import linear_gaussian, true_posterior_linear_gaussian_mvn_prior
from sbi_amd.utils.metrics import c2st
from tests.parity_log import record

pytestmark = pytest.mark.gpu


def _check_c2st_recorded(samples, target, alg, tol):
    """sbi_amd.utils.metrics.check_c2st, with the score kept in the parity record."""
    score = c2st(samples, target).item()
    print(f"c2st for {alg} is {score:.2f}.")
    record("c2st", alg, c2st=score)
    assert (0.5 - tol) <= score <= (0.5 + tol), f"{alg}'s c2st={score:.2f} is too far from chance"


def test_npe_with_mafconfig_recovers_the_linear_gaussian_posterior():
    from sbi_amd.diagnostics import run_sbc

    dim, n = 3, 3000
    torch.manual_seed(0)
    shift, cov = -1.0 * torch.ones(dim), 0.3 * torch.eye(dim)
    prior = MultivariateNormal(torch.zeros(dim, device="cuda"), torch.eye(dim, device="cuda"))
    theta = prior.sample((n,)).cpu()
    x = linear_gaussian(theta, shift, cov)
    x_o = torch.zeros(1, dim)
    target = true_posterior_linear_gaussian_mvn_prior(x_o, shift, cov, torch.zeros(dim), torch.eye(dim)).sample((1000,))
    torch.manual_seed(1)
    inf = NPE(prior=prior, density_estimator=MAFConfig(), device="cuda", show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = inf.append_simulations(theta, x).train(training_batch_size=100)
    assert isinstance(est, MAFFlow)
    assert inf._stepper is not None          # the fused device-resident step trained it
    post = inf.build_posterior().set_default_x(x_o)
    samples = post.sample((1000,), show_progress_bars=False).cpu()
    score = c2st(samples, target).item()
    print(f"maf NPE c2st={score:.3f} epochs={inf.summary['epochs_trained'][-1]}")
    record("c2st", "maf (affine) dim3 2.7k sims", c2st=score)
    assert 0.4 <= score <= 0.6
    assert torch.isfinite(post.log_prob(samples[:5].cuda())).all()
    # batched sampling, SBC and MAP run on the estimator and return finite values of the right shape
    sb = post.sample_batched((4,), x[:3].cuda(), show_progress_bars=False)
    assert sb.shape == (4, 3, dim) and torch.isfinite(sb).all()
    ranks, dap = run_sbc(theta[:20], x[:20], post, num_posterior_samples=50, show_progress_bar=False)
    assert ranks.shape == (20, dim) and torch.isfinite(ranks.float()).all() and torch.isfinite(dap).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = post.map(num_iter=50, num_init_samples=200, num_to_optimize=20, show_progress_bars=False)
    assert m.reshape(-1).shape == (dim,) and torch.isfinite(m).all()


def test_nle_with_mafconfig_mcmc_and_rejection_on_iid_trials():
    num_dim, num_samples, num_simulations = 2, 500, 3000
    shift, cov = -1.0 * torch.ones(num_dim), 0.8 * torch.eye(num_dim)
    torch.manual_seed(0)
    prior = MultivariateNormal(torch.zeros(num_dim, device="cuda"), torch.eye(num_dim, device="cuda"))
    theta = prior.sample((num_simulations,)).cpu()
    x = linear_gaussian(theta, shift, cov)
    inf = NLE(prior=prior, density_estimator=MAFConfig(num_transforms=3), device="cuda", show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        estimator = inf.append_simulations(theta, x).train(training_batch_size=100)
    assert isinstance(estimator, MAFFlow) and estimator.input_shape == (num_dim,)
    assert inf._stepper is not None

    for num_trials in (1, 5):
        x_o = torch.zeros(num_trials, num_dim)
        target = true_posterior_linear_gaussian_mvn_prior(x_o, shift, cov, torch.zeros(num_dim),
                                                          torch.eye(num_dim)).sample((num_samples,))
        potential_fn, theta_transform = likelihood_estimator_based_potential(estimator, prior, x_o.cuda())
        posterior = MCMCPosterior(potential_fn, prior, theta_transform, num_chains=20, thin=3, warmup_steps=100,
                                  init_strategy="resample", device="cuda")
        samples = posterior.sample((num_samples,), x=x_o, show_progress_bars=False)
        assert samples.shape == (num_samples, num_dim) and torch.isfinite(samples).all()

        # trials kernel and generic (expand, log_prob, sum) potentials at the same theta
        th = samples[:200].contiguous()
        potential_fn.set_x(x_o.cuda())
        fused = potential_fn(th, track_gradients=False)
        generic = potential_fn(th, track_gradients=True).detach()
        rows = estimator.log_prob(x_o.cuda().unsqueeze(1).expand(-1, th.shape[0], -1), condition=th).detach()
        tol = 4e-5 * (1.0 + rows.abs()).sum(0) + 1e-5 * prior.log_prob(th).abs()
        assert bool(((fused - generic).abs() <= tol).all())
        _check_c2st_recorded(samples.cpu(), target, f"nle-maf-{num_dim}d-{num_trials}trials",
                             0.1 if num_trials == 1 else 0.25)

    # rejection sampling on the same potential (five iid trials)
    rej = inf.build_posterior(sample_with="rejection").set_default_x(x_o)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = rej.sample((num_samples,), show_progress_bars=False)
    assert r.shape == (num_samples, num_dim) and torch.isfinite(r).all()
    _check_c2st_recorded(r.cpu(), target, f"nle-maf-rejection-{num_dim}d-5trials", 0.25)
