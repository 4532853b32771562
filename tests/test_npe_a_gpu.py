"""NPE-A end to end on the device: rounds of maximum-likelihood training through the fused MDN step, then the analytic
MoG correction (sbi_amd_mog_correct / _log_prob / _sample) behind ``NPE_A_Posterior``.

Task: the linear-Gaussian model of tests.helpers at theta-dim 3 -- theta ~ N(0, 0.1 I), x = theta + N(0, 0.1 I) -- so
the posterior at x_o is N(x_o / 2, 0.05 I), std 0.2236 per coordinate.  Round 2 is proposed from the round-1 posterior
at x_o; its network alone learns the PROPOSAL posterior (precision about 2 * 20 - 10 = 30, std 0.18), the correction
brings it back.

Fixed configuration: 3000 simulations per round, training batch 100, torch seeds `seed`, `seed + 1 + round`.  The
accuracy tests run NPE-A as the paper does, with ONE Gaussian component (num_components = 1): then the proposal is a
single Gaussian and q prior / proposal is exactly a Gaussian.  With K >= 2 the L K-component formula (sbi's, and this
package's) treats 1 / proposal as if the proposal were one of its components at a time; on this Gaussian target the
split of the fitted mixtures into components is not identified, and P_d - P_p + P_0 of two fitted components was not
positive definite for some pair by round 3 at K = 2 for 15 of the seeds 0 .. 27, and at K = 4 for every one of the
seeds 0 .. 27 at 3000 simulations and 0, 1 at 10 000 (sbi's ValueError, raised as the reference raises it).  The K = 4
third-round test therefore runs on a task whose four components ARE identified: theta ~ N(0, I) in two dimensions,
x = theta^2 + 0.2 N(0, I), x_o = (1, 1), a posterior with the four modes (+-1, +-1); 10 000 simulations per round, seed 0
(all of the seeds 0 .. 5 reached a positive definite third round there; at 3000 simulations 5 of 6).  It checks that
the 64-component posterior builds, samples and evaluates, not that it is accurate: the cross-mode pairs of the L K
formula carry weight they should not have."""

import functools
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from tests.parity_log import record

pytestmark = pytest.mark.gpu

DIM, N_SIM, K = 3, 3000, 4
NOISE = 0.1


def x_obs():
    return torch.tensor([[0.3, -0.2, 0.4]])


def simulate(theta):
    return theta + NOISE**0.5 * torch.randn_like(theta)


def run_rounds(prior, num_rounds, num_components=1, n_sim=N_SIM, seed=0, simulator=simulate, x_o=None):
    from sbi_amd.inference import NPE_A

    torch.manual_seed(seed)
    inf = NPE_A(prior=prior, num_components=num_components, device="cuda", show_progress_bars=False)
    proposal, posts, data = prior, [], []
    for r in range(num_rounds):
        torch.manual_seed(seed + 1 + r)
        # (the time limit turns a corrected mixture that lies outside a box prior into an error instead of a wait)
        kw = {} if r == 0 else {"show_progress_bars": False, "max_sampling_time": 20.0}
        theta = proposal.sample((n_sim,), **kw).reshape(n_sim, -1).cpu()
        x = simulator(theta)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            inf.append_simulations(theta, x, proposal=None if r == 0 else proposal).train(training_batch_size=100)
        assert not [w for w in caught if "atomic" in str(w.message)]
        assert inf._stepper is not None          # the fused device-resident MDN step trained every round
        proposal = inf.build_posterior().set_default_x(x_obs() if x_o is None else x_o)
        posts.append(proposal)
        data.append((theta, x))
    return inf, posts, data


@functools.lru_cache(maxsize=None)
def gaussian_prior_rounds():
    prior = MultivariateNormal(torch.zeros(DIM, device="cuda"), NOISE * torch.eye(DIM, device="cuda"))
    return run_rounds(prior, 2)


def test_two_rounds_recover_the_linear_gaussian_posterior_and_the_correction_matters():
    from sbi_amd.inference import NPE_A_Posterior
    from sbi_amd.simulators.linear_gaussian import true_posterior_linear_gaussian_mvn_prior
    from sbi_amd.utils.metrics import c2st

    inf, posts, data = gaussian_prior_rounds()
    post1, post2 = posts[0], posts[1]
    assert isinstance(post2, NPE_A_Posterior) and not post1._apply_correction and post2._apply_correction
    assert post2.get_mog_params(x_obs().cuda()).num_components == 1
    target = true_posterior_linear_gaussian_mvn_prior(x_obs(), torch.zeros(DIM), NOISE * torch.eye(DIM),
                                                      torch.zeros(DIM), NOISE * torch.eye(DIM))
    torch.manual_seed(5)
    corrected = post2.sample((1000,), show_progress_bars=False).cpu()
    score = c2st(corrected, target.sample((1000,))).item()
    raw = post2.posterior_estimator.sample(torch.Size([1000]), condition=x_obs().cuda())[:, 0].cpu()
    std_true = target.covariance_matrix.diagonal().sqrt()
    err_corrected = (corrected.std(0) - std_true).abs().max().item()
    err_raw = (raw.std(0) - std_true).abs().max().item()
    print(f"NPE-A round 2: c2st={score:.3f} std error corrected {err_corrected:.4f} uncorrected {err_raw:.4f}")
    record("c2st", "npe_a dim3 2 rounds x 3k sims", c2st=score, std_err_corrected=err_corrected,
           std_err_uncorrected=err_raw)
    assert 0.4 <= score <= 0.6
    assert err_corrected < err_raw            # the round-2 network alone is the (narrower) proposal posterior
    lp = post2.log_prob(corrected[:5].cuda())
    assert lp.shape == (5,) and torch.isfinite(lp).all()
    with pytest.raises(NotImplementedError, match="map"):
        post2.map()
    with pytest.raises(ValueError, match="batchsize == 1"):
        post2.sample((2,), x=data[1][1][:2].cuda(), show_progress_bars=False)
    with pytest.raises(ValueError, match="batchsize == 1"):
        post2.log_prob(corrected[:5].cuda(), x=data[1][1][:2].cuda())


def test_batched_calls_apply_the_correction_per_observation():
    from sbi_amd.diagnostics import run_sbc

    inf, posts, data = gaussian_prior_rounds()
    post2 = posts[1]
    theta2, x2 = data[1]
    xs = x2[:3].cuda()
    torch.manual_seed(6)
    draws = post2.sample_batched((400,), xs, show_progress_bars=False)
    assert draws.shape == (400, 3, DIM)
    assert post2.sample_batched((4,), xs, show_progress_bars=False).shape == (4, 3, DIM)
    raw = post2.posterior_estimator.sample(torch.Size([400]), condition=xs)
    # the uncorrected network is the narrower proposal posterior: corrected draws spread wider for every observation
    assert (draws.std(0).mean(-1) > 1.08 * raw.std(0).mean(-1)).all()
    theta = draws[:6]
    batched = post2.log_prob_batched(theta, xs, norm_posterior=False)
    assert batched.shape == (6, 3)
    for b in range(3):
        single = post2.log_prob(theta[:, b], x=xs[b : b + 1], norm_posterior=False)
        assert (batched[:, b] - single).abs().max() <= 1e-5 * (1 + single.abs().max())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ranks, dap = run_sbc(theta2[:50], x2[:50], post2, num_posterior_samples=100, show_progress_bar=False)
    assert ranks.shape == (50, DIM) and torch.isfinite(ranks.float()).all() and torch.isfinite(dap).all()


def test_a_third_round_builds_and_samples_k_cubed_components():
    prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
    x_o = torch.ones(1, 2)
    inf, posts, data = run_rounds(prior, 3, num_components=K, n_sim=10_000, seed=0, x_o=x_o,
                                  simulator=lambda theta: theta**2 + 0.2 * torch.randn_like(theta))
    assert posts[1].get_mog_params(x_o.cuda()).num_components == K * K
    post3 = posts[2]
    mog = post3.get_mog_params(x_o.cuda())
    assert mog.num_components == K**3 and mog.logits.is_cuda
    draws = post3.sample((500,), show_progress_bars=False, max_sampling_time=20.0)
    assert draws.shape == (500, 2) and torch.isfinite(draws).all()
    assert torch.isfinite(post3.log_prob(draws[:7])).all()


def test_box_uniform_prior_runs_and_gives_finite_log_prob():
    from sbi_amd.utils.torchutils import BoxUniform

    prior = BoxUniform(-torch.ones(DIM, device="cuda"), torch.ones(DIM, device="cuda"))
    inf, posts, data = run_rounds(prior, 2)
    post2 = posts[1]
    assert post2._apply_correction and post2._prior_mog is None
    draws = post2.sample((300,), show_progress_bars=False, max_sampling_time=20.0)
    assert draws.shape == (300, DIM) and (draws.abs() <= 1).all()
    lp = post2.log_prob(draws[:9])
    assert torch.isfinite(lp).all()
    outside = post2.log_prob(torch.full((1, DIM), 2.0, device="cuda"))
    assert torch.isinf(outside).all() and (outside < 0).all()
