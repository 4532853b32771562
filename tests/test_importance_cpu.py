"""Host layer of importance sampling / SIR / truncated proposals without a GPU: signatures against the reference's
(sbi/samplers/importance/, sbi/inference/posteriors/importance_posterior.py, sbi/utils/restriction_estimator.py), the
torch selection path, the SIR loop, the normalisation constant, batched sampling, the density thresholder and
`RestrictedPrior`.  The device route of the same functions: tests/test_importance_gpu.py."""
import ctypes
import inspect
import math
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd import _build, _lib
from sbi_amd.diagnostics.sbc import run_sbc
from sbi_amd.inference import ImportanceSamplingPosterior
from sbi_amd.inference.potentials.likelihood_based_potential import LikelihoodBasedPotential
from sbi_amd.samplers.importance import importance_sample, sampling_importance_resampling, sir_select
from sbi_amd.utils import BoxUniform, RestrictedPrior, get_density_thresholder


def defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}


E = inspect.Parameter.empty


def test_signatures_and_defaults():
    assert defaults(importance_sample) == dict(potential_fn=E, proposal=E, num_samples=1, show_progress_bars=False)
    assert defaults(sampling_importance_resampling) == dict(
        potential_fn=E, proposal=E, num_samples=1, num_candidate_samples=32, max_sampling_batch_size=10_000,
        show_progress_bars=False, device="cpu", kwargs=E)
    P = ImportanceSamplingPosterior
    assert defaults(P.__init__) == dict(potential_fn=E, proposal=E, theta_transform=None, method="sir",
                                        oversampling_factor=32, max_sampling_batch_size=10_000, device=None,
                                        x_shape=None)
    assert defaults(P.sample) == dict(sample_shape=torch.Size(), x=None, method=None, oversampling_factor=32,
                                      max_sampling_batch_size=10_000, show_progress_bars=False)
    assert defaults(P.log_prob) == dict(theta=E, x=None, track_gradients=False, normalization_constant_params=None)
    assert defaults(P.estimate_normalization_constant) == dict(x=E, num_samples=10_000, force_update=False)
    assert list(defaults(P.sample_batched))[:2] == ["sample_shape", "x"]
    for name in ("map", "to", "set_default_x", "default_x", "potential"):
        assert hasattr(P, name)
    assert defaults(get_density_thresholder) == dict(dist=E, quantile=1e-4, num_samples_to_estimate_support=1_000_000)
    R = RestrictedPrior
    assert issubclass(R, torch.distributions.Distribution)
    assert defaults(R.__init__) == dict(prior=E, accept_reject_fn=E, posterior=None, sample_with="rejection",
                                        device="cpu")
    assert defaults(R.sample) == dict(sample_shape=torch.Size(), sample_with=None, max_sampling_batch_size=10_000,
                                      oversampling_factor=1024, save_acceptance_rate=False, show_progress_bars=False,
                                      print_rejected_frac=True)
    assert defaults(R.log_prob) == dict(theta=E, norm_restricted_prior=True, track_gradients=False,
                                        prior_acceptance_params=None)
    assert defaults(R.prior_acceptance) == dict(num_rejection_samples=10_000, force_update=False,
                                                show_progress_bars=False, rejection_sampling_batch_size=10_000)


def test_abi_version_and_symbol():
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    assert lib.sbi_amd_nsf_abi_version() >= 118 and _lib.ABI_VERSION >= 118
    assert hasattr(lib, "sbi_amd_sir_resample")
    assert _lib.exported_symbols_sir() == ["sbi_amd_sir_resample"]
    loaded = _lib.load()
    # host-side argument checks: nothing is launched
    assert loaded.sbi_amd_sir_resample(None, None, None, 4, 3, 2, None, 0, 0, None, None, None, None, None) == \
        _lib.E_BADARG


def test_torch_selection_rule_matches_an_fp64_restatement():
    """softmax, cumsum, first cumulative weight >= u in fp64; rows within 1e-5 of a boundary left out."""
    g = torch.Generator().manual_seed(0)
    for K in (1, 2, 31, 64, 65, 1000):
        B = 400
        lw = torch.randn(B, K, generator=g) * 3
        cand = torch.randn(B, K, 3, generator=g)
        u = torch.rand(B, generator=g)
        c = torch.softmax(lw.double(), -1).cumsum(-1)
        want = torch.argmax((c >= u.double().unsqueeze(-1)).to(torch.int8), dim=-1)
        keep = ((c - u.double().unsqueeze(-1)).abs() >= 1e-5).all(-1)
        assert keep.float().mean() >= 0.98
        out, idx, n_dead, lse = sir_select(lw, None, cand, u, return_lse=True)
        assert int(n_dead) == 0
        assert torch.equal(idx[keep].long(), want[keep])
        assert torch.equal(out, cand[torch.arange(B), idx.long()])
        assert torch.allclose(lse.double(), torch.logsumexp(lw.double(), -1), rtol=1e-5, atol=1e-5)
    # dead rows and zero weights
    inf = float("inf")
    lw = torch.randn(6, 9, generator=g)
    lw[0] = -inf
    lw[1, 4] = float("nan")
    lw[2, 8] = inf
    lw[3, :5] = -inf
    lw[4, 3:] = -inf
    u = torch.tensor([0.5, 0.5, 0.5, 0.0, 1 - 2.0**-24, 0.3])
    out, idx, n_dead = sir_select(lw, None, torch.randn(6, 9, 2, generator=g), u)
    assert idx[:3].tolist() == [-1, -1, -1] and int(n_dead) == 3
    assert idx[3] == 5 and 0 <= idx[4] <= 2
    # a proposal term: the weights are log_p - log_q
    a = sir_select(lw[3:] + 1.5, torch.full((3, 9), 1.5), torch.zeros(3, 9, 1), u[3:])
    assert torch.equal(a[1], idx[3:])


class Shifted:
    """Stand-in proposal: an isotropic normal with `.sample` / `.log_prob` and no progress-bar argument."""

    def __init__(self, loc, scale):
        self.d = MultivariateNormal(loc, scale**2 * torch.eye(loc.numel()))

    def sample(self, shape=torch.Size()):
        return self.d.sample(shape)

    def log_prob(self, theta):
        return self.d.log_prob(theta)


class GaussianLikelihood:
    """Stand-in estimator q(x | theta) = N(theta, I) with the estimator interface the likelihood potential uses."""

    def eval(self):
        return self

    def to(self, device):
        return self

    def log_prob(self, x, condition):
        return torch.distributions.Normal(condition, 1.0).log_prob(x).sum(-1)


def make_posterior(method="sir"):
    prior = MultivariateNormal(torch.zeros(2), 4 * torch.eye(2))
    potential = LikelihoodBasedPotential(GaussianLikelihood(), prior, device="cpu")
    post = ImportanceSamplingPosterior(potential, Shifted(torch.zeros(2), 2.0), method=method)
    return post.set_default_x(torch.tensor([[0.5, -0.3]])), prior


@pytest.mark.parametrize("shape", [(), (7,), (2, 3)])
def test_sample_shapes(shape):
    post, _ = make_posterior()
    s = post.sample(shape)
    assert s.shape == (*shape, 2) and torch.isfinite(s).all()
    theta, lw = post.sample(shape, method="importance")
    assert theta.shape == (*shape, 2) and lw.shape == (torch.Size(shape).numel(),)


def test_importance_method_returns_samples_and_log_weights():
    post, _ = make_posterior("importance")
    theta, lw = post.sample((50,))
    want = post.potential_fn(theta) - post.proposal.log_prob(theta)
    assert torch.allclose(lw, want, atol=1e-6)
    with pytest.raises(NameError):
        post.sample((3,), method="psis")
    with pytest.raises(ValueError, match="set_default_x"):
        ImportanceSamplingPosterior(post.potential_fn, post.proposal).sample((2,))


def test_sir_posterior_is_close_to_the_analytic_one():
    """Prior N(0, 4 I), likelihood N(theta, I): posterior N(0.8 x, 0.8 I).  20 000 draws at 64 candidates: the mean's
    standard error is sqrt(0.8 / 20 000) = 0.0063; 0.05 also covers the O(1 / K) bias of SIR."""
    post, _ = make_posterior()
    s = post.sample((20_000,), oversampling_factor=64)
    assert torch.allclose(s.mean(0), 0.8 * torch.tensor([0.5, -0.3]), atol=0.05)
    assert torch.allclose(s.var(0), torch.full((2,), 0.8), atol=0.08)


def test_loop_refills_after_dead_rows():
    """Potential -inf on half the proposal's support; at one candidate per row about half the rows are all-dead."""
    calls = []

    def potential(theta):
        calls.append(theta.shape[0])
        return torch.where(theta[:, 0] > 0, torch.zeros(theta.shape[0]), torch.full((theta.shape[0],), -float("inf")))

    proposal = Shifted(torch.zeros(2), 3.0)
    s = sampling_importance_resampling(potential, proposal, num_samples=500, num_candidate_samples=1,
                                       max_sampling_batch_size=200)
    assert s.shape == (500, 2) and (s[:, 0] > 0).all()
    assert len(calls) > 3 and max(calls) <= 200
    s = sampling_importance_resampling(potential, proposal, num_samples=300, num_candidate_samples=4)
    assert s.shape == (300, 2) and (s[:, 0] > 0).all()


def test_normalization_constant_and_log_prob():
    proposal = Shifted(torch.zeros(2), 1.5)

    class Pot:
        device = "cpu"
        n_calls = 0

        def set_x(self, x, x_is_iid=True):
            self.x = x

        def __call__(self, theta, track_gradients=True):
            Pot.n_calls += 1
            return proposal.log_prob(theta) + math.log(3.0) + 0.0 * self.x.sum()

    post = ImportanceSamplingPosterior(Pot(), proposal).set_default_x(torch.zeros(1, 2))
    z = post.estimate_normalization_constant(post.default_x, num_samples=2000)
    assert abs(float(z) - 3.0) <= 1e-4 * 3.0
    n = Pot.n_calls
    assert post.estimate_normalization_constant(post.default_x) is not None and Pot.n_calls == n       # cached
    post.estimate_normalization_constant(torch.zeros(1, 2))                     # equal to the default x: cached too
    assert Pot.n_calls == n
    post.estimate_normalization_constant(torch.ones(1, 2), num_samples=100)     # another x: computed, not kept
    assert Pot.n_calls == n + 1
    post.estimate_normalization_constant(post.default_x)
    assert Pot.n_calls == n + 1
    post.estimate_normalization_constant(post.default_x, num_samples=100, force_update=True)
    assert Pot.n_calls == n + 2
    theta = proposal.sample((20,))
    lp = post.log_prob(theta, normalization_constant_params=dict(num_samples=500))
    assert torch.allclose(lp, post.potential(theta) - math.log(3.0), atol=1e-4)
    assert torch.allclose(lp, proposal.log_prob(theta), atol=1e-4)      # normalised: the proposal's own density


def test_sample_batched_and_sbc():
    post, prior = make_posterior()
    xs = torch.randn(5, 2)
    s = post.sample_batched((4, 3), xs)
    assert s.shape == (4, 3, 5, 2) and torch.isfinite(s).all()
    # each observation gets its own posterior: N(0.8 x_b, 0.8 I); 2000 draws: standard error 0.02
    s = post.sample_batched((2000,), xs, max_sampling_batch_size=3000, oversampling_factor=64)
    assert torch.allclose(s.mean(0), 0.8 * xs, atol=0.15)
    bare = ImportanceSamplingPosterior(lambda theta: -theta.pow(2).sum(-1), Shifted(torch.zeros(2), 1.0))
    with pytest.raises(NotImplementedError):
        bare.sample_batched((3,), xs)
    thetas = prior.sample((6,))
    x6 = thetas + torch.randn(6, 2)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="Batched sampling not implemented")      # no fall-back loop
        ranks, dap = run_sbc(thetas, x6, post, num_posterior_samples=50, show_progress_bar=False)
    assert ranks.shape == (6, 2) and dap.shape == (6, 2)


def test_density_thresholder():
    dist = MultivariateNormal(torch.zeros(3), torch.eye(3))
    n, q = 5000, 0.01
    torch.manual_seed(11)
    thresholder = get_density_thresholder(dist, q, n)
    torch.manual_seed(11)
    want = torch.sort(dist.log_prob(dist.sample((n,)))).values[int(q * n)]
    assert float(thresholder.log_prob_threshold) == float(want)
    theta = torch.tensor([[0.0, 0.0, 0.0], [9.0, 9.0, 9.0]])
    got = thresholder(theta)
    assert got.dtype == torch.bool and got.tolist() == [True, False]
    draws = dist.sample((2000,))
    assert torch.equal(thresholder(draws), dist.log_prob(draws) > want)


def test_restricted_prior(capsys):
    prior = BoxUniform(-torch.ones(2), torch.ones(2))

    def accept(theta):
        return theta[..., 0] > 0.5            # a quarter of the box

    rp = RestrictedPrior(prior, accept)
    assert rp._prior is prior and rp.acceptance_rate is None
    s = rp.sample((700,), save_acceptance_rate=True)
    assert "rejected" in capsys.readouterr().out
    assert s.shape == (700, 2) and accept(s).all() and (s.abs() <= 1).all()
    assert 0.15 < float(rp.acceptance_rate) < 0.35
    assert rp.sample((2, 3), print_rejected_frac=False).shape == (2, 3, 2)
    theta = torch.tensor([[0.7, 0.0], [0.2, 0.0]])
    lp = rp.log_prob(theta)
    assert lp[1] == -float("inf")
    assert torch.allclose(lp[0], prior.log_prob(theta[:1])[0] - torch.log(rp.acceptance_rate))
    assert torch.equal(rp.log_prob(theta, norm_restricted_prior=False)[:1], prior.log_prob(theta[:1]))
    assert rp.support is prior.support or type(rp.support) is type(prior.support)
    with pytest.raises(NotImplementedError):
        rp.mean
    with pytest.raises(NotImplementedError):
        rp.variance
    with pytest.raises(ValueError, match="rejection \\| sir"):
        rp.sample((3,), sample_with="mcmc")
    with pytest.raises(AssertionError, match="you must provide a `posterior`"):
        rp.sample((3,), sample_with="sir")
    # the sir route: the posterior is the proposal, and `oversampling_factor` reaches the SIR loop
    seen = []

    class Post(Shifted):
        def sample(self, shape=torch.Size()):
            seen.append(torch.Size(shape).numel())
            return super().sample(shape)

    rp_sir = RestrictedPrior(prior, accept, posterior=Post(torch.tensor([0.6, 0.0]), 0.3), sample_with="sir")
    s = rp_sir.sample((40,), oversampling_factor=16)
    assert s.shape == (40, 2) and seen[0] == 40 * 16 and torch.isfinite(s).all()
    # (the "potential" is the accept function cast to float -- 1 inside, 0 outside, as LOG-weights, exactly as in the
    #  reference: points outside are e times less likely, not excluded, so nothing about acceptance is asserted)


def test_the_string_route_stays_refused():
    """`build_posterior(sample_with="importance")` keeps raising on all four trainers: the entry point is the class on
    top of the `*_estimator_based_potential` functions."""
    import sbi_amd.inference as inf
    from sbi_amd.neural_nets import NSFConfig, classifier_nn
    from sbi_amd.neural_nets.net_builders.estimator_configs import MixedConfig

    prior = BoxUniform(-torch.ones(2), torch.ones(2))
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        inf.NPE(prior).build_posterior(sample_with="importance")
    with pytest.raises(NotImplementedError, match="outside the accelerated path"):
        inf.NLE(prior, density_estimator=NSFConfig(hidden_features=8, num_transforms=1)).build_posterior(
            sample_with="importance")
    with pytest.raises(NotImplementedError, match="'mcmc' or 'rejection'"):
        inf.MNLE(density_estimator=MixedConfig()).build_posterior(sample_with="importance")
    with pytest.raises(NotImplementedError, match="mcmc"):
        inf.NRE_B(show_progress_bars=False).build_posterior(
            sample_with="importance", prior=prior,
            density_estimator=classifier_nn("resnet")(torch.randn(20, 2), torch.randn(20, 2)))


def test_a_restricted_prior_proposal_stays_in_round_zero():
    """TSNPE needs no proposal correction: the trainer files data drawn from a `RestrictedPrior` over ITS prior under
    round 0 (the first-round loss); a restricted version of another prior opens round 1."""
    import sbi_amd.inference as inf

    prior = BoxUniform(-torch.ones(2), torch.ones(2))
    theta = prior.sample((20,))
    x = theta + 0.1 * torch.randn(20, 2)
    trainer = inf.NPE(prior, show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trainer.append_simulations(theta, x)
        trainer.append_simulations(theta, x, proposal=RestrictedPrior(prior, lambda t: t[..., 0] > 0))
        assert trainer._data_round_index == [0, 0]
        trainer.append_simulations(theta, x, proposal=RestrictedPrior(BoxUniform(-torch.ones(2), torch.ones(2)),
                                                                      lambda t: t[..., 0] > 0))
    assert trainer._data_round_index == [0, 0, 1]


def test_live_rows_are_gathered_from_a_known_count():
    from sbi_amd.samplers.importance.sir import live_first

    idx = torch.tensor([3, -1, 0, -1, -1, 7, 2], dtype=torch.int32)
    live, dead = live_first(idx, 3)
    assert live.tolist() == [0, 2, 5, 6] and dead.tolist() == [1, 3, 4]
    live, dead = live_first(idx.clamp(min=0), 0)
    assert live.tolist() == list(range(7)) and dead.numel() == 0
