"""VIPosterior on the host: the Gaussian family against torch's distributions, the link descriptors, the eager route
of the four divergences on an analytic target, the PSIS generalised-Pareto fit, the loss statistics against a literal
loop, the hyper-parameter checks, the refusals, pickling and multi-round copies."""
import copy
import math
import pickle

import numpy as np
import pytest
import torch
from torch.distributions import (Dirichlet, Exponential, Independent, MultivariateNormal, Normal,
                                 TransformedDistribution)

from sbi_amd.inference import VIPosterior
from sbi_amd.inference.posteriors import VIPosterior as VIPosteriorFromPosteriors
from sbi_amd.samplers.importance.importance_sampling import exponentiate_weights, gpdfit, largest_weight_indices
from sbi_amd.samplers.vi import (ElboOptimizer, ForwardKLOptimizer, IWElboOptimizer, LearnableGaussian,
                                 RenyiDivergenceOptimizer, get_default_VI_method, get_quality_metric, get_VI_method,
                                 link_descriptor)
from sbi_amd.utils import BoxUniform
from sbi_amd.utils.sbiutils import mcmc_transform
from tests import vi_oracle as O

M_TRUE = torch.tensor([0.5, -1.0, 1.5])
A_TRUE = torch.tensor([[0.5, 0.0, 0.0], [0.3, 0.4, 0.0], [-0.2, 0.1, 0.3]])


class AnalyticPotential:
    """log N(theta; m, A A^T) + log prior(theta): the small potential object the posterior classes take."""

    def __init__(self, prior, device="cpu"):
        self.prior, self.device, self.x_o = prior, device, None
        self.m, self.A = M_TRUE.to(device), A_TRUE.to(device)

    def set_x(self, x_o, x_is_iid=True):
        self.x_o = x_o

    def to(self, device):
        self.device = device
        self.m, self.A = self.m.to(device), self.A.to(device)
        self.prior = self.prior.to(device)
        return self

    def __call__(self, theta, track_gradients=True):
        with torch.set_grad_enabled(track_gradients):
            return MultivariateNormal(self.m, scale_tril=self.A).log_prob(theta) + self.prior.log_prob(theta)


def box(d=3, bound=4.0):
    return BoxUniform(-bound * torch.ones(d), bound * torch.ones(d))


def make_posterior(method="rKL", q="gaussian", **kw):
    prior = box()
    return VIPosterior(AnalyticPotential(prior), prior, q=q, vi_method=method, **kw).set_default_x(torch.zeros(1, 2))


# ---- the family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [True, False])
def test_learnable_gaussian_matches_torch_distributions(full):
    D = 4
    link = mcmc_transform(box(D)).inv
    q = LearnableGaussian(D, full_covariance=full, link_transform=link)
    with torch.no_grad():
        q.loc.copy_(torch.randn(D) * 0.3)
        if full:
            q.scale_tril.copy_(torch.eye(D) * 0.7 + 0.2 * torch.randn(D, D))       # the upper triangle is NOT zero
            base = MultivariateNormal(q.loc, scale_tril=q.scale_tril.tril())
        else:
            q.log_scale.copy_(torch.randn(D) * 0.3)
            base = Independent(Normal(q.loc, q.log_scale.exp()), 1)
    ref = TransformedDistribution(base, [link])
    assert sorted(q.state_dict()) == (["loc", "scale_tril"] if full else ["loc", "log_scale"])
    theta = ref.sample((64,))
    assert torch.allclose(q.log_prob(theta), ref.log_prob(theta), atol=1e-4)
    torch.manual_seed(3)
    th, lq = q.sample_and_log_prob((32,))
    assert th.shape == (32, D) and lq.shape == (32,) and th.requires_grad
    assert torch.allclose(lq, ref.log_prob(th.detach()), atol=1e-4)
    assert q.sample((5, 2)).shape == (5, 2, D)
    if full:
        (-(lq.sum() + th.sum())).backward()
        upper = torch.triu(torch.ones(D, D), diagonal=1).bool()
        assert bool((q.scale_tril.grad[upper] == 0).all()) and bool((q.scale_tril.grad[~upper] != 0).any())
        before = q.log_prob(theta)
        with torch.no_grad():
            q.scale_tril[upper] += 5.0
        assert torch.equal(q.log_prob(theta), before)


def test_link_descriptors():
    t, why = link_descriptor(mcmc_transform(BoxUniform(torch.tensor([-1.0, 0.0]), torch.tensor([2.0, 5.0]))).inv, 2)
    assert why == "" and t.shape == (4, 2)
    assert t[0].tolist() == [1.0, 1.0] and t[1].tolist() == [-1.0, 0.0] and t[2].tolist() == [3.0, 5.0]
    assert t[3].tolist() == [2.0, 5.0]
    mvn = MultivariateNormal(torch.tensor([1.0, -2.0]), covariance_matrix=torch.tensor([[4.0, 0.0], [0.0, 0.25]]))
    t, why = link_descriptor(mcmc_transform(mvn).inv, 2)
    assert why == "" and t[0].tolist() == [0.0, 0.0] and t[1].tolist() == [1.0, -2.0]
    assert torch.allclose(t[2], torch.tensor([2.0, 0.5]))
    ind = Independent(Normal(torch.zeros(3), 2 * torch.ones(3)), 1)
    t, why = link_descriptor(mcmc_transform(ind).inv, 3)
    assert why == "" and t[0].tolist() == [0.0] * 3 and t[2].tolist() == [2.0] * 3
    half = Independent(Exponential(torch.ones(2)), 1)          # support: greater_than_eq(0)
    t, why = link_descriptor(mcmc_transform(half).inv, 2)
    assert why == "" and t[0].tolist() == [2.0, 2.0] and t[1].tolist() == [0.0, 0.0]
    t, why = link_descriptor(None, 2)
    assert why == "" and t[0].tolist() == [0.0, 0.0] and t[2].tolist() == [1.0, 1.0]
    t, why = link_descriptor(torch.distributions.biject_to(Dirichlet(torch.ones(3)).support), 3)
    assert t is None and "does not decompose per dimension" in why


# ---- the eager route on an analytic target ------------------------------------------------------------------------
@pytest.mark.parametrize("method,kw", [("rKL", {}), ("fKL", {}), ("IW", {"K": 8}), ("alpha", {"alpha": 0.5})])
def test_eager_route_recovers_the_analytic_posterior(method, kw):
    torch.manual_seed(0)
    post = make_posterior(method)
    ok, why = post.kernel_route()
    assert not ok and "cpu" in why
    post.train(max_num_iters=800, n_particles=256, learning_rate=1e-2, quality_control=False, show_progress_bar=False,
               check_for_convergence=False, **kw)
    s = post.sample((2000,))
    mean_err = (s.mean(0) - M_TRUE).abs().max().item()
    cov_err = (torch.cov(s.T) - A_TRUE @ A_TRUE.T).abs().max().item()
    print(f"{method}: max-abs mean error {mean_err:.4f}, covariance error {cov_err:.4f}")
    assert mean_err <= 0.1 and cov_err <= 0.1
    lp = post.log_prob(s[:50])
    assert lp.shape == (50,) and torch.isfinite(lp).all()


# ---- PSIS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0.1, 0.5, 0.9])
def test_gpdfit_recovers_the_shape(k):
    from scipy.stats import genpareto

    x = torch.from_numpy(genpareto.rvs(k, size=20_000, random_state=np.random.default_rng(7)))
    k_hat, sigma = gpdfit(x, sorted=False)
    print(f"k = {k}: k_hat = {float(k_hat):.4f}, sigma = {float(sigma):.4f}")
    assert abs(float(k_hat) - k) <= 0.1
    kq, sq, ks, w = gpdfit(x.sort().values, return_quadrature=True)
    assert float(kq) == float(k_hat) and ks.shape == w.shape and abs(float(w.sum()) - 1) < 1e-9


def test_weight_helpers():
    lw = torch.tensor([0.0, -float("inf"), 2.0, float("nan"), 1.0])
    w = exponentiate_weights(lw)
    assert torch.allclose(w, torch.tensor([math.exp(-2.0), 1.0, math.exp(-1.0)]))
    weights = torch.rand(1000)
    idx = largest_weight_indices(weights)
    assert len(idx) == int(min(1000 / 5, 3 * math.sqrt(1000)))
    assert torch.equal(weights[idx], weights.sort().values[-len(idx):])
    fn, msg = get_quality_metric("psis")
    assert callable(fn) and "Smaller than 0.5" in msg
    assert callable(get_quality_metric("prop")[0]) and callable(get_quality_metric("prop_prior")[0])


# ---- the loss statistics ------------------------------------------------------------------------------------------
def test_loss_statistics_follow_the_written_recurrences():
    prior = box()
    opt = ElboOptimizer(AnalyticPotential(prior), LearnableGaussian(3), prior=prior, lr=1e-3, gamma=0.999)
    g = torch.Generator().manual_seed(5)
    rec = 3.0 * torch.exp(-torch.arange(2100) / 300.0) + 0.05 * torch.randn(2100, generator=g)
    rec[37] = float("nan")
    window = 20
    losses, avg, std, slope = [], [], [], []
    flags = []
    for n, v in enumerate(rec.tolist()):
        if n == 0:
            losses.append(v), avg.append(v), std.append(1.0), slope.append(1.0)
        elif not math.isfinite(v):
            losses.append(1.0 if n < 2000 else 0.0), avg.append(avg[-1]), std.append(std[-1]), slope.append(slope[-1])
        else:
            back = max(n - window, 0)
            d = (np.float32(v) - np.float32(losses[back])) / window
            losses.append(v)
            std.append(abs(np.float32(std[-1]) + d - np.float32(std[-1]) / (window - 1)))
            slope.append((np.float32(v) - np.float32(avg[back])) / window)
            avg.append(np.float32(avg[-1]) + d)
        opt.update_loss_stats(torch.tensor(v))
        flags.append(opt.converged())
        if n + 1 >= 50:
            assert flags[-1] == (abs(float(np.mean(np.float32(slope[n + 1 - 50: n + 1])))) < opt.eps)
        else:
            assert flags[-1] is False
    assert opt.num_step == 2100 and len(opt.losses) == 4000                       # grown past 2 000 once
    for mine, ref in ((opt.moving_average, avg), (opt.moving_std, std), (opt.moving_slope, slope)):
        assert torch.allclose(mine[:2100], torch.tensor(np.float32(ref)), rtol=1e-4, atol=1e-5)
    m, s = opt.get_loss_stats()
    assert float(m) == float(opt.moving_average[2099]) and float(s) == float(opt.moving_std[2099])
    opt.reset_loss_stats()
    assert opt.num_step == 0 and len(opt.losses) == 2000


# ---- the public surface -------------------------------------------------------------------------------------------
def test_registry_and_defaults():
    assert get_default_VI_method() == ["rKL", "IW", "fKL", "alpha"]
    assert get_VI_method("rKL") is ElboOptimizer and get_VI_method("IW") is IWElboOptimizer
    assert get_VI_method("fKL") is ForwardKLOptimizer and get_VI_method("alpha") is RenyiDivergenceOptimizer
    assert VIPosteriorFromPosteriors is VIPosterior
    post = make_posterior()
    assert post.vi_method == "rKL" and isinstance(post.q, LearnableGaussian)
    post.vi_method = "alpha"
    assert post._optimizer_builder is RenyiDivergenceOptimizer
    post.q = "gaussian_diag"
    assert sorted(post.q.state_dict()) == ["loc", "log_scale"]


@pytest.mark.parametrize("kw,msg", [
    ({"n_particles": 0}, "n_particles must be positive"), ({"learning_rate": 0.0}, "learning_rate must be positive"),
    ({"gamma": 1.5}, r"gamma must be in \(0, 1\]"), ({"gamma": 0.0}, r"gamma must be in \(0, 1\]"),
    ({"max_num_iters": 0}, "max_num_iters must be positive"), ({"min_num_iters": -1}, "min_num_iters must be non-negative"),
    ({"clip_value": 0.0}, "clip_value must be positive")])
def test_train_validates_its_hyper_parameters(kw, msg):
    with pytest.raises(ValueError, match=msg):
        make_posterior().train(**kw)


def test_refusals_and_errors():
    prior = box()
    pot = AnalyticPotential(prior)
    for flow in ("maf", "nsf", "naf", "unaf", "nice", "sospf", "gf"):
        with pytest.raises(NotImplementedError, match="q='gaussian'"):
            VIPosterior(pot, prior, q=flow)
    with pytest.raises(NotImplementedError, match="q='gaussian'"):
        VIPosterior(pot, prior)                                  # the reference's default family is a flow
    with pytest.raises(ValueError, match="Unknown variational family 'cauchy'"):
        VIPosterior(pot, prior, q="cauchy")
    post = make_posterior()
    with pytest.raises(NotImplementedError, match="train_amortized"):
        post.train_amortized(torch.zeros(4, 3), torch.zeros(4, 2))
    with pytest.raises(NotImplementedError, match="Batched sampling is not implemented for single-x VI mode"):
        post.sample_batched((2,), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="was not fit on the specified observation"):
        post.log_prob(torch.zeros(1, 3))
    with pytest.raises(ValueError, match="was not fit on the specified observation"):
        post.sample((2,))
    post.train(max_num_iters=5, quality_control=False, show_progress_bar=False, warm_up_rounds=2)
    assert torch.isfinite(post.log_prob(torch.zeros(1, 3))).all()
    with pytest.raises(ValueError, match="was not fit on the specified observation"):
        post.log_prob(torch.zeros(1, 3), x=torch.ones(1, 2))
    with pytest.raises(ValueError, match="could not find a suitable prior"):
        VIPosterior(lambda theta, track_gradients=True: theta.sum(-1), q="gaussian")


def test_pickle_retrain_and_copies():
    torch.manual_seed(2)
    post = make_posterior("rKL")
    post.train(max_num_iters=30, n_particles=64, learning_rate=1e-2, quality_control=False, show_progress_bar=False)
    assert post._optimizer is not None
    clone = pickle.loads(pickle.dumps(post))
    assert clone._optimizer is None and post._optimizer is not None          # saving leaves the original untouched
    theta = post.sample((8,))
    assert torch.equal(clone.log_prob(theta), post.log_prob(theta))
    assert copy.deepcopy(post)._optimizer is None
    clone.train(max_num_iters=5, quality_control=False, show_progress_bar=False)     # builds a new optimiser

    second = VIPosterior(AnalyticPotential(box()), q=post)                   # multi-round: arguments copied from q
    assert second.vi_method == "rKL" and second.q is not post.q
    assert torch.equal(second.q.loc, post.q.loc) and torch.equal(second.log_prob(theta), post.log_prob(theta))
    with torch.no_grad():
        second.q.loc += 1.0
    assert not torch.equal(second.q.loc, post.q.loc)

    loc_before = post.q.loc.detach().clone()
    post.train(max_num_iters=1, learning_rate=1e-8, retrain_from_scratch=True, quality_control=False,
               show_progress_bar=False, warm_up_rounds=0)
    assert not torch.allclose(post.q.loc, loc_before) and post.q.loc.abs().max() < 1e-3      # a fresh q (loc = 0)
    inst = VIPosterior(AnalyticPotential(box()), box(), q=LearnableGaussian(3, link_transform=mcmc_transform(box()).inv))
    inst.set_default_x(torch.zeros(1, 2))
    with pytest.raises(ValueError, match="Cannot rebuild `q`"):
        inst.train(max_num_iters=1, retrain_from_scratch=True, quality_control=False, show_progress_bar=False)


def test_user_distribution_and_builder_run_eager():
    prior = box()
    loc = torch.zeros(3, requires_grad=True)
    log_scale = torch.zeros(3, requires_grad=True)

    class UserQ(Independent):
        def __init__(self):
            super().__init__(Normal(loc, log_scale.exp(), validate_args=False), 1, validate_args=False)

        def rsample(self, shape=torch.Size()):
            return loc + log_scale.exp() * torch.randn(*shape, 3)

        def log_prob(self, value):
            return Independent(Normal(loc, log_scale.exp(), validate_args=False), 1).log_prob(value)

    post = VIPosterior(AnalyticPotential(prior), prior, q=UserQ(), parameters=[loc, log_scale])
    post.set_default_x(torch.zeros(1, 2))
    ok, why = post.kernel_route()
    assert not ok and "Gaussian families only" in why
    post.train(max_num_iters=20, n_particles=32, quality_control=False, show_progress_bar=False, warm_up_rounds=5)
    s = post.sample((10,))
    assert s.shape == (10, 3) and bool(prior.support.check(s).all())
    built = VIPosterior(AnalyticPotential(prior), prior, q=_diag_builder).set_default_x(torch.zeros(1, 2))
    assert isinstance(built.q, LearnableGaussian) and built._q_recipe.kind == "callable"


def _diag_builder(event_shape, link_transform, device="cpu"):
    return LearnableGaussian(event_shape[0], full_covariance=False, link_transform=link_transform, device=device)


# ---- the oracle against the package's own eager losses ------------------------------------------------------------
@pytest.mark.parametrize("method,kw", [("rKL", {}), ("rKL", {"stick_the_landing": True}), ("IW", {"K": 4}),
                                       ("IW", {"K": 4, "dreg": True}), ("alpha", {"alpha": 0.5}),
                                       ("alpha", {"alpha": 2.0, "unbiased": True}), ("fKL", {})])
def test_oracle_agrees_with_the_eager_optimisers(method, kw):
    """tests/vi_oracle.py and the eager optimisers are two independent writings of the same losses: on the same eps
    their gradients agree to fp32 rounding."""
    D, n = 3, 24
    prior = box(D)
    pot = AnalyticPotential(prior)
    link = mcmc_transform(prior).inv
    q = LearnableGaussian(D, link_transform=link)
    with torch.no_grad():
        q.loc.copy_(torch.tensor([0.2, -0.1, 0.3]))
        q.scale_tril.copy_(torch.eye(D) * 0.6 + 0.1 * torch.randn(D, D).tril(-1))
    particles = n // kw.get("K", 1)
    opt = get_VI_method(method)(pot, q, prior=prior, n_particles=particles, lr=1e-3, gamma=0.999, **kw)
    eps = torch.randn(n, D)
    import torch.distributions.multivariate_normal as mvn_module

    real = mvn_module._standard_normal
    mvn_module._standard_normal = lambda shape, dtype, device: eps.to(dtype)      # rsample / sample draw THESE eps
    try:
        surrogate, _ = opt._loss(torch.zeros(1, 2))
    finally:
        mvn_module._standard_normal = real
    grads = torch.autograd.grad(surrogate, [q.loc, q.scale_tril])
    mine = torch.cat([grads[0], grads[1].reshape(-1)])

    phi = q.flat_parameters()
    table, _ = link_descriptor(link, D)
    _, theta, _ = O.forward(phi.double(), table, eps.double(), D, True)
    th = theta.float().requires_grad_(True)
    p = pot(th, track_gradients=True)
    (r,) = torch.autograd.grad(p.sum(), th)
    g, _ = O.gradient(method, phi, table, eps, p.detach(), None if method == "fKL" else r, D, True, **kw)
    assert torch.allclose(mine.double(), g, rtol=2e-3, atol=2e-4), (mine.double() - g).abs().max()
