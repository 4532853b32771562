"""VIPosterior end to end on the device: the analytic target on the kernel route (all four divergences), the routing
answers, and the kernel route over a trained NLE and NRE potential -- its gradient against the eager route's autograd
gradient on the same eps, then a short training with quality control, `log_prob`, `evaluate` and `map`.  The nets are
tiny and train for three epochs: nothing here asserts the quality of THEIR fit."""
import functools
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd.inference import NLE, NRE_B, VIPosterior
from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential
from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential
from sbi_amd.neural_nets import NSFConfig, classifier_nn
from sbi_amd.samplers.vi import LearnableGaussian
from sbi_amd.simulators.linear_gaussian import linear_gaussian
from sbi_amd.utils import BoxUniform
from sbi_amd.utils.metrics import c2st
from sbi_amd.utils.parity import row_parity
from sbi_amd.utils.sbiutils import within_support
from tests.test_vi_cpu import A_TRUE, M_TRUE, AnalyticPotential

pytestmark = pytest.mark.gpu

DIM = 2


def analytic_posterior(method, d=3, **kw):
    prior = BoxUniform(-4.0 * torch.ones(d), 4.0 * torch.ones(d), device="cuda")
    post = VIPosterior(AnalyticPotential(prior, device="cuda"), prior, q="gaussian", vi_method=method, device="cuda", **kw)
    return post.set_default_x(torch.zeros(1, 2))


@pytest.mark.parametrize("method,kw", [("rKL", {}), ("fKL", {}), ("IW", {"K": 8}), ("alpha", {"alpha": 0.5})])
def test_kernel_route_recovers_the_analytic_posterior(method, kw):
    torch.manual_seed(0)
    post = analytic_posterior(method)
    assert post.kernel_route() == (True, "")
    post.train(max_num_iters=800, n_particles=256, learning_rate=1e-2, quality_control=False, show_progress_bar=False,
               check_for_convergence=False, **kw)
    assert post.kernel_route() == (True, "") and post._optimizer._kstate is not None
    assert int(post._optimizer._kstate.status[0]) == 0                     # the guard never fired
    assert post._optimizer.num_step == 800 and torch.isfinite(post._optimizer.losses[:800]).all()
    s = post.sample((2000,))
    assert s.is_cuda and s.shape == (2000, 3)
    mean_err = (s.mean(0).cpu() - M_TRUE).abs().max().item()
    cov_err = (torch.cov(s.T).cpu() - A_TRUE @ A_TRUE.T).abs().max().item()
    print(f"{method}: max-abs mean error {mean_err:.4f}, covariance error {cov_err:.4f}")
    assert mean_err <= 0.1 and cov_err <= 0.1
    if method == "rKL":
        exact = MultivariateNormal(M_TRUE, scale_tril=A_TRUE).sample((2000,))
        score = float(c2st(s.cpu(), exact))
        print(f"c2st against exact draws: {score:.3f}")
        assert score <= 0.55
    lp = post.log_prob(s[:100])
    ref = MultivariateNormal(post.q.loc.detach(), scale_tril=post.q.scale_tril.detach().tril())
    z = post.link_transform.inv(s[:100])
    want = ref.log_prob(z) + post.link_transform.inv.log_abs_det_jacobian(s[:100], z)
    assert torch.allclose(lp, want, atol=1e-3)                              # the kernel's log q IS q's normalised density


def test_routing_answers():
    post = analytic_posterior("rKL")
    assert post.kernel_route() == (True, "")
    post.force_eager = True
    assert post.kernel_route() == (False, "force_eager is set")
    post.train(max_num_iters=3, quality_control=False, show_progress_bar=False, warm_up_rounds=2)
    assert post._optimizer._kstate is None and post.sample((4,)).shape == (4, 3)
    post.force_eager = False
    ok, why = analytic_posterior("rKL", d=17).kernel_route()
    assert not ok and "17" in why
    fkl = analytic_posterior("fKL")
    fkl.train(max_num_iters=2, n_particles=16, quality_control=False, show_progress_bar=False, warm_up_rounds=1,
              weight_transform=lambda w: w.clamp(max=10.0))
    assert fkl.kernel_route() == (False, "a custom weight_transform") and fkl._optimizer._kstate is None
    sgd = analytic_posterior("rKL")
    sgd.train(max_num_iters=2, n_particles=16, quality_control=False, show_progress_bar=False, warm_up_rounds=1,
              optimizer=torch.optim.SGD)
    assert not sgd.kernel_route()[0] and "Adam" in sgd.kernel_route()[1]
    diag = analytic_posterior("rKL")
    diag.q = "gaussian_diag"
    assert diag.kernel_route() == (True, "")


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
    return potential_fn, transform, prior


@pytest.mark.parametrize("kind", ["nle", "nre"])
def test_kernel_route_over_a_trained_potential(kind):
    import torch.distributions.multivariate_normal as mvn_module

    potential_fn, transform, prior = trained(kind)
    torch.manual_seed(6)
    post = VIPosterior(potential_fn, prior, q="gaussian", theta_transform=transform, device="cuda")
    x_o = torch.zeros(1, DIM, device="cuda")
    post.set_default_x(x_o)
    assert post.kernel_route() == (True, "")
    with torch.no_grad():
        post.q.loc.copy_(torch.tensor([0.3, -0.2]))
        post.q.scale_tril.copy_(torch.tensor([[0.6, 0.0], [0.2, 0.5]]))
    phi0 = post.q.flat_parameters().clone()
    opt = post._new_optimizer(1e-3, 10.0, 0.999, 256, {})
    theta, eps, grad = opt.kernel_gradient_probe(x_o)
    assert theta.shape == (256, DIM) and bool(within_support(prior, theta).all())

    twin = LearnableGaussian(DIM, link_transform=post.link_transform, device="cuda")
    twin.load_flat_parameters(phi0)
    eager = post._optimizer_builder(potential_fn, twin, lr=1e-3, gamma=0.999, n_particles=256, prior=prior)
    eager.force_eager = True
    real = mvn_module._standard_normal
    mvn_module._standard_normal = lambda shape, dtype, device: eps.to(dtype)      # the same eps
    try:
        surrogate, _ = eager._loss(x_o)
    finally:
        mvn_module._standard_normal = real
    g_loc, g_tril = torch.autograd.grad(surrogate, [twin.loc, twin.scale_tril])
    want = torch.cat([g_loc, g_tril.reshape(-1)])
    rp = row_parity(grad.cpu(), want.cpu())
    print(f"{kind}: kernel-route gradient vs eager autograd: worst {rp['worst_scaled']:.3f} x bound")
    assert rp["worst_scaled"] <= 1.0, rp

    post.train(max_num_iters=50, n_particles=128, learning_rate=1e-2, quality_control=True, show_progress_bar=False)
    assert post._optimizer.kernel_route()[0] and post._optimizer.num_step >= 25
    s = post.sample((500,))
    assert s.is_cuda and torch.isfinite(s).all() and bool(within_support(prior, s).all())
    assert torch.isfinite(post.log_prob(s)).all()
    assert isinstance(post.evaluate("psis", N=5000), float)
    best = post.map(num_iter=20, num_init_samples=200, num_to_optimize=10)
    assert best.shape == (1, DIM) and bool(within_support(prior, best).all())
