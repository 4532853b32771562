"""Batched MCMC (MCMCPosterior.sample_batched): the generic, fused two-launch and persistent tick routes, the persistent
one-lane-per-chain kernel on the ratio classifier (sbi_amd_nre_mcmc_slice_run), and SBC / TARP end to end on the device."""

import time
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd import _lib
from sbi_amd.diagnostics import check_sbc, check_tarp, run_sbc, run_tarp
from sbi_amd.diagnostics.sbc import check_uniformity_frequentist
from sbi_amd.inference import NPE, NRE_B
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior, unconstrained_potential
from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential
from sbi_amd.inference.potentials.posterior_based_potential import posterior_estimator_based_potential
from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential
from sbi_amd.neural_nets import NSFConfig, classifier_nn
from sbi_amd.samplers.mcmc import SliceSamplerVectorized
from sbi_amd.simulators.linear_gaussian import linear_gaussian
from sbi_amd.utils.metrics import c2st
from sbi_amd.utils.sbiutils import mcmc_transform, within_support
from sbi_amd.utils.torchutils import BoxUniform
from tests.helpers import matched_pair

pytestmark = pytest.mark.gpu


class GaussianPotential:
    """log N(theta; x_c, sigma^2): one observation per theta row when `x_is_iid=False` (torch only: the generic route)."""

    def __init__(self, sigma):
        self.sigma, self.device = sigma, "cuda"

    def set_x(self, x_o, x_is_iid=True):
        self.x_o, self.x_is_iid = x_o.to("cuda"), x_is_iid

    def __call__(self, theta, track_gradients=True):
        assert theta.shape[0] == self.x_o.shape[0]
        return -0.5 * (((theta - self.x_o) / self.sigma) ** 2).sum(-1)


def test_generic_route_orders_and_distributes_the_draws_per_observation():
    """B = 30 observations x K = 200 chains, thin 1, the LAST sample of every chain: K independent draws of
    N(x_b, sigma^2) per observation, so every per-observation, per-dimension mean lies within 5 sigma / sqrt(K) of x_b."""
    torch.manual_seed(0)
    B, K, D, sigma = 30, 200, 2, 0.7
    prior = MultivariateNormal(torch.zeros(D, device="cuda"), 9.0 * torch.eye(D, device="cuda"))
    post = MCMCPosterior(GaussianPotential(sigma), prior, mcmc_transform(prior, device="cuda"), num_chains=K, thin=1,
                         warmup_steps=60, init_strategy="proposal", device="cuda")
    xs = 3.0 * torch.randn(B, D, device="cuda")
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # 6 000 chains: no warning about their number
        s = post.sample_batched((K,), xs, show_progress_bars=False)
    assert post.posterior_sampler.route == "generic"
    assert s.shape == (K, B, D) and torch.isfinite(s).all()
    err = (s.mean(0) - xs).abs().max().item()
    print(f"generic batched: max |mean - x_b| = {err:.4f} (bound {5 * sigma / K**0.5:.4f}), std {s.std(0).mean().item():.3f}")
    assert err < 5 * sigma / K**0.5
    assert s.reshape(5, 40, B, D).shape == post.sample_batched((5, 40), xs, show_progress_bars=False).shape


def _ratio_estimator(D=3, C=3, H=50, NB=2, std=0.3):
    torch.manual_seed(0)
    theta = torch.randn(500, D) * 1.5 + 0.3
    x = theta[:, :1].repeat(1, C) * 0.7 + torch.randn(500, C)
    est = classifier_nn("resnet", hidden_features=H, num_blocks=NB)(theta, x)
    with torch.no_grad():      # weights away from nflows' near-zero init of the last block layer
        est.net.flat_params.normal_(0.0, std)
    return est.to("cuda")


def _ratio_posterior(prior, **kw):
    est = _ratio_estimator(**kw)
    pot, tf = ratio_estimator_based_potential(est, prior, x_o=None)
    return MCMCPosterior(pot, prior, tf, device="cuda")


def _box(D=3):
    return BoxUniform(-2.0 * torch.ones(D), 2.0 * torch.ones(D), device="cuda")


@pytest.mark.parametrize("kind", ["npe-gaussian", "npe-box", "nle-gaussian", "nre-box", "nre-gaussian"])
def test_fused_batched_potential_equals_the_generic_one(kind):
    """What the fused two-launch route feeds the tick -- log q - log|det| -- equals potential_fn(theta) - log|det| of
    the generic route (tolerance of tests/test_nre_gpu.py's fused-against-generic check)."""
    torch.manual_seed(4)
    B, K = 5, 7
    family, prior_kind = kind.split("-")
    D = 3
    prior = _box(D) if prior_kind == "box" else MultivariateNormal(torch.zeros(D, device="cuda"),
                                                                    torch.eye(D, device="cuda"))
    if family == "npe":
        _, est, _, x = matched_pair(D=D, C=4)
        pot, _ = posterior_estimator_based_potential(est, prior, x_o=None)
        post = MCMCPosterior(pot, prior, mcmc_transform(prior, device="cuda"), device="cuda")
        xs = x[:B].cuda()
    elif family == "nle":
        _, est, flow_inputs, _ = matched_pair(D=4, C=D)          # the flow's input is x (4), its condition theta (3)
        pot, tf = likelihood_estimator_based_potential(est, prior, x_o=None)
        post = MCMCPosterior(pot, prior, tf, device="cuda")
        xs = flow_inputs[:B].cuda()
    else:
        post = _ratio_posterior(prior)
        xs = torch.randn(B, 3, device="cuda")
    post.potential_fn.set_x(xs.repeat_interleave(K, dim=0), x_is_iid=False)
    fused = post._fused_potential_batched(xs, K)
    assert fused is not None and fused.persistent_capable is False and len(fused.fused_spec) == 6
    assert (getattr(fused, "nre_persistent", None) is not None) == (family == "nre")
    u = torch.randn(B * K, D, device="cuda") * 1.5
    logp, lad = fused(u)
    generic = unconstrained_potential(post.potential_fn, post.theta_transform, "cuda")(u).reshape(-1)
    err = (logp - lad - generic).abs().max().item()
    print(f"{kind}: max |fused - generic| = {err:.2e}")
    assert torch.allclose(logp - lad, generic, atol=1e-4, rtol=1e-5)
    # every chain is held against its own observation: another observation gives another value
    other = post._fused_potential_batched(xs.flip(0), K)(u)
    assert not torch.allclose(other[0], logp, atol=1e-3)


def _run_sampler(fused, init, persistent, num_samples=12, tuning=10, poll_every=16, seed=11):
    torch.manual_seed(seed)
    s = SliceSamplerVectorized(fused, init.clone(), num_chains=init.shape[0], thin=1, tuning=tuning, poll_every=poll_every,
                               persistent=persistent)
    return s.run(num_samples).clone(), s


def _batched_spec(post, xs, K):
    post.potential_fn.set_x(xs.repeat_interleave(K, dim=0), x_is_iid=False)
    fused = post._fused_potential_batched(xs, K)
    assert fused is not None and fused.nre_persistent is not None
    return fused


def test_persistent_nre_sampler_equals_the_two_launch_loop():
    """sbi_amd_nre_mcmc_slice_run (a lane owns a chain for `poll_every` ticks) against the loop of log-ratio + tick
    launches: the same Philox counters and the same fma sequence -> the same chains, bit for bit.  7 x 30 = 210 chains
    leave a ragged last workgroup."""
    post = _ratio_posterior(_box())
    B, K = 7, 30
    torch.manual_seed(2)
    xs = torch.randn(B, 3, device="cuda")
    fused = _batched_spec(post, xs, K)
    init = torch.randn(B * K, 3, device="cuda") * 0.3
    (a, sa), (b, sb) = _run_sampler(fused, init, True), _run_sampler(fused, init, False)
    assert sa.route == "nre_persistent" and sb.route == "two_launch"
    assert sa.num_ticks >= sb.num_ticks and sa.num_ticks - sb.num_ticks < 16
    assert torch.equal(a, b) and torch.equal(sa.width, sb.width) and torch.equal(sa.x, sb.x)
    assert torch.isfinite(a).all() and a.std() > 0.05
    # the other workgroup sizes walk the same chains
    for wg in (128, 256):
        torch.manual_seed(11)
        s = SliceSamplerVectorized(fused, init.clone(), num_chains=B * K, thin=1, tuning=10, poll_every=16,
                                   persistent=True, nre_wg_size=wg)
        assert torch.equal(s.run(12), a)


def test_persistent_chains_depend_on_their_own_observation_only():
    post = _ratio_posterior(_box())
    K = 40
    torch.manual_seed(3)
    xs = torch.randn(3, 3, device="cuda")
    init = torch.randn(3 * K, 3, device="cuda") * 0.3
    a, sa = _run_sampler(_batched_spec(post, xs, K), init, True)
    b, sb = _run_sampler(_batched_spec(post, xs[1:2].expand(3, 3).contiguous(), K), init, True)
    assert sa.route == sb.route == "nre_persistent"
    assert torch.equal(a[K : 2 * K], b[K : 2 * K])
    assert not torch.equal(a[:K], b[:K])


def test_unsupported_prior_falls_through_to_the_two_launch_route():
    D = 3
    prior = MultivariateNormal(torch.zeros(D, device="cuda"), torch.eye(D, device="cuda"))
    post = _ratio_posterior(prior)
    torch.manual_seed(5)
    xs = torch.randn(4, 3, device="cuda")
    fused = _batched_spec(post, xs, 10)
    kind, p0, p1 = fused.fused_spec[:3]
    assert kind == 1
    # the entry point itself refuses every prior but a box under the logit map
    nre = fused.nre_persistent
    pk, zs = nre["net"].packed(torch.device("cuda"))
    C = 40
    f = lambda *shape: torch.zeros(*shape, device="cuda")
    i = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda")
    args = [f(C, D), f(C, D), f(C, D), i(C, D), i(C, 4), f(C, 8), f(C, 1, D), i(1)]
    tail = [f(C, D), f(C), f(C)]
    rc = _lib.load().sbi_amd_nre_mcmc_slice_run(
        nre["net"].hyper.c_config(), _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(nre["x"]), 4, 10, 1, 0, 3.0e38,
        *[_lib.ptr(t) for t in args], 1, 0, 1, kind, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(p0), _lib.ptr(p1), 0.0,
        *[_lib.ptr(t) for t in tail], 0, _lib.current_stream(torch.device("cuda")))
    assert rc == _lib.E_UNSUPPORTED
    # ... and the sampler, asked for the persistent kernel, runs two launches per tick instead
    out, s = _run_sampler(fused, torch.randn(C, D, device="cuda") * 0.3, True)
    assert s.route == "two_launch" and torch.isfinite(out).all()
    post.batched_persistent = True
    samples = post.sample_batched((20,), xs, num_chains=10, warmup_steps=5, init_strategy="proposal")
    assert samples.shape == (20, 4, D) and torch.isfinite(samples).all()
    assert post.posterior_sampler.route == "two_launch"


def test_persistent_kernel_answers_minus_inf_on_the_box_bound():
    """One tick of the persistent kernel from prepared states: the value it ticks on is log r + BoxUniform.log_prob --
    -inf for a theta that sits on the upper bound (sigmoid rounds to 1 from u = 40 on), finite inside and on the lower
    bound, the same bits as the two-launch route's sum."""
    prior = _box()
    post = _ratio_posterior(prior)
    D, K = 3, 4
    xs = torch.randn(1, 3, device="cuda")
    fused = _batched_spec(post, xs, K)
    kind, p0, p1, log_q = fused.fused_spec[:4]
    nre = fused.nre_persistent
    assert kind == 2 and nre["prior_log_prob"] == pytest.approx(-3 * torch.log(torch.tensor(4.0)).item())
    u = torch.zeros(K, D, device="cuda")
    u[0, 1] = 40.0                                   # onto the upper bound
    u[1, 2] = -200.0                                 # onto the lower bound (inside BoxUniform's support)
    u[2] = torch.tensor([0.3, -1.0, 2.0])
    theta = torch.empty_like(u)
    lad = torch.empty(K, device="cuda")
    lib = _lib.load()
    st = _lib.current_stream(torch.device("cuda"))
    assert lib.sbi_amd_mcmc_to_constrained(kind, K, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u), _lib.ptr(theta),
                                           _lib.ptr(lad), st) == 0
    assert theta[0, 1].item() == 2.0 and theta[1, 2].item() == -2.0
    want = log_q(theta)
    assert want[0].item() == float("-inf") and torch.isfinite(want[1:]).all()
    pk, zs = nre["net"].packed(torch.device("cuda"))
    x, nxt = u.clone(), u.clone()
    width = torch.full((K, D), 0.01, device="cuda")
    order = torch.arange(D, dtype=torch.int32, device="cuda").repeat(K, 1).contiguous()
    istate = torch.zeros(K, 4, dtype=torch.int32, device="cuda")
    fstate, samples = torch.zeros(K, 8, device="cuda"), torch.zeros(K, 1, D, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(K, device="cuda")
    theta_next, lad_next = theta.clone(), lad.clone()
    rc = lib.sbi_amd_nre_mcmc_slice_run(
        nre["net"].hyper.c_config(), _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(nre["x"]), 1, K, 1, 0, 3.0e38, _lib.ptr(x),
        _lib.ptr(nxt), _lib.ptr(width), _lib.ptr(order), _lib.ptr(istate), _lib.ptr(fstate), _lib.ptr(samples),
        _lib.ptr(done), 1, 0, 1, kind, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(nre["low"]), _lib.ptr(nre["high"]),
        nre["prior_log_prob"], _lib.ptr(theta_next), _lib.ptr(lad_next), _lib.ptr(scratch), 0, st)
    assert rc == 0
    assert torch.equal(scratch, want), (scratch, want)


@pytest.fixture(scope="module")
def linear_gaussian_task():
    """The 2-D linear-Gaussian task of tests/test_nre_gpu.py with a box prior; NRE_B and NPE trained once."""
    torch.manual_seed(0)
    dim = 2
    shift, cov = -1.0 * torch.ones(dim), 0.8 * torch.eye(dim)
    prior = BoxUniform(-2.0 * torch.ones(dim), 2.0 * torch.ones(dim), device="cuda")
    theta = prior.sample((3000,)).cpu()
    x = linear_gaussian(theta, shift, cov)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nre = NRE_B(prior=prior, device="cuda", show_progress_bars=False)
        nre.append_simulations(theta, x).train(max_num_epochs=60)
        npe = NPE(prior=prior, density_estimator=NSFConfig(), device="cuda", show_progress_bars=False)
        npe.append_simulations(theta, x).train(training_batch_size=100, max_num_epochs=40)
    torch.manual_seed(7)
    thetas = prior.sample((200,)).cpu()
    xs = linear_gaussian(thetas, shift, cov)
    return dict(prior=prior, nre=nre, npe=npe, thetas=thetas, xs=xs)


def test_batched_block_matches_the_single_observation_sampler(linear_gaussian_task):
    t = linear_gaussian_task
    params = dict(num_chains=20, thin=3, warmup_steps=100, init_strategy="resample")
    post = t["nre"].build_posterior(mcmc_parameters=params)
    xs = t["xs"][:4].cuda()
    torch.manual_seed(1)
    post.batched_persistent = False
    batched = post.sample_batched((500,), xs, show_progress_bars=False)
    assert batched.shape == (500, 4, 2) and bool(within_support(t["prior"], batched.reshape(-1, 2)).all())
    assert post.posterior_sampler.route == "two_launch"
    single = post.sample((500,), x=xs[2:3], show_progress_bars=False)
    score = c2st(batched[:, 2].cpu(), single.cpu()).item()
    other = c2st(batched[:, 0].cpu(), single.cpu()).item()
    print(f"c2st(batched block, single run) = {score:.3f}; against another observation's block: {other:.3f}")
    assert 0.4 <= score <= 0.62
    # the persistent kernel samples the same posterior, and is what a box prior gets when nothing is asked for
    post.batched_persistent = None
    pers = post.sample_batched((500,), xs, show_progress_bars=False)
    assert post.posterior_sampler.route == "nre_persistent"
    score_p = c2st(pers[:, 2].cpu(), single.cpu()).item()
    print(f"c2st(persistent batched block, single run) = {score_p:.3f}")
    assert 0.4 <= score_p <= 0.62


def _calibration(thetas, xs, posterior, L, reduce_fns="marginals"):
    ranks, dap = run_sbc(thetas, xs, posterior, num_posterior_samples=L, reduce_fns=reduce_fns, show_progress_bar=False)
    ecp, alpha = run_tarp(thetas, xs, posterior, num_posterior_samples=L, show_progress_bar=False)
    N = thetas.shape[0]
    assert ranks.shape[0] == N and dap.shape == thetas.shape and ecp.shape == alpha.shape == (N // 10 + 1,)
    assert torch.isfinite(ranks).all() and torch.isfinite(dap).all() and torch.isfinite(ecp).all()
    assert ((ranks >= 0) & (ranks <= L)).all() and ecp[0] == 0 and abs(ecp[-1].item() - 1) < 1e-6
    atc, _ = check_tarp(ecp, alpha)
    return check_uniformity_frequentist(ranks, L).min().item(), atc, ranks, dap


def test_sbc_and_tarp_end_to_end_through_batched_mcmc(linear_gaussian_task):
    """A trained posterior is better calibrated than the same posterior asked about permuted observations: smaller |atc|
    and a larger min KS p.  (No absolute threshold: nobody has measured one for a trained net.)"""
    t = linear_gaussian_task
    thetas, xs, L = t["thetas"], t["xs"], 100
    post = t["nre"].build_posterior(mcmc_parameters=dict(num_chains=20, thin=2, warmup_steps=50,
                                                         init_strategy="resample",
                                                         init_strategy_parameters=dict(num_candidate_samples=1000)))
    torch.manual_seed(3)
    t0 = time.time()
    p, atc, ranks, dap = _calibration(thetas, xs, post, L)
    wall = time.time() - t0
    assert ranks.shape == (200, 2)
    out = check_sbc(ranks, thetas, dap.cpu(), num_posterior_samples=L)
    assert set(out) == {"ks_pvals", "c2st_ranks", "c2st_dap"}
    perm = torch.randperm(200)
    p_perm, atc_perm, _, _ = _calibration(thetas, xs[perm], post, L)
    print(f"NRE_B batched MCMC: min KS p {p:.3g}, atc {atc:+.4f} ({wall:.1f} s for SBC + TARP); permuted observations: "
          f"min KS p {p_perm:.3g}, atc {atc_perm:+.4f}")
    assert p > p_perm and abs(atc) < abs(atc_perm)


def test_expected_coverage_end_to_end_through_the_direct_posterior(linear_gaussian_task):
    t = linear_gaussian_task
    thetas, xs, L = t["thetas"], t["xs"], 100
    post = t["npe"].build_posterior()
    torch.manual_seed(4)
    p, atc, ranks, _ = _calibration(thetas, xs, post, L, reduce_fns=post.log_prob)
    assert ranks.shape == (200, 1)
    perm = torch.randperm(200)
    p_perm, atc_perm, _, _ = _calibration(thetas, xs[perm], post, L, reduce_fns=post.log_prob)
    print(f"NPE direct, expected coverage: min KS p {p:.3g}, atc {atc:+.4f}; permuted observations: "
          f"min KS p {p_perm:.3g}, atc {atc_perm:+.4f}")
    assert p > p_perm and abs(atc) < abs(atc_perm)
