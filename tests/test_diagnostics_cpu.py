"""sbi_amd.diagnostics on the CPU: run_sbc / check_sbc / get_nltp / run_tarp / check_tarp against
tests/golden/diagnostics_reference.pt (written by the reference's own functions, tools/make_golden_diagnostics.py) and on a
stand-in posterior that answers `sample_batched` with the analytic linear-Gaussian posterior."""

import os
import warnings

import pytest
import torch

from sbi_amd.diagnostics import check_sbc, check_tarp, get_nltp, run_sbc, run_tarp
from sbi_amd.diagnostics.sbc import _run_sbc, check_uniformity_frequentist
from sbi_amd.diagnostics.tarp import _run_tarp
from sbi_amd.utils.diagnostics_utils import get_posterior_samples_on_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diagnostics_reference.pt")


def reduce_sqnorm(theta, x):      # the callable reduce of tools/make_golden_diagnostics.py
    return (theta**2).sum(-1) + x.reshape(-1)[0]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


@pytest.mark.parametrize("case", ["calibrated", "narrow", "wide"])
def test_ranks_and_ks_pvalues_equal_the_reference(golden, case):
    c = golden["cases"][case]
    L = golden["num_posterior_samples"]
    for key, fns in (("marginals", "marginals"), ("callable", reduce_sqnorm)):
        ranks = _run_sbc(golden["thetas"], golden["xs"], c["posterior_samples"], fns, show_progress_bar=False)
        assert ranks.shape == c[f"ranks_{key}"].shape and ranks.dtype == torch.float32
        assert torch.equal(ranks, c[f"ranks_{key}"])                      # integers: exact
        pvals = check_uniformity_frequentist(ranks, L)
        want = c[f"ks_pvals_{key}"]
        print(case, key, pvals.tolist(), want.tolist())
        assert pvals.shape == want.shape
        assert ((pvals.double() - want.double()).abs() <= 1e-9 * want.double().abs()).all()


@pytest.mark.parametrize("case", ["calibrated", "narrow", "wide"])
@pytest.mark.parametrize("z_score", [True, False])
def test_tarp_curve_and_area_equal_the_reference(golden, case, z_score):
    """ecp within 1 / N per entry (a distance that ties to the last ulp may fall on the other side of a bin edge), atc
    therefore within (num_bins / 2) / N."""
    c = golden["cases"][case]
    tag = "z" if z_score else "raw"
    N = golden["thetas"].shape[0]
    ecp, alpha = _run_tarp(c["posterior_samples"], golden["thetas"], golden["references"], num_bins=None,
                           z_score_theta=z_score)
    num_bins = N // 10
    assert ecp.shape == alpha.shape == (num_bins + 1,)
    print(case, tag, "max |ecp - ref|", (ecp - c[f"ecp_{tag}"]).abs().max().item())
    assert torch.allclose(alpha, c[f"alpha_{tag}"], rtol=0, atol=1e-6)
    assert ((ecp - c[f"ecp_{tag}"]).abs() <= 1.0 / N + 1e-6).all()
    atc, ks = check_tarp(ecp, alpha)
    print(case, tag, "atc", atc, "ref", c[f"atc_{tag}"])
    assert abs(atc - c[f"atc_{tag}"]) <= (num_bins / 2) / N
    assert isinstance(atc, float) and isinstance(ks, float) and 0.0 <= ks <= 1.0


class AnalyticPosterior:
    """theta ~ N(0, 1), x = theta + 0.5 eps: p(theta | x) = N(x / 1.25, 0.2), drawn with its std scaled by `scale`."""

    def __init__(self, scale=1.0, batched=True, error=NotImplementedError):
        self.scale, self.batched, self.error = scale, batched, error
        self.batched_calls = self.single_calls = self.log_prob_batched_calls = 0

    def _std(self):
        return self.scale * 0.2**0.5

    def sample_batched(self, sample_shape, x, show_progress_bars=True):
        self.batched_calls += 1
        if not self.batched:
            raise self.error("no batched sampling here")
        return x / 1.25 + self._std() * torch.randn(*sample_shape, *x.shape)

    def sample(self, sample_shape, x=None, show_progress_bars=True):
        self.single_calls += 1
        return x.reshape(-1) / 1.25 + self._std() * torch.randn(*sample_shape, x.numel())

    def log_prob(self, theta, x=None):
        raise AssertionError("the expected-coverage route must not evaluate one observation at a time")

    def log_prob_batched(self, theta, x):
        self.log_prob_batched_calls += 1
        return torch.distributions.Normal(x / 1.25, self._std()).log_prob(theta).sum(-1)


def _task(seed, N=300, D=3):
    torch.manual_seed(seed)
    thetas = torch.randn(N, D)
    return thetas, thetas + 0.5 * torch.randn(N, D)


def _diagnose(scale, seed=0, N=300, L=200):
    thetas, xs = _task(seed, N)
    post = AnalyticPosterior(scale)
    ranks, dap = run_sbc(thetas, xs, post, num_posterior_samples=L, show_progress_bar=False)
    assert ranks.shape == (N, 3) and dap.shape == (N, 3)
    pvals = check_uniformity_frequentist(ranks, L)
    ecp, alpha = run_tarp(thetas, xs, post, num_posterior_samples=L, show_progress_bar=False)
    atc, _ = check_tarp(ecp, alpha)
    print(f"scale {scale}: min KS p {pvals.min().item():.3g}, atc {atc:+.4f}")
    return pvals.min().item(), atc


def test_a_calibrated_posterior_passes():
    p, atc = _diagnose(1.0)
    assert p > 0.01 and abs(atc) < 0.03


def test_a_too_narrow_posterior_fails_with_negative_area():
    p, atc = _diagnose(0.5)
    assert p < 1e-6 and atc < -0.03


def test_a_too_wide_posterior_fails_with_positive_area():
    p, atc = _diagnose(2.0)
    assert p < 1e-6 and atc > 0.03


def test_check_sbc_returns_the_three_checks():
    thetas, xs = _task(3, N=120)
    ranks, dap = run_sbc(thetas, xs, AnalyticPosterior(), num_posterior_samples=100, show_progress_bar=False)
    out = check_sbc(ranks, thetas, dap, num_posterior_samples=100)
    assert set(out) == {"ks_pvals", "c2st_ranks", "c2st_dap"}
    assert out["ks_pvals"].shape == out["c2st_ranks"].shape == out["c2st_dap"].shape == (3,)
    assert ((out["c2st_dap"] > 0.35) & (out["c2st_dap"] < 0.65)).all()


@pytest.mark.parametrize("error", [NotImplementedError, AssertionError])
def test_fallback_loops_over_sample_in_this_process(error):
    thetas, xs = _task(1, N=12)
    post = AnalyticPosterior(batched=False, error=error)
    with pytest.warns(UserWarning, match="Falling back to non-batched sampling"):
        s = get_posterior_samples_on_batch(xs, post, (7,))
    assert s.shape == (7, 12, 3) and post.batched_calls == 1 and post.single_calls == 12
    # observation b's draws centre on its own posterior mean
    many = get_posterior_samples_on_batch(xs, post, (4000,), use_batched_sampling=False)
    assert torch.allclose(many.mean(0), xs / 1.25, atol=5 * 0.2**0.5 / 4000**0.5)
    assert post.batched_calls == 1
    # per-observation seeds from torch's generator: the same seed gives the same draws
    torch.manual_seed(5)
    a = get_posterior_samples_on_batch(xs, post, (3,), use_batched_sampling=False)
    torch.manual_seed(5)
    assert torch.equal(a, get_posterior_samples_on_batch(xs, post, (3,), use_batched_sampling=False))


def test_num_workers_is_accepted_and_ignored_with_a_warning():
    thetas, xs = _task(1, N=5)
    with pytest.warns(UserWarning, match="num_workers=4 is ignored"):
        s = get_posterior_samples_on_batch(xs, AnalyticPosterior(), (2,), num_workers=4)
    assert s.shape == (2, 5, 3)


def test_input_validation_and_warnings():
    thetas, xs = _task(2, N=20)
    post = AnalyticPosterior()
    with pytest.warns(UserWarning) as rec:
        run_sbc(thetas, xs, post, num_posterior_samples=10, show_progress_bar=False)
    text = " ".join(str(w.message) for w in rec)
    assert "Number of SBC samples should be on the order of 100s" in text
    assert "Number of posterior samples for ranking should be on the order" in text
    with pytest.raises(ValueError, match="Unequal number of parameters and observations"):
        run_sbc(thetas[:10], xs, post, num_posterior_samples=100, show_progress_bar=False)
    with pytest.raises(ValueError, match="marginals"):
        run_sbc(thetas, xs, post, num_posterior_samples=100, reduce_fns="joint", show_progress_bar=False)
    with pytest.warns(UserWarning, match="Number of TARP samples should be on the order of 100s"):
        run_tarp(thetas, xs, post, num_posterior_samples=100, num_bins=4, show_progress_bar=False)
    with pytest.raises(AssertionError, match="references must have the same shape"):
        run_tarp(thetas, xs, post, references=thetas[:5], num_posterior_samples=100, num_bins=4)
    with pytest.warns(UserWarning, match="less than 100 samples"):
        check_sbc(torch.rand(20, 3) * 100, thetas, thetas.flip(0), num_posterior_samples=100)
    with pytest.raises(ValueError, match="same shape"):
        check_sbc(torch.rand(120, 3) * 100, torch.randn(120, 3), torch.randn(100, 3), num_posterior_samples=100)
    # rows whose x holds a NaN / Inf are dropped, with a count
    bad = xs.clone()
    bad[3, 0], bad[7, 1] = float("nan"), float("inf")
    with pytest.warns(UserWarning, match="Found 1 NaNs and 1 Infs"):
        ranks, dap = run_sbc(thetas, bad, post, num_posterior_samples=100, show_progress_bar=False)
    assert ranks.shape == (18, 3) and dap.shape == (18, 3)


def test_expected_coverage_is_two_batched_log_prob_calls():
    thetas, xs = _task(4, N=150)
    post = AnalyticPosterior()
    ranks, _ = run_sbc(thetas, xs, post, num_posterior_samples=100, reduce_fns=post.log_prob, show_progress_bar=False)
    assert post.log_prob_batched_calls == 2 and ranks.shape == (150, 1)
    # the same ranks as asking one observation at a time
    torch.manual_seed(9)
    samples = post.sample_batched((100,), xs)
    dist = lambda th, x: torch.distributions.Normal(x / 1.25, 0.2**0.5).log_prob(th).sum(-1)
    assert torch.equal(_run_sbc(thetas, xs, samples, post.log_prob), _run_sbc(thetas, xs, samples, dist))
    assert check_uniformity_frequentist(ranks, 100).item() > 0.01
    # a list mixes both kinds; get_nltp asks all N in one call
    both = _run_sbc(thetas, xs, samples, [post.log_prob, reduce_sqnorm])
    assert both.shape == (150, 2)
    before = post.log_prob_batched_calls
    nltp = get_nltp(thetas, xs, post)
    assert post.log_prob_batched_calls == before + 1 and nltp.shape == (150,)
    assert torch.allclose(nltp, -dist(thetas, xs))
