"""MCABC / SMCABC, the distances and the KDE on the host route (the eager fallback of every kernel), against the fp64
oracle (tests/abc_oracle.py) and, where scikit-learn imports, against scikit-learn itself.  The same end-to-end checks
run on the device in tests/test_abc_gpu.py."""

import math
import warnings

import numpy as np
import pytest
import torch

from sbi_amd.inference.abc.abc_base import ABCBASE, polynomial_features
from sbi_amd.inference.abc.smcabc import weighted_covariance
from sbi_amd.simulators.simutils import simulate_in_batches
from sbi_amd.utils import kde as kde_mod
from sbi_amd.utils.metrics import (Distance, l1, l2, mmd_distance, mse_distance, regularized_ot_dual,
                                   unbiased_mmd_squared, wasserstein_2_squared, wasserstein_distance)
from sbi_amd.utils.parity import row_parity
from sbi_amd.utils.sbiutils import process_x
from tests import abc_checks, abc_oracle


@pytest.mark.parametrize("distance", ["l1", "mse", "l2"])
def test_mcabc_quantile_returns_exactly_the_closest(distance):
    abc_checks.check_mcabc_quantile("cpu", distance)


def test_mcabc_eps_and_messages():
    abc_checks.check_mcabc_eps("cpu")


def test_mcabc_iid_kde_lra_sass():
    abc_checks.check_mcabc_iid_and_kde("cpu")


@pytest.mark.parametrize("variant,kernel,fill", [("A", "gaussian", True), ("B", "gaussian", False),
                                                 ("C", "gaussian", True), ("C", "uniform", True),
                                                 ("C", "gaussian", False)])
def test_smcabc_populations_and_weights(variant, kernel, fill):
    abc_checks.check_smcabc("cpu", variant, kernel, fill)


def test_smcabc_resamples_on_a_low_ess():
    abc_checks.check_smcabc_resampling("cpu")


def test_smcabc_kde_and_lra_sass():
    abc_checks.check_smcabc_kde("cpu")
    from tests.abc_replay import RecordingSimulator

    inference = abc_checks.smcabc("cpu", RecordingSimulator())
    theta = inference(abc_checks.X_O, 100, 500, 1500, 0.5, lra=True, lra_with_weights=True, sass=True)
    assert theta.shape == (100, 2) and bool(torch.isfinite(theta).all())


def test_refusals_and_argument_checks():
    with pytest.raises(NotImplementedError, match="num_workers"):
        simulate_in_batches(lambda t: t, torch.zeros(3, 2), num_workers=2)
    with pytest.raises(NotImplementedError):
        ABCBASE(lambda t: t, None, num_workers=4)
    with pytest.raises(AssertionError, match="Kernel 'cauchy' not supported"):
        abc_checks.SMCABC(lambda t: t, abc_checks.prior("cpu"), kernel="cauchy")
    with pytest.raises(AssertionError, match="SMCABC variant 'D' not supported"):
        abc_checks.SMCABC(lambda t: t, abc_checks.prior("cpu"), algorithm_variant="D")
    with pytest.warns(UserWarning, match="requires_iid_data=False"):
        d = Distance(lambda a, b: (a - b).abs().sum(-1))
    assert d.requires_iid_data is False
    assert Distance("mmd").requires_iid_data and not Distance("l2").requires_iid_data
    with pytest.raises(AssertionError, match="must be one of"):
        Distance("cosine")
    assert process_x(torch.zeros(3), torch.Size([3])).shape == (1, 3)
    assert process_x(np.zeros((4, 3)), torch.Size([3])).shape == (4, 3)
    with pytest.raises(ValueError):
        process_x(torch.zeros(4), torch.Size([3]))
    out = simulate_in_batches(lambda t: t * 2, torch.ones(7, 2), sim_batch_size=3, show_progress_bars=False)
    assert out.shape == (7, 2) and bool((out == 2).all())


def test_distances_and_chunking():
    g = torch.Generator().manual_seed(0)
    x_o, x = torch.randn(1, 3, generator=g), torch.randn(50, 3, generator=g)
    assert torch.equal(l1(x_o, x), (x_o - x).abs().mean(-1)) and torch.equal(mse_distance(x_o, x), ((x_o - x) ** 2).mean(-1))
    for name in ("l1", "l2", "mse"):
        assert torch.equal(Distance(name, batch_size=7)(x_o, x), Distance(name)(x_o, x))
    xs_o, xs = torch.randn(6, 2, generator=g), torch.randn(50, 5, 2, generator=g) + 0.3
    for name, kw in (("mmd", {}), ("mmd", dict(scale=0.7)), ("wasserstein", dict(epsilon=0.5, tol=1e-5))):
        whole = Distance(name, distance_kwargs=kw)(xs_o, xs)
        assert whole.shape == (50,) and torch.equal(Distance(name, distance_kwargs=kw, batch_size=7)(xs_o, xs), whole)
    got = mmd_distance(xs_o, xs)
    want = torch.stack([unbiased_mmd_squared(xs_o, xs[b]) for b in range(50)])
    assert torch.allclose(got, want, atol=2e-6, rtol=0)
    with pytest.raises(AssertionError, match="simulated data needs batch dimension"):
        Distance("l2")(x_o[0], x[0])
    with pytest.raises(AssertionError):
        Distance("mmd")(xs_o, xs[0])


def test_wasserstein_fallback_matches_the_oracle():
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(4, 33, 3, generator=g), torch.randn(4, 17, 3, generator=g) + 0.5
    a, b = torch.full((4, 33), 1 / 33), torch.full((4, 17), 1 / 17)
    _, _, w64, _ = abc_oracle.sinkhorn(abc_oracle.squared_distances(x, y), a, b, 0.5, 1000, 1e-4)
    got = wasserstein_2_squared(x, y, epsilon=0.5, tol=1e-4)
    assert got.shape == (4,) and (((got.double() - w64).abs() / (1 + w64.abs())) <= 1e-5).all()
    assert wasserstein_2_squared(x[0], y[0], epsilon=0.5, tol=1e-4).shape == ()
    one = wasserstein_distance(x[0], y, epsilon=0.5, tol=1e-4)
    rep = wasserstein_2_squared(x[:1].repeat(4, 1, 1), y, epsilon=0.5, tol=1e-4)
    assert torch.equal(one, rep)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # reaching max_iter never warns
        coupling = regularized_ot_dual(a[0], b[0], abc_oracle.squared_distances(x[0], y[0]).float(), 0.5, 3, 1e-9)
    assert coupling.shape == (33, 17)


def test_weighted_covariance_is_numpys():
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(100, 3, generator=g), torch.rand(100, generator=g)
    assert torch.allclose(weighted_covariance(x, w), abc_oracle.weighted_covariance(x, w), rtol=1e-12, atol=1e-14)


def test_lra_and_sass_regressions_match_scikit_learn():
    from sklearn.linear_model import LinearRegression
    from sklearn.preprocessing import PolynomialFeatures

    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(200, 3, generator=g), torch.rand(200, generator=g) + 0.1
    theta = x @ torch.randn(3, 2, generator=g) + 0.1 * torch.randn(200, 2, generator=g) + 1.0
    obs = torch.randn(1, 3, generator=g)
    for sw in (None, w):
        model = LinearRegression().fit(x.numpy(), theta.numpy(), sample_weight=None if sw is None else sw.numpy())
        want = theta + torch.from_numpy(model.predict(obs.numpy()) - model.predict(x.numpy()))
        assert torch.allclose(ABCBASE._run_lra(theta, x, obs, sw), want, atol=1e-5)
    for degree in (1, 2, 3):
        expansion = PolynomialFeatures(degree=degree, include_bias=False)
        expanded = expansion.fit_transform(x.numpy())
        assert np.allclose(polynomial_features(x, degree).numpy(), expanded, atol=1e-6)
        model = LinearRegression().fit(expanded, theta.numpy())
        want = torch.from_numpy(expanded.astype(np.float32)) @ torch.tensor(model.coef_.T, dtype=torch.float32)
        assert torch.allclose(ABCBASE._get_sass_transform(theta, x, degree)(x), want, atol=1e-4)


@pytest.mark.parametrize("D", [1, 2, 10])
def test_kde_matches_scikit_learn_and_the_oracle(D):
    from sklearn.neighbors import KernelDensity

    g = torch.Generator().manual_seed(D)
    samples, pts = torch.randn(257, D, generator=g), torch.randn(64, D, generator=g)
    weights = torch.rand(257, generator=g) + 0.05
    for w in (None, weights):
        for bw in ("scott", "silvermann", 0.37):
            kde = kde_mod.get_kde(samples, bandwidth=bw, sample_weights=w)
            sk = KernelDensity(kernel="gaussian", bandwidth=kde.kde.bandwidth).fit(
                samples.numpy(), sample_weight=None if w is None else w.numpy())
            want = abc_oracle.kde_log_density(pts, samples, kde.kde.bandwidth, w)
            assert row_parity(kde.log_prob(pts), want)["exceed_frac"] == 0
            if D == 10 and bw == 0.37:
                continue      # (scikit-learn's tree itself is off the formula by up to 0.6 here: far tails in 10-D)
            sk_scores = torch.from_numpy(sk.score_samples(pts.numpy()))
            assert row_parity(want, sk_scores, tol=1e-9)["exceed_frac"] == 0
    assert kde_mod.get_kde(samples, "scott").kde.bandwidth == pytest.approx(257 ** (-1.0 / (D + 4)))
    with pytest.raises(AssertionError, match="invalid kde bandwidth name."):
        kde_mod.get_kde(samples, "silverman")
    with pytest.raises(ValueError, match="bandwidth must be positive"):
        kde_mod.get_kde(samples, -1.0)
    # a transform: log_prob carries the log-abs-det, samples come back through the inverse
    tf = torch.distributions.transforms.ExpTransform().inv
    pos = samples.exp()
    kde = kde_mod.get_kde(pos, 0.5, transform=tf)
    want = abc_oracle.kde_log_density(pts, samples, 0.5) - pts.double().sum(-1)
    assert row_parity(kde.log_prob(pts.exp()), want)["exceed_frac"] == 0
    assert bool((kde.sample(100) > 0).all())


@pytest.mark.parametrize("N,D", [(100, 2), (257, 1), (150, 3)])
def test_cv_search_is_grid_search_cv(N, D):
    """The zoom loop of get_kde(bandwidth="cv") against the reference's recipe run with scikit-learn's GridSearchCV:
    the per-fold score table of the first grid within the project bound, and the same selected bandwidth."""
    from sklearn.model_selection import GridSearchCV
    from sklearn.neighbors import KernelDensity

    g = torch.Generator().manual_seed(10 * N + D)
    samples = torch.randn(N, D, generator=g) * torch.linspace(0.5, 2.0, D)
    x = samples.numpy()
    std = x.std()
    grid0 = np.linspace(0.1 * std, 0.5 * std, 10)
    search = GridSearchCV(KernelDensity(kernel="gaussian"), {"bandwidth": grid0}, cv=20).fit(x)
    want = torch.tensor(np.stack([search.cv_results_[f"split{f}_test_score"] for f in range(20)], axis=1))
    table = kde_mod.cv_score_table(samples, grid0, 20)
    assert row_parity(table, want)["exceed_frac"] == 0
    p = row_parity(abc_oracle.cv_score_table(samples, grid0, 20), want, tol=1e-7)
    assert p["exceed_frac"] == 0, p      # (scikit-learn sums in tree order: its own fp64 rounding, not the formula)

    lower, upper, current_best, steps = 0.1 * std, 0.5 * std, -10000000, 10      # the recipe, on scikit-learn
    for _ in range(5):
        bandwidth_range = np.linspace(lower, upper, steps)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            search = GridSearchCV(KernelDensity(kernel="gaussian"), {"bandwidth": bandwidth_range}, cv=20).fit(x)
        if abs(current_best - search.best_score_) > 0.001:
            current_best = search.best_score_
        else:
            break
        second = list(search.cv_results_["rank_test_score"]).index(2)
        if search.best_index_ == 0 or search.best_index_ == steps:
            diff = (lower - upper) / steps
            lower, upper = search.best_index_ - diff, search.best_index_ + diff
        else:
            upper, lower = bandwidth_range[second], bandwidth_range[search.best_index_]
            if upper < lower:
                upper, lower = lower, upper
    # (numpy takes the standard deviation of the fp32 samples in fp32, the package in fp64: the grids agree to ~1e-7)
    assert kde_mod.get_kde(samples, "cv").kde.bandwidth == pytest.approx(search.best_params_["bandwidth"], rel=1e-6)


def test_cv_search_at_the_lower_end_of_the_grid():
    """Clustered data: the best bandwidth is the smallest of the first grid, the reference re-centres on the INDEX 0
    and half of the next grid is negative -- scored NaN, ranked last."""
    g = torch.Generator().manual_seed(4)
    samples = torch.cat((0.01 * torch.randn(60, 1, generator=g), 0.01 * torch.randn(60, 1, generator=g) + 5.0))
    samples = samples[torch.randperm(120, generator=g)]
    table = kde_mod.cv_score_table(samples, [0.3, -0.1, 0.0], 20)
    assert torch.isfinite(table[0]).all() and torch.isnan(table[1:]).all()
    assert list(kde_mod._ranks(np.array([1.0, math.nan, 3.0, 3.0]))) == [3, 4, 1, 1]
    std = float(samples.double().std(unbiased=False))
    first = kde_mod.cv_score_table(samples, np.linspace(0.1 * std, 0.5 * std, 10), 20).mean(1)
    assert int(first.argmax()) == 0
    bw = kde_mod.get_kde(samples, "cv").kde.bandwidth
    assert 0 < bw <= 0.04 * std + 1e-12          # from the second grid: (upper - lower) / 10 downwards
