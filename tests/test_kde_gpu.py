"""The KDE on the device: `GaussianKDE.score_samples` and the cross-validation score table (one `sbi_amd_mixture_lse`
launch each) against the fp64 oracle within the project's row parity, and get_kde(bandwidth="cv") selecting the same
bandwidth as the host fallback on data where that selection is not a coin toss."""

import numpy as np
import pytest
import torch

from sbi_amd.utils import kde as kde_mod
from sbi_amd.utils.parity import row_parity
from tests import abc_oracle, parity_log

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N,D", [(2, 1), (257, 2), (1000, 10), (257, 1), (2, 10), (1000, 2)])
def test_score_samples(N, D, weighted):
    g = torch.Generator().manual_seed(N + D)
    samples, pts = torch.randn(N, D, generator=g), torch.randn(65, D, generator=g)
    w = torch.rand(N, generator=g) + 0.05 if weighted else None
    bw = N ** (-1.0 / (D + 4))
    kde = kde_mod.GaussianKDE(samples.cuda(), bw, None if w is None else w.cuda())
    want = abc_oracle.kde_log_density(pts, samples, bw, w)
    got = kde.score_samples(pts.cuda())
    p = row_parity(got.cpu(), want)
    print(f"N={N} D={D} weighted={weighted}: worst_scaled={p['worst_scaled']:.3e}")
    assert got.is_cuda and p["exceed_frac"] == 0, p
    assert row_parity(kde.score_samples(pts.cuda(), force_fallback=True).cpu(), want)["exceed_frac"] == 0


@pytest.mark.parametrize("N", [100, 257])
def test_cv_score_table(N):
    g = torch.Generator().manual_seed(N)
    samples = torch.randn(N, 2, generator=g)
    std = float(samples.double().std(unbiased=False))
    grid = np.linspace(0.1 * std, 0.5 * std, 10)
    want = abc_oracle.cv_score_table(samples, grid, 20)
    got = kde_mod.cv_score_table(samples.cuda(), grid, 20)
    p = row_parity(got.cpu(), want)
    print(f"cv table N={N}: worst_scaled={p['worst_scaled']:.3e}")
    assert got.is_cuda and got.shape == (10, 20) and p["exceed_frac"] == 0, p


def clustered(seed):
    g = torch.Generator().manual_seed(seed)
    samples = torch.cat((torch.randn(120, 2, generator=g), 0.3 * torch.randn(80, 2, generator=g) + 2.0))
    return samples[torch.randperm(200, generator=g)]


@pytest.mark.parametrize("seed", [7, 12, 36])
def test_cv_selects_the_same_bandwidth_as_the_host_fallback(seed):
    """The search zooms in until the best score stops moving, so its late repetitions compare scores that differ by
    1e-5 and less: there the selection is a coin toss between fp32 roundings, on any route.  These seeded data sets
    are the ones (of seeds 0 .. 59, scanned on the host) whose search ends after two repetitions with a clear winner
    in each (margins 0.17 / 3.8e-3, 0.17 / 6.6e-3, 0.15 / 4.6e-3).  The test ASSERTS that: on every grid the fallback
    visits, its best and second-best mean scores, and its stopping decision |best - previous best| against 1e-3, are
    more than 100 x the largest device-versus-fallback score difference seen on that data away from flipping.  Then
    both routes must select the same bandwidth, exactly."""
    samples = clustered(seed)
    trace = []
    want = kde_mod.cv_bandwidth(samples, trace=trace)
    gap, margin, previous = 0.0, float("inf"), -10000000.0
    for grid, host in trace:
        dev = kde_mod.cv_score_table(samples.cuda(), grid, 20).mean(1).cpu().numpy()
        ok = ~np.isnan(host)
        assert np.array_equal(np.isnan(dev), ~ok)
        gap = max(gap, float(np.abs(host[ok] - dev[ok]).max()))
        top = np.sort(host[ok])[::-1]
        margin = min(margin, float(top[0] - top[1]), abs(abs(previous - top[0]) - 0.001))
        previous = top[0]
    print(f"seed {seed}: repetitions={len(trace)} gap={gap:.3e} margin={margin:.3e} bandwidth={want:.6f}")
    parity_log.record("kde_cv_device_vs_host", f"seed{seed}", gap=gap, margin=margin)
    assert margin > 100 * gap, (margin, gap)
    assert kde_mod.get_kde(samples.cuda(), "cv").kde.bandwidth == want == kde_mod.get_kde(samples, "cv").kde.bandwidth
