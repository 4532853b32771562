"""The misspecification test and the MMD metrics on the device (one launch of sbi_amd_mmd_rbf_splits per call) against
the host fallback at the same seed and against the fp64 oracle.  Bounds as in tests/test_mmd_kernel_gpu.py: 2e-6
absolute on an MMD."""
import pytest
import torch

from sbi_amd.diagnostics import calc_misspecification_mmd, calculate_baseline_mmd
from sbi_amd.utils import metrics
from sbi_amd.utils.mmd_splits import STAGE_FLOATS
from tests import mmd_oracle, parity_log

pytestmark = pytest.mark.gpu
MMD_ATOL = 2e-6
N, D, N_OBS, N_SHUFFLE, MAX_SAMPLES = 500, 10, 20, 64, 200


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(1)
    return torch.randn(N, D, generator=g), torch.randn(N_OBS, D, generator=g)


@pytest.mark.parametrize("mode", ["biased", "unbiased"])
def test_baseline_matches_the_fallback_at_the_same_seed(data, mode):
    x, _ = data
    host = calculate_baseline_mmd(N_OBS, x, n_shuffle=N_SHUFFLE, max_samples=MAX_SAMPLES, mode=mode, seed=31)
    dev = calculate_baseline_mmd(N_OBS, x.cuda(), n_shuffle=N_SHUFFLE, max_samples=MAX_SAMPLES, mode=mode, seed=31)
    assert dev.is_cuda and dev.shape == (N_SHUFFLE,) and dev.dtype == torch.float32
    err = (dev.cpu() - host).abs().max().item()
    print(f"baseline {mode}: max |device - fallback| = {err:.3e}")
    parity_log.record("mmd_baseline_device_vs_fallback", mode, max_abs=err, bound=MMD_ATOL)
    assert err <= MMD_ATOL


def test_p_values_match_the_fallback(data):
    x, x_obs = data
    kw = dict(n_shuffle=N_SHUFFLE, max_samples=MAX_SAMPLES, seed=31)
    p_host, (b_host, m_host) = calc_misspecification_mmd(x_obs, x, **kw)
    p_dev, (b_dev, m_dev) = calc_misspecification_mmd(x_obs.cuda(), x.cuda(), **kw)
    assert b_dev.is_cuda and m_dev.is_cuda and b_dev.shape == (N_SHUFFLE,)
    assert abs(m_dev.item() - m_host.item()) <= MMD_ATOL
    assert abs(m_dev.item() - mmd_oracle.misspecification_mmd(x_obs, x[:MAX_SAMPLES])) <= MMD_ATOL
    # one near-tie of a baseline value with the observed one may fall either side, not more
    assert abs(p_dev - p_host) <= 1.0 / N_SHUFFLE + 1e-12
    p_host, _ = calc_misspecification_mmd(x_obs + 3, x, **kw)
    p_dev, _ = calc_misspecification_mmd(x_obs.cuda() + 3, x.cuda(), **kw)
    assert p_host == 0.0 and p_dev == 0.0


def test_metrics_on_device_tensors_match_the_fp64_oracle():
    g = torch.Generator().manual_seed(9)
    for nx, ny, d, shift in [(130, 77, 10, 0.0), (64, 64, 3, 100.0), (2, 33, 1, 0.0)]:
        x = 2 * torch.randn(nx, d, generator=g) + 1 + shift
        y = 1.5 * torch.randn(ny, d, generator=g) + shift
        for scale in (None, 1.7):
            b = metrics.biased_mmd(x.cuda(), y.cuda(), scale)
            u = metrics.unbiased_mmd_squared(x.cuda(), y.cuda(), scale)
            assert b.is_cuda and u.is_cuda and b.dim() == 0 and u.dim() == 0
            eb = abs(b.item() ** 2 - mmd_oracle.biased_mmd(x, y, scale) ** 2)
            eu = abs(u.item() - mmd_oracle.unbiased_mmd_squared(x, y, scale))
            print(f"nx={nx} ny={ny} d={d} shift={shift} scale={scale}: biased^2 {eb:.3e} unbiased {eu:.3e}")
            # the bound holds on the squared biased MMD (sqrt divides the error by 2 sqrt); the unbiased estimator
            # carries the reference's factor 2
            assert eb <= MMD_ATOL and eu <= 2 * MMD_ATOL


def test_over_budget_inputs_take_the_fallback_instead_of_raising():
    g = torch.Generator().manual_seed(4)
    d = 64
    m = STAGE_FLOATS // (d | 1) + 1                               # one row past the kernel's LDS staging
    x = torch.randn(m + 30, d, generator=g)
    host = calculate_baseline_mmd(10, x, n_shuffle=2, max_samples=m, seed=8)
    dev = calculate_baseline_mmd(10, x.cuda(), n_shuffle=2, max_samples=m, seed=8)
    assert dev.is_cuda and torch.allclose(dev.cpu(), host, atol=MMD_ATOL, rtol=0)
