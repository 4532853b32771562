"""MCABC and SMCABC end to end on the device, deterministic by replay (tests/abc_replay.py, tests/abc_checks.py): the
recording simulator stores every (theta, x) it is handed and the checks recompute on the host, in fp64, what must have
been accepted -- exactly, on grid data, with no row left out.  The SMC weights (one `sbi_amd_mixture_lse` launch per
population) are held to the project's row parity against the fp64 formula."""

import pytest
import torch

from tests import abc_checks
from tests.abc_replay import RecordingSimulator

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("distance", ["l1", "mse", "l2"])
def test_mcabc_quantile_returns_exactly_the_closest(distance):
    abc_checks.check_mcabc_quantile("cuda", distance)


def test_mcabc_eps_and_messages():
    abc_checks.check_mcabc_eps("cuda")


def test_mcabc_iid_kde_lra_sass():
    abc_checks.check_mcabc_iid_and_kde("cuda")


@pytest.mark.parametrize("variant,kernel,fill", [("A", "gaussian", True), ("B", "gaussian", False),
                                                 ("C", "gaussian", True), ("C", "uniform", True),
                                                 ("C", "gaussian", False)])
def test_smcabc_populations_and_weights(variant, kernel, fill):
    abc_checks.check_smcabc("cuda", variant, kernel, fill)


def test_smcabc_resamples_on_a_low_ess():
    abc_checks.check_smcabc_resampling("cuda")


def test_smcabc_kde_log_prob_and_samples():
    abc_checks.check_smcabc_kde("cuda")


def test_smcabc_lra_sass_and_wasserstein():
    inference = abc_checks.smcabc("cuda", RecordingSimulator())
    theta = inference(abc_checks.X_O, 100, 500, 1500, 0.5, lra=True, lra_with_weights=True, sass=True)
    assert theta.is_cuda and theta.shape == (100, 2) and bool(torch.isfinite(theta).all())
    inference = abc_checks.SMCABC(RecordingSimulator(), abc_checks.prior("cuda"), distance="wasserstein",
                                  distance_kwargs=dict(epsilon=0.1, tol=1e-4), simulation_batch_size=5000,
                                  show_progress_bars=False)
    x_o = torch.round(torch.randn(5, 2) * 4) / 8
    theta, summary = inference(x_o, 50, 200, 600, 0.8, num_iid_samples=5, return_summary=True)
    assert theta.shape == (50, 2) and summary["xs"][-1].shape == (50, 5, 2)
    assert inference.simulation_counter <= 600 * 5 + 50 * 5


def test_the_device_and_host_routes_give_the_same_weights():
    """The kernel route against the package's own eager fallback on one population (Gaussian and uniform kernels)."""
    g = torch.Generator().manual_seed(6)
    old, new = torch.randn(100, 2, generator=g).cuda(), torch.randn(77, 2, generator=g).cuda()
    old_lw = torch.log_softmax(torch.randn(100, generator=g), dim=0).cuda()
    for kernel, variance in (("gaussian", torch.tensor([[0.5, 0.2], [0.2, 0.4]]).cuda()),
                             ("uniform", torch.tensor([1.25, 0.75]).cuda())):
        inference = abc_checks.smcabc("cuda", RecordingSimulator(), "C", kernel)
        inference.kernel_variance = variance
        dev = inference.kernel_log_mixture(new, old, old_lw)
        host = inference.kernel_log_mixture(new, old, old_lw, force_fallback=True)
        fin = torch.isfinite(host)
        assert torch.equal(torch.isfinite(dev), fin)
        assert abc_checks.row_parity(dev[fin], host[fin])["exceed_frac"] == 0
