"""NPSE with iid observations end to end on the GPU: the linear-Gaussian task and training budget of
tests/test_npse_e2e_gpu.py, then N = 4 observations composed with auto_gauss and gauss.  The bounds are coarse by design
(they catch a broken composition; tests/test_npse_iid_gpu.py is the pin); mean / std error and c2st against the analytic
posterior are printed and recorded."""

import pytest
import torch

from tests.parity_log import record

pytestmark = pytest.mark.gpu

MAX_EPOCHS = 60      # the budget of tests/test_npse_e2e_gpu.py


def test_npse_iid_concentrates_on_the_linear_gaussian_posterior():
    from torch.distributions import Independent, Normal

    from sbi_amd.inference import NPSE
    from sbi_amd.utils.metrics import c2st

    torch.manual_seed(0)
    D, n, N = 3, 4000, 4
    sp, sn = 1.0, 0.5      # analytic std ratio sqrt((1/sp^2 + 1/sn^2) / (1/sp^2 + N/sn^2)) = sqrt(5 / 17) = 0.54 <= 0.65
    prior = Independent(Normal(torch.zeros(D, device="cuda"), sp * torch.ones(D, device="cuda")), 1)
    theta = prior.sample((n,))
    x = theta + sn * torch.randn_like(theta)
    inference = NPSE(prior=prior, sde_type="ve", device="cuda", show_progress_bars=False)
    est = inference.append_simulations(theta, x).train(training_batch_size=200, max_num_epochs=MAX_EPOCHS)
    posterior = inference.build_posterior(est)
    theta_o = torch.tensor([0.6, -0.3, 0.2], device="cuda")
    xs = theta_o + sn * torch.randn(N, D, device="cuda")
    single = posterior.sample((2000,), x=xs[:1])
    prec = 1 / sp**2 + N / sn**2
    mean_true = (xs.sum(0) / sn**2 / prec).cpu()
    std_true = prec**-0.5
    std_single_true = (1 / sp**2 + 1 / sn**2) ** -0.5
    exact = mean_true + std_true * torch.randn(2000, D)
    for method in ("auto_gauss", "gauss"):
        draws = posterior.sample((2000,), x=xs, iid_method=method)
        assert draws.shape == (2000, D) and torch.isfinite(draws).all()
        assert prior.support.check(draws).all()
        m, sd = draws.mean(0).cpu(), draws.std(0).cpu()
        ratio = sd / single.std(0).cpu()
        score = float(c2st(draws.cpu(), exact))
        mean_err, std_err = float((m - mean_true).abs().max()), float(((sd - std_true).abs() / std_true).max())
        print(f"{method}: mean {m.tolist()} true {mean_true.tolist()} | std {sd.tolist()} true {std_true:.4f} | std ratio "
              f"to single-observation draws {ratio.tolist()} (analytic {std_true / std_single_true:.3f}) | c2st {score:.3f}")
        record("test_npse_iid_concentrates_on_the_linear_gaussian_posterior", method, mean_abs_err=mean_err,
               std_rel_err=std_err, c2st=score, std_ratio_max=float(ratio.max()))
        assert (ratio < 0.8).all()
        assert mean_err < std_single_true
    default = posterior.sample((64,), x=xs)          # iid_method=None -> auto_gauss
    assert default.shape == (64, D) and torch.isfinite(default).all()
    with pytest.raises(NotImplementedError, match="sde"):
        inference.build_posterior(est, sample_with="ode").sample((4,), x=xs)
    with pytest.raises(NotImplementedError):
        posterior.log_prob(draws[:4], x=xs)
