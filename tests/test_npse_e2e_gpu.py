"""NPSE end to end on the GPU: the trainer + posterior on the linear-Gaussian task of tests/test_fmpe_e2e_gpu.py (analytic
posterior known), sampled with the default fused SDE sampler and with the probability-flow ODE."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sde_type", ["ve", "vp"])
def test_npse_trains_and_recovers_linear_gaussian_posterior(sde_type):
    from torch.distributions import Independent, Normal

    from sbi_amd.inference import NPSE
    from sbi_amd.utils.metrics import c2st

    torch.manual_seed(0)
    D, n = 3, 4000
    sp, sn = 1.0, 0.5
    prior = Independent(Normal(torch.zeros(D, device="cuda"), sp * torch.ones(D, device="cuda")), 1)
    theta = prior.sample((n,))
    x = theta + sn * torch.randn_like(theta)
    inference = NPSE(prior=prior, sde_type=sde_type, device="cuda", show_progress_bars=False)
    est = inference.append_simulations(theta, x).train(training_batch_size=200, max_num_epochs=MAX_EPOCHS)
    s = inference.summary
    assert s["validation_loss"][-1] < s["validation_loss"][0]
    posterior = inference.build_posterior(est)
    assert posterior.sample_with == "sde"
    x_o = torch.tensor([[0.8, -0.4, 0.2]], device="cuda")
    samples = posterior.sample((4000,), x=x_o)
    assert samples.shape == (4000, D)
    k = sp**2 / (sp**2 + sn**2)
    mean_true = (x_o[0] * k).cpu()
    std_true = (sp**2 * sn**2 / (sp**2 + sn**2)) ** 0.5
    m, sd = samples.mean(0).cpu(), samples.std(0).cpu()
    print(sde_type, "posterior mean", m.tolist(), "true", mean_true.tolist(), "std", sd.tolist(), "true", std_true)
    assert (m - mean_true).abs().max() < 0.12
    assert ((sd - std_true).abs() / std_true).max() < 0.25
    exact = mean_true + std_true * torch.randn(4000, D)
    score = float(c2st(samples.cpu(), exact))
    print(f"c2st(NPSE {sde_type} sde, exact) =", score)
    assert score < 0.56     # measured at 60 epochs: 0.516 (ve), 0.530 (vp)
    # the probability-flow ODE of the same trained net
    ode = inference.build_posterior(est, sample_with="ode").sample((4000,), x=x_o)
    score_ode = float(c2st(ode.cpu(), exact))
    print(f"c2st(NPSE {sde_type} ode, exact) =", score_ode)
    assert ode.shape == (4000, D) and score_ode < 0.56     # measured: 0.537 (ve), 0.517 (vp)
    # batched observations: (samples, batch, D)
    sb = posterior.sample_batched((50,), x=torch.stack([x_o[0], -x_o[0]]))
    assert sb.shape == (50, 2, D)
    assert (sb[:, 0].mean(0).cpu() - mean_true).abs().max() < 0.4
    assert (sb[:, 1].mean(0).cpu() + mean_true).abs().max() < 0.4
    sb = inference.build_posterior(est, sample_with="ode").sample_batched((20,), x=torch.stack([x_o[0], -x_o[0]]))
    assert sb.shape == (20, 2, D)
    with pytest.raises(NotImplementedError):
        posterior.log_prob(samples[:4], x=x_o)


MAX_EPOCHS = 60      # the budget of tests/test_fmpe_e2e_gpu.py
