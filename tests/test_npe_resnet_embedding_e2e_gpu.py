"""NPE with a trainable ResNetEmbedding1D in front of the NSF, end to end on the device.

Linear-Gaussian task: theta in R^2 with a standard normal prior; x = A theta + noise in R^10 with a fixed design A, so
the posterior at x_o is an analytic Gaussian.  The kernel route and the `force_eager` twin are trained from the same
seeds on the same 2000 simulations for 20 epochs at batch 200, and each one's 2000 posterior draws are compared with
2000 draws of the analytic posterior by c2st.

Condition: the kernel route's c2st is at most the eager twin's + 0.05.  The c2st of 2000 + 2000 points has a standard
error of about 0.011, so the margin is 4 sigma of the yardstick.  No absolute c2st is asserted.  Both values go to the
parity artifact (tests/parity_log.py)."""
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd.inference import NPE
from sbi_amd.neural_nets import NSFConfig, ResNetEmbedding1D
from sbi_amd.utils.metrics import c2st
from tests import parity_log

pytestmark = pytest.mark.gpu

DIM, SIGMA, N, EPOCHS = 10, 1.0, 2000, 20


def design():
    return torch.randn(DIM, 2, generator=torch.Generator().manual_seed(7)) / 2.0


def analytic_posterior(x_o, A):
    precision = torch.eye(2) + A.T @ A / SIGMA**2
    cov = torch.linalg.inv(precision)
    return MultivariateNormal(cov @ (A.T @ x_o) / SIGMA**2, covariance_matrix=cov)


def train_and_sample(theta, x, x_o, force_eager):
    torch.manual_seed(3)
    emb = ResNetEmbedding1D(c_in=DIM, c_out=8, n_blocks=3, c_internal=32, c_hidden_final=32,
                            construct_mapping_kwargs={"c_hidden": 32})
    emb.force_eager = force_eager
    prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
    inf = NPE(prior=prior, density_estimator=NSFConfig(embedding_net=emb), device="cuda", show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = inf.append_simulations(theta, x).train(training_batch_size=200, max_num_epochs=EPOCHS)
    net = est.embedding_net[-1]
    assert isinstance(net, ResNetEmbedding1D) and net.force_eager == force_eager
    assert net.kernel_route(torch.zeros(200, DIM, device="cuda"))[0] == (not force_eager)
    torch.manual_seed(4)
    samples = inf.build_posterior().set_default_x(x_o[None]).sample((2000,), show_progress_bars=False).cpu()
    return samples, inf.summary["epochs_trained"][-1]


def test_npe_with_a_resnet_embedding_learns_what_the_eager_twin_learns():
    torch.manual_seed(0)
    A = design()
    theta = torch.randn(N, 2)
    x = theta @ A.T + SIGMA * torch.randn(N, DIM)
    x_o = torch.tensor([0.8, -0.5]) @ A.T + SIGMA * torch.randn(DIM)
    target = analytic_posterior(x_o, A).sample((2000,))
    scores = {}
    for name, force_eager in (("kernel", False), ("eager", True)):
        samples, epochs = train_and_sample(theta, x, x_o, force_eager)
        assert samples.shape == (2000, 2) and torch.isfinite(samples).all()
        scores[name] = c2st(samples, target).item()
        print(f"resnet embedding NPE [{name}] c2st={scores[name]:.3f} epochs={epochs}")
    parity_log.record("npe_resnet_embedding_e2e", "linear_gaussian", kernel_c2st=scores["kernel"],
                      eager_c2st=scores["eager"])
    assert scores["kernel"] <= scores["eager"] + 0.05, scores
