"""The end-to-end checks of MCABC / SMCABC, written once for both routes (TEST INFRASTRUCTURE): tests/test_abc_gpu.py
runs them on the device (kernels), tests/test_abc_host_cpu.py on the host (eager fallback).  Deterministic by replay:
the recording simulator of tests/abc_replay.py stores what it was handed, and the checks recompute in fp64 what must
have come out.  No row is left out of any comparison."""
import math

import pytest
import torch

from sbi_amd.inference import MCABC, SMCABC
from sbi_amd.utils.kde import KDEWrapper
from sbi_amd.utils.parity import row_parity
from sbi_amd.utils.torchutils import BoxUniform
from tests import abc_oracle
from tests.abc_replay import RecordingSimulator, exact_distances

X_O = torch.tensor([[0.25, -0.5]])


def prior(device, half=2.0):
    return BoxUniform(-half * torch.ones(2), half * torch.ones(2), device=device)


def mcabc(device, sim, distance="l2", **kw):
    return MCABC(sim, prior(device), distance=distance, simulation_batch_size=500, show_progress_bars=False, **kw)


def check_mcabc_quantile(device, distance):
    sim = RecordingSimulator()
    theta, summary = mcabc(device, sim, distance)(X_O, 2000, quantile=0.1, return_summary=True)
    rec_theta, rec_x = sim.recorded()
    assert rec_theta.shape == (2000, 2)
    d = exact_distances(X_O, rec_x, distance)
    order = torch.argsort(d, stable=True)[:200]
    assert theta.device.type == device and theta.shape == (200, 2)
    assert torch.equal(theta.cpu(), rec_theta[order])
    assert set(summary) == {"distances", "x"}
    assert summary["distances"].shape == (200,) and summary["x"].shape == (200, 2)
    assert torch.equal(summary["x"].cpu(), rec_x[order])
    if distance == "l2":      # the square root of an exact number: within one rounding of the fp64 value
        assert torch.allclose(summary["distances"].cpu().double(), d[order], rtol=1.2e-7, atol=0)
    else:
        assert torch.equal(summary["distances"].cpu().double(), d[order])


def check_mcabc_eps(device):
    sim = RecordingSimulator()
    theta = mcabc(device, sim)(X_O, 2000, eps=0.6)
    rec_theta, rec_x = sim.recorded()
    keep = exact_distances(X_O, rec_x, "l2") < 0.6          # d^2 is a multiple of 1/64: none within 1e-3 of 0.36
    assert 0 < int(keep.sum()) < 2000
    assert torch.equal(theta.cpu(), rec_theta[keep])
    with pytest.raises(AssertionError, match="No parameters accepted, eps=1e-06 too small"):
        mcabc(device, RecordingSimulator())(X_O, 100, eps=1e-6)
    with pytest.raises(AssertionError, match="Eps or quantile must be passed, but not both."):
        mcabc(device, RecordingSimulator())(X_O, 100, eps=1.0, quantile=0.1)


def check_mcabc_iid_and_kde(device):
    sim = RecordingSimulator()
    x_o = torch.round(torch.randn(5, 2) * 4) / 8
    theta, summary = mcabc(device, sim, "mmd")(x_o, 300, quantile=0.1, num_iid_samples=5, return_summary=True)
    assert theta.shape == (30, 2) and summary["x"].shape == (30, 5, 2)
    assert bool((summary["distances"][1:] >= summary["distances"][:-1]).all())
    with pytest.raises(AssertionError, match="simulated data needs batch dimension"):
        mcabc(device, sim, "mmd").distance(x_o.to(device), torch.zeros(4, 2, device=device))
    kde, summary = mcabc(device, RecordingSimulator())(X_O, 1000, quantile=0.1, kde=True, return_summary=True,
                                                       kde_kwargs=dict(bandwidth="scott"))
    assert isinstance(kde, KDEWrapper) and set(summary) == {"theta", "distances", "x"}
    assert kde.sample(7).shape == (7, 2)
    lra = mcabc(device, RecordingSimulator())(X_O, 1000, quantile=0.1, lra=True, sass=True)
    assert lra.shape == (75, 2) and bool(torch.isfinite(lra).all())


def smcabc(device, sim, variant="C", kernel="gaussian", half=2.0):
    return SMCABC(sim, prior(device, half), simulation_batch_size=500, show_progress_bars=False,
                  algorithm_variant=variant, kernel=kernel)


def check_populations(inference, summary, num_particles, budget, filled_last=False, resampled=False):
    """The budget may run out inside the last population, which is then filled up with the best particles of the
    population before it (or, without `use_last_pop_samples`, replaced by it): those rows keep their old distances,
    inside the epsilon before.  `filled_last` False: no population may hold such a row unless it IS the one before.
    `resampled`: with ess_min a population's particles may have been redrawn, so its rows no longer pair up with its
    distances and only the distances are checked."""
    eps = summary["epsilons"]
    assert inference.simulation_counter <= budget + num_particles          # at most one batch past the budget
    assert all(e1 <= e0 for e0, e1 in zip(eps, eps[1:]))
    assert len({len(summary[k]) for k in ("particles", "weights", "epsilons", "distances", "xs")}) == 1
    for p, lw, e, d, x in zip(summary["particles"], summary["weights"], eps, summary["distances"], summary["xs"]):
        assert p.shape == (num_particles, 2) and lw.shape == (num_particles,) and x.shape == (num_particles, 2)
        assert bool((d[1:] >= d[:-1]).all()), "a population is sorted by distance"
        over = d > e
        if bool(over.any()):
            assert p is summary["particles"][-1] and (filled_last or torch.equal(p, summary["particles"][-2]))
            before = {tuple(r.tolist()) for r in summary["particles"][-2].cpu()}
            assert resampled or all(tuple(r.tolist()) in before for r in p[over].cpu())
            assert bool((d[over] <= eps[-2]).all())
        assert abs(float(lw.double().exp().sum()) - 1.0) <= 1e-5


def check_smcabc(device, variant, kernel, use_last_pop_samples):
    sim = RecordingSimulator()
    inference = smcabc(device, sim, variant, kernel)
    theta, summary = inference(X_O, num_particles=100, num_initial_pop=500, num_simulations=2000, epsilon_decay=0.5,
                               use_last_pop_samples=use_last_pop_samples, return_summary=True)
    check_populations(inference, summary, 100, 2000, filled_last=use_last_pop_samples)
    assert set(summary) == {"particles", "weights", "epsilons", "distances", "xs"}
    assert len(summary["particles"]) >= 2 and torch.equal(theta, summary["particles"][-1])
    # the initial population: the 100 closest of the first 500 recorded simulations, in order
    rec_theta, rec_x = sim.recorded()
    d0 = exact_distances(X_O, rec_x[:500], "l2")
    order = torch.argsort(d0, stable=True)[:100]
    assert torch.equal(summary["particles"][0].cpu(), rec_theta[:500][order])
    assert summary["epsilons"][0] == pytest.approx(float(d0[order[-1]].float()))
    # every later (particle, x, distance) is a recorded simulation with its exact distance
    seen = {tuple(r.tolist()) for r in torch.cat((rec_theta, rec_x), dim=1)}
    for p_k, x_k, d_k in zip(summary["particles"][1:], summary["xs"][1:], summary["distances"][1:]):
        assert all(tuple(r.tolist()) in seen for r in torch.cat((p_k, x_k), dim=1).cpu())
        assert torch.allclose(d_k.cpu().double(), exact_distances(X_O, x_k.cpu(), "l2"), rtol=1.2e-7, atol=0)
    # the last population's weights against the fp64 formula on the population before it
    old, old_lw, new = summary["particles"][-2], summary["weights"][-2], summary["particles"][-1]
    previous_returned = torch.equal(new, old)
    if use_last_pop_samples or not previous_returned:
        want = abc_oracle.smc_log_weights(inference.prior.log_prob(new), new, old, old_lw, inference.kernel_variance,
                                          kernel)
        p = row_parity(summary["weights"][-1].cpu(), want)
        print(f"{device} variant {variant} {kernel}: last log-weights worst_scaled={p['worst_scaled']:.3e}")
        assert torch.isfinite(want).all() and p["exceed_frac"] == 0, p
    else:
        # (the population before, returned again: renormalised once more, which moves a log-weight by an ulp at most)
        assert torch.allclose(summary["weights"][-1], old_lw, rtol=0, atol=1e-6)


def check_smcabc_resampling(device):
    """Variant C perturbs with the (narrow) weighted covariance of the population before, so under a prior much wider
    than the posterior (half width 4 against ~0.5) the importance weights come out uneven: measured on the host over
    eight seeds the relative effective sample size of a population after the first falls to 0.7 .. 0.89, below
    ess_min = 0.9, and the population is resampled to uniform weights.  3000 simulations give four or more
    populations, each one a chance."""
    inference = smcabc(device, RecordingSimulator(), "C", "gaussian", half=4.0)
    _, summary = inference(X_O, num_particles=100, num_initial_pop=500, num_simulations=3000, epsilon_decay=0.5,
                           ess_min=0.9, return_summary=True, distance_based_decay=True)
    check_populations(inference, summary, 100, 3000, filled_last=True, resampled=True)
    assert inference.num_resamples >= 1
    uniform = torch.full((100,), -math.log(100))
    assert any(torch.allclose(lw.cpu(), uniform, atol=1e-6) for lw in summary["weights"][1:])


def check_smcabc_kde(device):
    inference = smcabc(device, RecordingSimulator())
    kde = inference(X_O, num_particles=100, num_initial_pop=500, num_simulations=1500, epsilon_decay=0.5, kde=True,
                    kde_sample_weights=True)
    assert isinstance(kde, KDEWrapper)
    g = torch.Generator().manual_seed(2)
    pts = (X_O + 0.3 * torch.randn(64, 2, generator=g)).to(device)
    want = abc_oracle.kde_log_density(pts, kde.kde.samples, kde.kde.bandwidth, kde.kde.weights)
    p = row_parity(kde.log_prob(pts).cpu(), want)
    print(f"{device} kde log_prob worst_scaled={p['worst_scaled']:.3e} bandwidth={kde.kde.bandwidth:.4f}")
    assert p["exceed_frac"] == 0, p
    s = kde.sample(1000)
    assert s.shape == (1000, 2) and s.device.type == device and bool(torch.isfinite(s).all())
