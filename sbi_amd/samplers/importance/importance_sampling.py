"""Importance sampling: proposal draws and the logarithm of their importance weights.

Same contract as sbi/samplers/importance/importance_sampling.py:11-37.  Everything here is a call into the proposal
and the potential, whose sampling and log-density kernels do the work.  `exponentiate_weights`,
`largest_weight_indices` and `gpdfit` are what the Pareto-smoothed importance sampling diagnostic (k-hat) of the
variational posterior needs (same file of the reference, :40-143).
"""

from __future__ import annotations

import math
from typing import Tuple

import torch
from torch import Tensor


def importance_sample(potential_fn, proposal, num_samples: int = 1,
                      show_progress_bars: bool = False) -> Tuple[Tensor, Tensor]:
    """(samples, log importance weights) with `log_weights = potential_fn(samples) - proposal.log_prob(samples)`.
    A proposal whose `.sample` takes no progress-bar argument is sampled without one."""
    try:
        samples = proposal.sample((num_samples,), show_progress_bar=show_progress_bars)
    except TypeError:
        samples = proposal.sample((num_samples,))
    return samples, potential_fn(samples) - proposal.log_prob(samples)


def exponentiate_weights(log_weights: Tensor) -> Tensor:
    """exp(log_weights - max) over the FINITE entries (the output can be shorter than the input)."""
    log_weights = log_weights[torch.isfinite(log_weights)]
    return torch.exp(log_weights - log_weights.max())


def largest_weight_indices(weights: Tensor) -> Tensor:
    """Indices of the M = min(n / 5, 3 sqrt(n)) largest weights in ascending order of weight: the tail that PSIS fits
    (Vehtari, Gelman & Gabry 2017; Yao et al. 2018)."""
    n = len(weights)
    m = int(min(n / 5, 3 * math.sqrt(n)))
    return torch.argsort(weights)[n - m:]


def gpdfit(x: Tensor, sorted: bool = True, eps: float = 1e-8, return_quadrature: bool = False) -> Tuple:
    """(k, sigma) of a generalised Pareto distribution fitted to `x` by the empirical-Bayes estimate of Zhang &
    Stephens (2009) as PSIS uses it, in host fp64: a grid of M = 30 + floor(sqrt(N)) values of theta = -k / sigma,
        theta_j = 1 / x_max + (1 - sqrt(M / (j - 1/2))) / (3 x_q1),   j = 1..M,   x_q1 the first quartile,
    the profile log-likelihood l_j = N (log(-theta_j / k_j) - k_j - 1) with k_j = mean log1p(-theta_j x), weights
    w_j = 1 / sum_i exp(l_i - l_j) (those below 10 eps are dropped), theta = sum w_j theta_j, k = mean log1p(-theta x),
    sigma = -k / theta, and the weakly informative prior of PSIS on k: k <- (N k + 5) / (N + 10).
    `return_quadrature` also returns the per-node k_j (with the same prior) and the weights."""
    v = torch.as_tensor(x).detach().to("cpu", torch.float64).reshape(-1)
    if not sorted:
        v = torch.sort(v).values
    N = v.numel()
    M = 30 + int(math.sqrt(N))
    j = torch.arange(1, M + 1, dtype=torch.float64)
    first_quartile = v[int(N / 4 + 0.5) - 1]
    theta = 1.0 / v[-1] + (1.0 - torch.sqrt(M / (j - 0.5))) / (3.0 * first_quartile)
    k_nodes = torch.log1p(-theta[:, None] * v[None, :]).mean(dim=1)
    loglik = N * (torch.log(-theta / k_nodes) - k_nodes - 1.0)
    w = 1.0 / torch.exp(loglik[None, :] - loglik[:, None]).sum(dim=1)
    keep = w >= 10 * eps
    w, theta, k_nodes = w[keep], theta[keep], k_nodes[keep]
    w = w / w.sum()
    theta_hat = torch.sum(theta * w)
    k = torch.log1p(-theta_hat * v).mean()
    sigma = -k / theta_hat
    prior_weight = 10.0
    k = (k * N + prior_weight * 0.5) / (N + prior_weight)
    if return_quadrature:
        return k, sigma, (k_nodes * N + prior_weight * 0.5) / (N + prior_weight), w
    return k, sigma
