"""Misspecification diagnostics: could the observed data have come from the simulator at all?

Same functions, argument order, defaults, return shapes and error messages as sbi/diagnostics/misspecification.py:
an MMD permutation test in data or embedding space (Schmitt et al. 2023), and a log-probability test against a marginal
density estimator.  Written from the algorithm.

MI355X-first.  The reference's `calculate_baseline_mmd` is a Python loop over `n_shuffle` shuffles, each a randperm,
three `cdist`, an exact median read back with `.item()` and three exp + mean passes.  Here all shuffles are ONE launch
of `sbi_amd_mmd_rbf_splits` (include/sbi_amd_mmd.h): one workgroup per shuffle, the rows staged once in LDS, distances
from differences, the median by an exact radix select, fixed-order sums; the normalisation is a few vectorised
operations on the `(n_shuffle, 4)` result and nothing is read by the host.  The observed statistic is a second launch
with one split.  Host tensors, and shapes outside the kernel's LDS envelope (min(max_samples, N) * (D | 1) > 15 360),
take an eager-torch evaluation of the same splits (sbi_amd/utils/mmd_splits.py).

Randomness: the shuffles come from a keyed pseudo-random permutation (csrc/shuffle_prp.h), one key per shuffle derived
from `seed`.  They are NOT the reference's `torch.randperm` stream and cannot be; a given seed selects the same
shuffles on the device and on the host.  `seed=None` draws the seed from torch's global generator, so
`torch.manual_seed` makes a run reproducible.

Not built: `MarginalTrainer` and the `Marginal*Config` estimators `calc_misspecification_logprob` is usually fed with;
any object with `.log_prob(x)` and `.sample(shape)` serves.
"""

from __future__ import annotations

import warnings
from typing import Any, Optional

import torch
import torch.nn as nn
from torch import Tensor

from sbi_amd.utils.metrics import check_c2st
from sbi_amd.utils.mmd_splits import _dist, rbf_splits


def rbf_kernel(x: Tensor, y: Tensor, bandwidth: float):
    """(nx, ny) Gaussian kernel matrix exp(-|x_i - y_j|^2 / (2 bandwidth^2)); distances from differences."""
    dist = _dist(x, y)
    return torch.exp(-(dist**2) / (2.0 * bandwidth**2))


def _sums(x: Tensor, y: Tensor, bandwidth: Optional[float]) -> Tensor:
    """[bw, S_xx, S_yy, S_xy] (diagonals included, cross-pair median) for one pair of samples, on their device."""
    nx, ny = x.shape[0], y.shape[0]
    pool = torch.cat((x.reshape(nx, -1), y.reshape(ny, -1).to(x.device)))
    idx = torch.arange(nx + ny, device=pool.device).reshape(1, -1)
    bw = None if bandwidth is None else torch.as_tensor([float(bandwidth)], dtype=torch.float32, device=pool.device)
    return rbf_splits(pool, 1, nx + ny, nx, 0, 0, idx=idx, bandwidth=bw)[0]


def median_heuristic(x: Tensor, y: Tensor):
    """The (lower) median of the nx * ny Euclidean distances between x and y, as a float."""
    return _sums(x, y, None)[0].item()


def _normalise(sums: Tensor, n_a: int, n_b: int, mode: str) -> Tensor:
    """MMD from (..., 4) `[bw, S_aa, S_bb, S_ab]` whose within-set sums include the diagonal; the arithmetic in fp64."""
    s = sums.double()
    cross = 2.0 * s[..., 3] / (n_a * n_b)
    if mode == "biased":
        mmd = s[..., 1] / (n_a * n_a) + s[..., 2] / (n_b * n_b) - cross
    elif mode == "unbiased":
        # the reference's estimator as written: the diagonal stays in the sums, the divisor is m (m - 1)
        # (a float divisor: a one-row set divides by zero to inf / nan as the formula does, it does not raise)
        mmd = s[..., 1] / float(n_a * (n_a - 1)) + s[..., 2] / float(n_b * (n_b - 1)) - cross
    else:
        raise ValueError("mode should be either biased or unbiased")
    return mmd.to(torch.float32)


def compute_rbf_mmd(x: Tensor, y: Tensor, bandwidth: float = 1.0, mode: str = "biased"):
    if mode not in ("biased", "unbiased"):
        raise ValueError("mode should be either biased or unbiased")
    return _normalise(_sums(x, y, bandwidth), x.shape[0], y.shape[0], mode)


def compute_rbf_mmd_median_heuristic(x: Tensor, y: Tensor, mode: str = "biased"):
    """MMD with the bandwidth from the median heuristic (Garreau et al. 2018) on the cross distances."""
    if mode not in ("biased", "unbiased"):
        raise ValueError("mode should be either biased or unbiased")
    return _normalise(_sums(x, y, None), x.shape[0], y.shape[0], mode)


def _draw_seed(seed: Optional[int]) -> int:
    if seed is None:
        return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
    return int(seed)


def calculate_baseline_mmd(n_obs: int, y: Tensor, n_shuffle: int = 1_000, max_samples: int = 1_000,
                           mode: str = "biased", seed: Optional[int] = None):
    """MMDs between two sets of synthetic data: the distribution of the statistic under the null hypothesis that
    synthetic and observed samples share a distribution.

    Each of the `n_shuffle` shuffles takes min(max_samples, N) rows of `y` without replacement and compares the first
    `n_obs` of them with the rest.  Returns `(n_shuffle,)` fp32 on `y`'s device.  `seed`: see the module docstring (the
    shuffles are not the reference's randperm stream)."""
    N = y.shape[0]
    if n_obs > N:
        raise ValueError("n of observed samples should be less than n of synthetic samples")
    M = min(max_samples, N)
    if n_obs >= M:
        raise ValueError(f"n of observed samples ({n_obs}) should be less than the number of synthetic samples used "
                         f"per shuffle, min(max_samples, n of synthetic samples) = {M}: the second set would be empty")
    if mode not in ("biased", "unbiased"):
        raise ValueError("mode should be either biased or unbiased")
    sums = rbf_splits(y.reshape(N, -1), n_shuffle, M, n_obs, 0, 0, seed=_draw_seed(seed))
    return _normalise(sums, n_obs, M - n_obs, mode)


def calculate_p_misspecification(x_obs: Tensor, x: Tensor, n_shuffle: int = 1_000, max_samples: int = 1_000,
                                 mode: str = "biased", seed: Optional[int] = None):
    """p-value of the misspecification test: the share of baseline MMDs that are not below the observed one.
    Returns `p_val, (mmds_baseline, mmd)`."""
    mmds_baseline = calculate_baseline_mmd(x_obs.shape[0], x, n_shuffle=n_shuffle, max_samples=max_samples, mode=mode,
                                           seed=seed)
    mmd = compute_rbf_mmd_median_heuristic(x_obs.to(x.device), x[:max_samples], mode=mode)
    p_val = 1 - (mmds_baseline < mmd).sum().item() / n_shuffle
    return p_val, (mmds_baseline, mmd)


def calc_misspecification_mmd(x_obs: Tensor, x: Tensor, inference: Optional[Any] = None, mode: str = "x_space",
                              n_shuffle: int = 1_000, max_samples: int = 1_000, mmd_mode: str = "biased",
                              seed: Optional[int] = None):
    """Misspecification test based on MMD in data or embedding space.

    Args:
        x_obs: observed data.
        x: synthetic data.
        inference: a trained inference object (only for mode "embedding"; its `_neural_net.embedding_net` is used).
        mode: "x_space" or "embedding".
        n_shuffle: number of shuffles for the MMDs under H_0.
        max_samples: at most this many synthetic samples per shuffle.
        mmd_mode: "biased" or "unbiased".
        seed: selects the shuffles; None draws it from torch's global generator.

    Returns:
        p_val, (mmds_baseline, mmd).
    """
    if mode == "x_space":
        z_obs, z = x_obs, x
    elif mode == "embedding":
        if inference is None:
            raise ValueError("inference should not be None if mode is 'embedding'. "
                             "Please provide an sbi inference object.")
        if getattr(inference, "_neural_net", None) is None:
            raise ValueError("No neural net found. The inference object must be trained before "
                             "computing the MMD in mode 'embedding'.")
        net = inference._neural_net.embedding_net
        if isinstance(net, nn.Identity):
            warnings.warn("The embedding net might be the identity function, "
                          "in that case the MMD is computed in the x-space.", stacklevel=2)
        if net is None:
            raise AttributeError("embedding_net attribute is None but is required for misspecification detection.")
        with torch.no_grad():
            z_obs, z = net(x_obs).detach(), net(x).detach()
    else:
        raise ValueError("mode should be either 'x_space' or 'embedding'")
    return calculate_p_misspecification(z_obs, z, n_shuffle=n_shuffle, max_samples=max_samples, mode=mmd_mode,
                                        seed=seed)


def _log_prob_hypothesis_test(log_probs: Tensor, log_prob_xo: float, alpha: float = 0.05):
    """(p_value, reject_H0): the empirical CDF of `log_probs` at `log_prob_xo`, and whether it is below `alpha`."""
    p_value = (log_probs <= log_prob_xo).float().mean()
    return p_value, p_value < alpha


def calc_misspecification_logprob(x_val: Tensor, x_o: Tensor, estimator: Any, alpha: float = 0.05):
    """Is `estimator.log_prob(x_o)` unusually low among the log-probabilities of the known samples `x_val`?

    Host-side.  `estimator` is any object with `.log_prob(x)` and `.sample(shape)`: a marginal density estimator.  A
    C2ST between `x_val` and the estimator's samples comes first; when it is far from chance a warning says that the
    test below may not mean much.  Returns (p_value, reject_H0)."""
    log_probs_val = estimator.log_prob(x_val).detach()
    log_prob_xo = estimator.log_prob(x_o).detach().item()
    samples = estimator.sample(torch.Size((x_val.shape[0],)))
    try:
        check_c2st(x_val, samples, "MarginalEstimator")
    except AssertionError as e:
        warnings.warn(f"{str(e)} \nProceeding with logprob test, but results might not"
                      " be meaningful. Be careful with the interpretation!", stacklevel=2)
    return _log_prob_hypothesis_test(log_probs_val, log_prob_xo, alpha=alpha)
