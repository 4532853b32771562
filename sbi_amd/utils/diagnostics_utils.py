"""Posterior samples for a batch of observations, the common front of SBC and TARP (sbi/utils/diagnostics_utils.py).

`posterior.sample_batched` does the work wherever it exists: every posterior kind here has one except the rejection
posterior.  When it raises NotImplementedError or AssertionError (a sampler method that is not vectorised), the
observations are sampled one after the other in this process: no joblib, no worker processes.  A VIPosterior
(single-x: its `sample_batched` raises NotImplementedError) takes that loop and samples only at the x it was trained on.
"""

from __future__ import annotations

import warnings
from typing import Tuple

import torch
from torch import Tensor


def get_posterior_samples_on_batch(xs: Tensor, posterior, sample_shape, num_workers: int = 1,
                                   show_progress_bar: bool = False, use_batched_sampling: bool = True) -> Tensor:
    """(*sample_shape, len(xs), D) posterior samples, observation b conditioned on xs[b]."""
    sample_shape = tuple(torch.Size(sample_shape))
    num_xs = len(xs)
    if num_workers is not None and num_workers > 1:
        warnings.warn(f"num_workers={num_workers} is ignored: the observations are sampled in one batched call on the "
                      "device (or one after the other in this process), not in worker processes.", stacklevel=2)
    posterior_samples = None
    if use_batched_sampling:
        try:
            posterior_samples = posterior.sample_batched(sample_shape, x=xs, show_progress_bars=show_progress_bar)
        except (NotImplementedError, AssertionError):
            warnings.warn("Batched sampling not implemented for this posterior. Falling back to non-batched sampling.",
                          stacklevel=2)
    if posterior_samples is None:
        from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior

        if isinstance(posterior, MCMCPosterior):
            warnings.warn(f"Using non-batched sampling. Depending on the number of different xs ({num_xs}), this might "
                          "take a lot of time.", stacklevel=2)
        seeds = torch.randint(0, 2**32, (num_xs,))
        outputs = []
        for x, seed in zip(xs, seeds):
            torch.manual_seed(int(seed))
            outputs.append(posterior.sample(sample_shape, x=x, show_progress_bars=False))
        # (batch, *sample_shape, D) -> (*sample_shape, batch, D)
        stacked = torch.stack(outputs)
        posterior_samples = stacked.movedim(0, -2)
    assert tuple(posterior_samples.shape[:-1]) == sample_shape + (num_xs,), (
        f"Expected batched posterior samples of shape {sample_shape + (num_xs,)} got "
        f"{tuple(posterior_samples.shape[:-1])}.")
    return posterior_samples


def remove_nans_and_infs_in_x(thetas: Tensor, xs: Tensor) -> Tuple[Tensor, Tensor]:
    """Drop the (theta, x) pairs whose x holds a NaN or an Inf, with a warning that counts them."""
    flat = xs.reshape(xs.shape[0], -1)
    is_nan = torch.isnan(flat).any(dim=1)
    is_inf = torch.isinf(flat).any(dim=1)
    num_nans, num_infs = int(is_nan.sum()), int(is_inf.sum())
    if num_nans == 0 and num_infs == 0:
        return thetas, xs
    valid = ~is_nan & ~is_inf
    warnings.warn(f"Found {num_nans} NaNs and {num_infs} Infs in the data. These will be ignored below. Beware that only "
                  f"{int(valid.sum())} / {len(xs)} samples are left.", stacklevel=2)
    return thetas[valid.to(thetas.device)], xs[valid]
