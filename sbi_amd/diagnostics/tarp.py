"""TARP, tests of accuracy with random points (Lemos, Coogan et al. 2023), with the signatures and return conventions of
sbi/diagnostics/tarp.py.

Distances, coverage fractions and the histogram stay where the posterior samples live; `ecp` and `alpha` (num_bins + 1
numbers each) are what comes back.  The bin edges are laid out on the host from the two extreme coverage values, so that
they are the same numbers whatever device counted.
"""

from __future__ import annotations

import warnings
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from sbi_amd.utils.diagnostics_utils import get_posterior_samples_on_batch, remove_nans_and_infs_in_x
from sbi_amd.utils.metrics import l2


def run_tarp(thetas: Tensor, xs: Tensor, posterior, references: Optional[Tensor] = None,
             num_posterior_samples: int = 1000, num_workers: int = 1, show_progress_bar: bool = True,
             distance: Callable = l2, num_bins: Optional[int] = None, z_score_theta: bool = True,
             use_batched_sampling: bool = True) -> Tuple[Tensor, Tensor]:
    """(ecp, alpha): expected coverage probability on the grid of credibility levels `alpha`, both (num_bins + 1,).
    `references` (N, D) default to uniform draws from the box the true parameters span; `num_bins` to N // 10."""
    thetas, xs = remove_nans_and_infs_in_x(thetas, xs)
    num_tarp_samples, dim_theta = thetas.shape
    if num_tarp_samples < 100:
        warnings.warn("Number of TARP samples should be on the order of 100s to give reliable results.", stacklevel=2)
    posterior_samples = get_posterior_samples_on_batch(xs, posterior, (num_posterior_samples,), num_workers,
                                                       show_progress_bar=show_progress_bar,
                                                       use_batched_sampling=use_batched_sampling)
    assert posterior_samples.shape == (num_posterior_samples, num_tarp_samples, dim_theta), \
        f"Wrong posterior samples shape for TARP: {posterior_samples.shape}"
    if references is None:
        references = get_tarp_references(thetas)
    return _run_tarp(posterior_samples, thetas, references, distance, num_bins, z_score_theta)


def _unit_box(span_of: Tensor):
    """v -> v rescaled so that `span_of`'s rows span [0, 1] per parameter (run_tarp's `z_score_theta`)."""
    start = span_of.amin(dim=0, keepdim=True)
    extent = span_of.amax(dim=0, keepdim=True) - start + 1e-10
    return lambda v: (v - start) / extent


def _run_tarp(posterior_samples: Tensor, thetas: Tensor, references: Tensor, distance: Callable = l2,
              num_bins: Optional[int] = None, z_score_theta: bool = False) -> Tuple[Tensor, Tensor]:
    """The TARP curve from (L, N, D) draws, (N, D) true parameters and (N, D) reference points, on the draws' device."""
    L, N = posterior_samples.shape[:2]
    dev = posterior_samples.device
    assert references.shape == thetas.shape, "references must have the same shape as thetas"
    bins = N // 10 if num_bins is None else num_bins
    draws, truth, refs = posterior_samples, thetas.to(dev), references.to(dev)
    if z_score_theta:
        draws, truth, refs = map(_unit_box(truth), (draws, truth, refs))
    # per observation: the fraction of its draws that lie closer to its reference point than its true parameter does
    radius = distance(refs, truth)                                              # (N,)
    coverage = (distance(refs, draws) < radius).sum(dim=0) / L                  # (N,)
    # histogram over [min, max] in `bins` equal bins, left edges inclusive, the last bin closed
    lowest, highest = coverage.min().item(), coverage.max().item()
    if lowest == highest:                                                       # one value: a unit-wide range around it
        lowest, highest = lowest - 0.5, highest + 0.5
    alpha = torch.linspace(lowest, highest, bins + 1, dtype=coverage.dtype)
    edges = alpha.to(dev)
    which = (torch.bucketize(coverage, edges, right=True) - 1).clamp_(0, bins - 1)
    counts = torch.bincount(which, minlength=bins).to(coverage.dtype)
    ecp = torch.cumsum(counts, dim=0) / counts.sum()
    ecp = torch.cat([torch.zeros(1, dtype=ecp.dtype, device=dev), ecp])
    return ecp, edges


def get_tarp_references(thetas: Tensor) -> Tensor:
    """One reference point per true parameter, uniform in the box the true parameters span, (N, D)."""
    lo, hi = thetas.min(dim=0).values, thetas.max(dim=0).values
    return lo + (hi - lo) * torch.rand(thetas.shape, dtype=thetas.dtype, device=thetas.device)


def check_tarp(ecp: Tensor, alpha: Tensor) -> Tuple[float, float]:
    """(atc, ks_pval): the area between the ecp curve and the diagonal over the upper half of the alpha grid (about 0
    when calibrated, negative for a too-narrow posterior, positive for a too-wide one) and the p-value of the
    two-sample Kolmogorov-Smirnov test between ecp and alpha."""
    from scipy.stats import kstest

    ecp, alpha = ecp.detach().cpu(), alpha.detach().cpu()
    upper = slice(alpha.numel() // 2, None)                 # the grid's upper half, middle point included
    step = (alpha[1] - alpha[0]).item()
    atc = torch.sum(ecp[upper] - alpha[upper]).item() * step
    return atc, float(kstest(ecp.numpy(), alpha.numpy())[1])
