"""Importance sampling: proposal draws and the logarithm of their importance weights.

Same contract as sbi/samplers/importance/importance_sampling.py:11-37.  Everything here is a call into the proposal
and the potential, whose sampling and log-density kernels do the work.
"""

from __future__ import annotations

from typing import Tuple

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
