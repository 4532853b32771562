"""Cheap quality metrics of a variational posterior (sbi/samplers/vi/vi_quality_control.py): the PSIS k-hat of the
importance weights p / q ("psis") and the R^2 of a line through (q, p) at draws of q ("prop") or of the prior
("prop_prior").  The draws, log q and the potential are the device kernels of whatever sits underneath; the
generalised-Pareto fit runs on the host in fp64 (samplers/importance/importance_sampling.py `gpdfit`).
"""

from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch
from torch import Size

from sbi_amd.samplers.importance.importance_sampling import (exponentiate_weights, gpdfit, importance_sample,
                                                             largest_weight_indices)

_QUALITY_METRIC: Dict[str, Callable] = {}
_METRIC_MESSAGE: Dict[str, Optional[str]] = {}


def register_quality_metric(cls: Optional[Callable] = None, name: Optional[str] = None,
                            msg: Optional[str] = None) -> Callable:
    """Register `cls(posterior, N) -> float` under `name` with a one-line reading aid."""

    def _register(fn: Callable) -> Callable:
        key = fn.__name__ if name is None else name
        if key in _QUALITY_METRIC:
            raise ValueError(f"The metric {key} is already registered")
        _QUALITY_METRIC[key] = fn
        _METRIC_MESSAGE[key] = msg
        return fn

    return _register if cls is None else _register(cls)


def get_quality_metric(name: str) -> Tuple[Callable, str]:
    return _QUALITY_METRIC[name], _METRIC_MESSAGE[name]


def basic_checks(posterior, N: int = int(5e4)) -> None:
    """Finite samples inside the prior support, finite log_prob at posterior and at prior draws."""
    prior = posterior._prior
    assert prior is not None, "Posterior has no `._prior` attribute."
    with torch.no_grad():
        prior_samples = prior.sample(Size((N,)))
        samples = posterior.sample(Size((N,)))
        assert torch.isfinite(samples).all(), "Some of the samples are not finite"
        try:
            support = prior.support
        except (NotImplementedError, AttributeError):
            support = None
        if support is not None:
            assert support.check(samples).all(), "Some of the samples are not within the prior support."
        assert torch.isfinite(posterior.log_prob(samples)).all(), "The log probability is not finite for some samples"
        assert torch.isfinite(posterior.log_prob(prior_samples)).all(), \
            "The log probability is not finite for some samples"


def psis_diagnostics(potential_fn: Callable, q, N: int = int(5e4)) -> float:
    """The shape k-hat of a generalised Pareto distribution fitted to the largest importance weights p / q (Yao et al.
    2018): constant weights mean a perfect q; k > 1 means an importance-sampling estimate of infinite variance."""
    with torch.no_grad():
        _, log_importance_weights = importance_sample(potential_fn=potential_fn, proposal=q, num_samples=N)
        importance_weights = exponentiate_weights(log_importance_weights.reshape(-1))
        largest = importance_weights[largest_weight_indices(importance_weights)]
    k, _ = gpdfit(largest)
    return float(k)


def proportional_to_joint_diagnostics(potential_function: Callable, q, proposal=None, N: int = int(5e4)) -> float:
    """R^2 of the least-squares line through the origin of (q(theta), p(theta, x_o)) at draws of `proposal` (q when
    None): q proportional to the joint gives 1."""
    with torch.no_grad():
        samples = (q if proposal is None else proposal).sample(Size((N,)))
        X = q.log_prob(samples).exp().double()
        Y = potential_function(samples).exp().double()
        w = (X * Y).sum() / (X * X).sum()
        var_res = torch.sum((Y - w * X) ** 2)
        var_tot = torch.sum((Y - Y.mean()) ** 2)
    return float(1 - var_res / var_tot)


@register_quality_metric(name="psis", msg="\t Good: Smaller than 0.5  Bad: Larger than 1.0 \t\
         NOTE: Less sensitive to mode collapse.")
def psis_q(posterior, N: int = int(5e4)):
    basic_checks(posterior)
    return psis_diagnostics(posterior.potential_fn, posterior.q, N=N)


@register_quality_metric(name="prop", msg="\t Good: Larger than 0.5, best is 1.0  Bad: Smaller than 0.5")
def proportionality(posterior, N: int = int(5e4)):
    basic_checks(posterior)
    return proportional_to_joint_diagnostics(posterior.potential_fn, posterior.q, N=N)


@register_quality_metric(name="prop_prior", msg="\t Good: Larger than 0.5, best is 1.0  Bad: Smaller than 0.5")
def proportionality_prior(posterior, N: int = int(5e4)):
    basic_checks(posterior)
    return proportional_to_joint_diagnostics(posterior.potential_fn, posterior.q, proposal=posterior._prior, N=N)
