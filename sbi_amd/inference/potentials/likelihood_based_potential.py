"""Potential of NLE: log-likelihood of x_o under the estimator q(x | theta) plus the log-prior.

Mirror of sbi/inference/potentials/likelihood_based_potential.py:24-236 (and the ``BasePotential`` x_o handling,
base_potential.py:16-105).  With iid x_o (the default of ``set_x``) the potential is sum_i log q(x_i | theta) +
log p(theta).  The reference builds every (trial, theta) pair (``_log_likelihoods_over_trials`` expands x_o to
(num_trials, num_theta, D)); an NSF estimator here answers with ONE pass of sbi_amd_nsf_log_prob_trials that reads the
trials and the thetas in place and sums each theta's trials in a fixed order.  The expand-log_prob-sum path stays for
whatever the kernel does not take (another estimator, hidden 65 - 128, gradients).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.neural_nets.estimators.base import ConditionalDensityEstimator
from sbi_amd.neural_nets.estimators.shape_handling import reshape_to_batch_event, reshape_to_sample_batch_event
from sbi_amd.utils.sbiutils import mcmc_transform
from sbi_amd.utils.torchutils import ensure_theta_batched


def log_likelihoods_over_trials_generic(x: Tensor, theta: Tensor, estimator: ConditionalDensityEstimator,
                                        track_gradients: bool = False) -> Tensor:
    """The reference's `_log_likelihoods_over_trials` (likelihood_based_potential.py:186-236): x (num_trials, *event)
    expanded against theta (num_theta, *event), one batched log_prob, summed over the trials."""
    x = reshape_to_sample_batch_event(x, event_shape=x.shape[1:], leading_is_sample=True)
    trailing_minus_ones = [-1 for _ in range(x.dim() - 2)]
    x = x.expand(-1, theta.shape[0], *trailing_minus_ones)
    theta = reshape_to_batch_event(theta, event_shape=theta.shape[1:])
    with torch.set_grad_enabled(track_gradients):
        return estimator.log_prob(x, condition=theta).sum(0)


class LikelihoodBasedPotential:
    def __init__(self, likelihood_estimator: ConditionalDensityEstimator, prior: Distribution,
                 x_o: Optional[Tensor] = None, device: str = "cpu"):
        self.likelihood_estimator = likelihood_estimator
        self.prior = prior
        self.device = device
        self._x_o: Optional[Tensor] = None
        self._x_is_iid: Optional[bool] = None
        self.likelihood_estimator.eval()
        if x_o is not None:
            self.set_x(x_o)

    # -- x_o handling (base_potential.py:56-105) ------------------------------------------
    def set_x(self, x_o: Optional[Tensor], x_is_iid: Optional[bool] = True) -> None:
        if x_o is not None:
            x_o = torch.as_tensor(x_o, dtype=torch.float32)
            if x_o.dim() == 1:
                x_o = x_o.unsqueeze(0)
            x_o = x_o.to(self.device)
        self._x_o = x_o
        self._x_is_iid = x_is_iid

    @property
    def x_is_iid(self) -> bool:
        if self._x_is_iid is None:
            raise ValueError("No observed data is available. Use `potential_fn.set_x(x_o)`.")
        return self._x_is_iid

    @property
    def x_o(self) -> Tensor:
        if self._x_o is None:
            raise ValueError("No observed data is available. Use `potential_fn.set_x(x_o)`.")
        return self._x_o

    @x_o.setter
    def x_o(self, x_o: Optional[Tensor]) -> None:
        self.set_x(x_o)

    def return_x_o(self) -> Optional[Tensor]:
        return self._x_o

    def to(self, device: str) -> "LikelihoodBasedPotential":
        self.device = device
        self.likelihood_estimator.to(device)
        if hasattr(self.prior, "to"):
            self.prior = self.prior.to(device)
        if self._x_o is not None:
            self._x_o = self._x_o.to(device)
        return self

    # -- evaluation -----------------------------------------------------------------------
    def log_likelihood_over_trials(self, theta: Tensor, track_gradients: bool = False) -> Tensor:
        """sum_i log q(x_i | theta) over the iid trials of x_o, per theta row: the trials kernel when the estimator
        has one (and no gradient is asked for), the expand-log_prob-sum path otherwise."""
        est = self.likelihood_estimator
        if not track_gradients and hasattr(est, "log_prob_iid_trials") and self.x_o.is_cuda and theta.is_cuda:
            ll = est.log_prob_iid_trials(self.x_o, theta)
            if ll is not None:
                return ll
        return log_likelihoods_over_trials_generic(self.x_o, theta, est, track_gradients)

    def __call__(self, theta: Tensor, track_gradients: bool = True) -> Tensor:
        """log q(x_o | theta) + log p(theta); shape (num_thetas,)."""
        theta = ensure_theta_batched(torch.as_tensor(theta)).to(self.device)
        if self.x_is_iid:
            ll = self.log_likelihood_over_trials(theta, track_gradients)
            with torch.set_grad_enabled(track_gradients):
                return ll + self.prior.log_prob(theta)
        # one (theta, x) pair per row (likelihood_based_potential.py:117-131)
        if theta.shape[0] != self.x_o.shape[0]:
            raise ValueError(
                f"Batch size mismatch: {theta.shape[0]} and {self.x_o.shape[0]}. When performing batched sampling for "
                "multiple `x`, the batch size of `theta` must match the batch size of `x`."
            )
        with torch.set_grad_enabled(track_gradients):
            lp = self.likelihood_estimator.log_prob(self.x_o.unsqueeze(0), condition=theta)
            return lp + self.prior.log_prob(theta)


def likelihood_estimator_based_potential(likelihood_estimator: ConditionalDensityEstimator, prior: Distribution,
                                         x_o: Optional[Tensor],
                                         enable_transform: bool = True) -> Tuple[LikelihoodBasedPotential, object]:
    """(potential_fn, mcmc_transform(prior)) -- likelihood_based_potential.py:24-56."""
    device = str(next(likelihood_estimator.parameters()).device)
    potential_fn = LikelihoodBasedPotential(likelihood_estimator, prior, x_o, device=device)
    theta_transform = mcmc_transform(prior, device=device, enable_transform=enable_transform)
    return potential_fn, theta_transform


class MixedLikelihoodBasedPotential(LikelihoodBasedPotential):
    """Deprecated thin alias (as in the reference): the mixed estimator goes through ``LikelihoodBasedPotential``."""

    def __init__(self, *args, **kwargs):
        import warnings

        warnings.warn("MixedLikelihoodBasedPotential is deprecated; use LikelihoodBasedPotential.", DeprecationWarning,
                      stacklevel=2)
        super().__init__(*args, **kwargs)

    def condition_on_theta(self, *args, **kwargs):
        raise NotImplementedError("sbi_amd: condition_on_theta is not implemented for the mixed likelihood "
                                  "potential; sample the full posterior and slice the draws")


def mixed_likelihood_estimator_based_potential(likelihood_estimator, prior, x_o, enable_transform: bool = True):
    """Deprecated thin alias of ``likelihood_estimator_based_potential``."""
    import warnings

    warnings.warn("mixed_likelihood_estimator_based_potential is deprecated; use "
                  "likelihood_estimator_based_potential.", DeprecationWarning, stacklevel=2)
    return likelihood_estimator_based_potential(likelihood_estimator, prior, x_o, enable_transform=enable_transform)
