"""Potential of NRE: the classifier's log ratio summed over the iid trials of x_o plus the log-prior.

Mirror of sbi/inference/potentials/ratio_based_potential.py (and the ``BasePotential`` x_o handling,
base_potential.py:16-105).  With iid x_o (the default of ``set_x``) the potential is sum_i log r(theta, x_i) +
log p(theta).  The reference's ``_log_ratios_over_trials`` (ratio_based_potential.py:122-160) repeats theta against
every trial and evaluates every pair; here, without gradients, ONE pass of sbi_amd_nre_log_ratio_trials reads the
trials and the thetas in place and sums each theta's trials in a fixed order.  With gradients (``track_gradients``,
``map()``), the pairs go through the per-pair kernel's autograd bridge.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.neural_nets.estimators.ratio_estimator import RatioEstimator
from sbi_amd.utils.sbiutils import mcmc_transform
from sbi_amd.utils.torchutils import ensure_theta_batched


def log_ratios_over_trials_generic(x: Tensor, theta: Tensor, estimator: RatioEstimator,
                                   track_gradients: bool = False) -> Tensor:
    """The reference's `_log_ratios_over_trials`: every (trial, theta) pair, summed over the trials (theta-major
    pairs: theta c against trials 0 .. T - 1, the layout of the trials kernel)."""
    T, N = x.shape[0], theta.shape[0]
    th = theta.reshape(N, -1).repeat_interleave(T, dim=0) if T > 1 else theta.reshape(N, -1)
    with torch.set_grad_enabled(track_gradients):
        lr = estimator._log_ratio_rows(th, x.reshape(T, -1), T)
        return lr.reshape(N, T).sum(1)


class RatioBasedPotential:
    def __init__(self, ratio_estimator: RatioEstimator, prior: Distribution,
                 x_o: Optional[Tensor] = None, device: str = "cpu"):
        self.ratio_estimator = ratio_estimator
        self.prior = prior
        self.device = device
        self._x_o: Optional[Tensor] = None
        self._x_is_iid: Optional[bool] = None
        self.ratio_estimator.eval()
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

    def to(self, device: str) -> "RatioBasedPotential":
        self.device = device
        self.ratio_estimator.to(device)
        if hasattr(self.prior, "to"):
            self.prior = self.prior.to(device)
        if self._x_o is not None:
            self._x_o = self._x_o.to(device)
        return self

    # -- evaluation -----------------------------------------------------------------------
    def log_ratio_over_trials(self, theta: Tensor, track_gradients: bool = False) -> Tensor:
        """sum_i log r(theta, x_i) per theta row: the trials kernel without gradients, the per-pair autograd bridge
        with them."""
        x = self.x_o.reshape(self.x_o.shape[0], -1)
        if not track_gradients:
            return self.ratio_estimator.log_ratio_iid_trials(x, theta)
        return log_ratios_over_trials_generic(x, theta, self.ratio_estimator, True)

    def __call__(self, theta: Tensor, track_gradients: bool = True) -> Tensor:
        """sum_i log r(theta, x_i) + log p(theta); shape (num_thetas,)."""
        theta = ensure_theta_batched(torch.as_tensor(theta)).to(self.device)
        if self.x_is_iid:
            lr = self.log_ratio_over_trials(theta, track_gradients)
            with torch.set_grad_enabled(track_gradients):
                return lr + self.prior.log_prob(theta)
        if theta.shape[0] != self.x_o.shape[0]:
            raise ValueError(
                f"Batch size mismatch: {theta.shape[0]} and {self.x_o.shape[0]}. When performing batched sampling for "
                "multiple `x`, the batch size of `theta` must match the batch size of `x`."
            )
        with torch.set_grad_enabled(track_gradients):
            lr = self.ratio_estimator._log_ratio_rows(theta.reshape(theta.shape[0], -1),
                                                      self.x_o.reshape(self.x_o.shape[0], -1), self.x_o.shape[0])
            return lr + self.prior.log_prob(theta)


def ratio_estimator_based_potential(ratio_estimator: RatioEstimator, prior: Distribution, x_o: Optional[Tensor],
                                    enable_transform: bool = True) -> Tuple[RatioBasedPotential, object]:
    """(potential_fn, mcmc_transform(prior)) -- ratio_based_potential.py:20-52."""
    device = str(next(ratio_estimator.parameters()).device)
    potential_fn = RatioBasedPotential(ratio_estimator, prior, x_o, device=device)
    theta_transform = mcmc_transform(prior, device=device, enable_transform=enable_transform)
    return potential_fn, theta_transform
