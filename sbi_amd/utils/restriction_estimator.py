"""Truncated proposals (TSNPE): ``get_density_thresholder`` and ``RestrictedPrior``.

Mirror of the two pieces of sbi/utils/restriction_estimator.py that truncated sequential NPE needs (:484-521 and
:613-846; Deistler et al. 2022, "Truncated proposals for scalable and hassle-free simulation-based inference").  A
``RestrictedPrior`` is the prior cut down to the region a callable accepts -- here the high-probability region of the
previous round's posterior.  Truncation needs no proposal correction: ``append_simulations(theta, x,
proposal=restricted_prior)`` keeps the data in round 0 and training stays on the maximum-likelihood loss, which is
what gives the MDN and the affine MAF (no atomic loss) a multi-round route.

The draws and log-densities behind the threshold and behind every accept/reject decision are the estimator's
kernels; rejection goes through ``accept_reject_sample`` (one compaction launch per iteration), SIR through
``sampling_importance_resampling`` (one selection launch per iteration).  The classifier-based
``RestrictionEstimator`` / ``AcceptRejectFunction`` of the reference are not part of this module.
"""

from __future__ import annotations

from typing import Any, Callable, Optional

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.samplers.importance.sir import sampling_importance_resampling
from sbi_amd.samplers.rejection.rejection import accept_reject_sample
from sbi_amd.utils.torchutils import ensure_theta_batched, process_device


def get_density_thresholder(dist: Any, quantile: float = 1e-4,
                            num_samples_to_estimate_support: int = 1_000_000) -> Callable:
    """A callable that is True for theta inside the `1 - quantile` high-probability region of `dist` (which needs
    `.sample()` and `.log_prob()`).  The threshold is the element of rank `int(quantile * N)` of the ascending
    log-densities of N draws (selected with `kthvalue`: the sorted array's element exactly, without the sort)."""
    samples = dist.sample((num_samples_to_estimate_support,))
    log_probs = dist.log_prob(samples).reshape(-1)
    rank = int(quantile * num_samples_to_estimate_support)
    log_prob_threshold = torch.kthvalue(log_probs, rank + 1).values

    def density_thresholder(theta: Tensor) -> Tensor:
        theta_log_probs = dist.log_prob(theta)
        return (theta_log_probs > log_prob_threshold.to(theta_log_probs.device)).bool()

    density_thresholder.log_prob_threshold = log_prob_threshold
    return density_thresholder


class RestrictedPrior(Distribution):
    """The prior restricted to the region `accept_reject_fn` accepts."""

    def __init__(self, prior: Distribution, accept_reject_fn: Callable, posterior: Optional[Any] = None,
                 sample_with: str = "rejection", device: str = "cpu") -> None:
        """`posterior` is only the proposal of `sample_with="sir"`."""
        super().__init__(validate_args=False)
        self._prior = prior            # (this name is what the NPE trainer looks for to keep the data in round 0)
        self._accept_reject_fn = accept_reject_fn
        self._posterior = posterior
        self._sample_with = sample_with
        self._device = process_device(device)
        self.acceptance_rate: Optional[Tensor] = None      # only defined after rejection sampling

    def sample(self, sample_shape=torch.Size(), sample_with: Optional[str] = None,
               max_sampling_batch_size: int = 10_000, oversampling_factor: int = 1024,
               save_acceptance_rate: bool = False, show_progress_bars: bool = False,
               print_rejected_frac: bool = True) -> Tensor:
        """`"rejection"`: prior draws kept where the accept function is True.  `"sir"`: one winner among
        `oversampling_factor` posterior draws, weighted by accept (0 / 1) over the posterior density.

        `oversampling_factor` is honoured here: it is forwarded as `num_candidate_samples`.  (The reference passes it
        under a name that its SIR function swallows in `**kwargs`, so its SIR route always uses 32 candidates.)"""
        shape = torch.Size(sample_shape)
        num_samples = shape.numel()
        sample_with = self._sample_with if sample_with is None else sample_with
        if sample_with == "rejection":
            samples, acceptance_rate = accept_reject_sample(
                proposal=lambda sample_shape, **kwargs: self._prior.sample(sample_shape),
                accept_reject_fn=self._accept_reject_fn, num_samples=num_samples,
                show_progress_bars=show_progress_bars, max_sampling_batch_size=max_sampling_batch_size,
                alternative_method="sample_with='sir'", acceptance_on_device=False)
            acceptance_rate = acceptance_rate.min().item()
            if save_acceptance_rate:
                self.acceptance_rate = torch.as_tensor(acceptance_rate)
            if print_rejected_frac:
                print(f"The `RestrictedPrior` rejected {(1.0 - acceptance_rate) * 100:.1f}% of prior samples. You will "
                      f"get a speed-up of {(1.0 / acceptance_rate - 1.0) * 100:.1f}%.")
        elif sample_with == "sir":
            assert self._posterior is not None, (
                "In order to use SIR sampling, you must provide a `posterior`: "
                "`RestrictionEstimator(..., posterior=posterior)`.")
            samples = sampling_importance_resampling(
                lambda theta: self._accept_reject_fn(theta).type(torch.float32), proposal=self._posterior,
                num_samples=num_samples, num_candidate_samples=oversampling_factor,
                show_progress_bars=show_progress_bars, max_sampling_batch_size=max_sampling_batch_size,
                device=self._device)
        else:
            raise ValueError("Only [rejection | sir] implemented as `method`")
        return samples.reshape((*shape, -1)).to(self._device)

    def log_prob(self, theta: Tensor, norm_restricted_prior: bool = True, track_gradients: bool = False,
                 prior_acceptance_params: Optional[dict] = None) -> Tensor:
        """Prior log-density inside the accepted region (minus log of the accepted prior mass when
        `norm_restricted_prior`), -inf outside."""
        theta = ensure_theta_batched(torch.as_tensor(theta))
        with torch.set_grad_enabled(track_gradients):
            prior_log_prob = self._prior.log_prob(theta)
            accepted = self._accept_reject_fn(theta).bool().to(prior_log_prob.device)
            masked = torch.where(accepted, prior_log_prob, torch.full_like(prior_log_prob, float("-inf")))
            if not norm_restricted_prior:
                return masked
            acceptance = self.prior_acceptance(**(prior_acceptance_params or {}))
            return masked - torch.log(acceptance).to(masked.device)

    @torch.no_grad()
    def prior_acceptance(self, num_rejection_samples: int = 10_000, force_update: bool = False,
                         show_progress_bars: bool = False, rejection_sampling_batch_size: int = 10_000) -> Tensor:
        """Fraction of prior draws the accept function keeps, from the acceptance rate of a rejection-sampling run."""
        if self.acceptance_rate is None or force_update:
            self.sample(torch.Size((num_rejection_samples,)), sample_with="rejection",
                        show_progress_bars=show_progress_bars, max_sampling_batch_size=rejection_sampling_batch_size,
                        save_acceptance_rate=True)
        return self.acceptance_rate

    @property
    def mean(self) -> Tensor:
        raise NotImplementedError("Mean is not implemented for RestrictedPrior.")

    @property
    def variance(self) -> Tensor:
        raise NotImplementedError("Variance is not implemented for RestrictedPrior.")

    @property
    def support(self):
        try:
            return self._prior.support
        except AttributeError as e:
            raise NotImplementedError("Support is not implemented for this RestrictedPrior.") from e
