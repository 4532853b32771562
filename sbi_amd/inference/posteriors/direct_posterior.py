"""``DirectPosterior`` -- sample / evaluate the NPE posterior through the estimator.

Mirror of sbi/inference/posteriors/direct_posterior.py:44-523 (+ the x handling of
base_posterior.py:170-214): ``sample`` rejects draws outside the prior support via
``accept_reject_sample``; ``log_prob`` is the estimator log-prob, -inf outside the
support, minus log(acceptance rate) (``leakage_correction``, cached per x);
batched variants for many x_o.
"""

from __future__ import annotations

import warnings
from typing import Optional, Union

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.inference.potentials.posterior_based_potential import posterior_estimator_based_potential
from sbi_amd.neural_nets.estimators.base import ConditionalDensityEstimator
from sbi_amd.neural_nets.estimators.shape_handling import reshape_to_batch_event, reshape_to_sample_batch_event
from sbi_amd.samplers.rejection import rejection
from sbi_amd.utils.sbiutils import warn_if_outside_prior_support, within_support
from sbi_amd.utils.torchutils import ensure_theta_batched, process_device


class DirectPosterior:
    def __init__(self, posterior_estimator: ConditionalDensityEstimator, prior: Distribution,
                 max_sampling_batch_size: int = 10_000, device: Optional[Union[str, torch.device]] = None,
                 x_shape: Optional[torch.Size] = None, enable_transform: bool = True,
                 check_finite_x: bool = True, allow_nan_x: bool = False):
        self.posterior_estimator = posterior_estimator
        self.prior = prior
        self.max_sampling_batch_size = max_sampling_batch_size
        self.enable_transform = enable_transform
        self._check_finite_x = check_finite_x
        # missing iid trials of x_o are NaN by design behind a PermutationInvariantEmbedding (Inf is still refused)
        self._allow_nan_x = allow_nan_x
        if device is None:
            device = str(next(posterior_estimator.parameters()).device)
        self._device = process_device(device)
        self.posterior_estimator.to(self._device)
        self.potential_fn, self.theta_transform = posterior_estimator_based_potential(
            posterior_estimator, prior, x_o=None, enable_transform=enable_transform)
        self._x: Optional[Tensor] = None
        self._x_shape = x_shape
        self._leakage_density_correction_factor = None
        self._leakage_x = None
        self._purpose = "It samples the posterior network and rejects samples that lie outside of the prior bounds."

    # -- x handling ---------------------------------------------------------------------
    _allow_nan_x = False      # (subclasses and copies made before the argument existed)

    def _x_is_acceptable(self, x: Tensor) -> bool:
        if self._allow_nan_x:
            return not torch.isinf(x).any()
        return bool(torch.isfinite(x).all())

    @property
    def default_x(self) -> Optional[Tensor]:
        return self._x

    def set_default_x(self, x: Tensor) -> "DirectPosterior":
        x = torch.as_tensor(x, dtype=torch.float32)
        if self._check_finite_x and not self._x_is_acceptable(x):
            raise ValueError("x_o contains NaN or Inf values.")
        x = reshape_to_batch_event(x, self.posterior_estimator.condition_shape) if x.dim() <= len(
            self.posterior_estimator.condition_shape) + 1 else x
        self._x = x.to(self._device)
        return self

    def _x_else_default_x(self, x: Optional[Tensor]) -> Tensor:
        if x is not None:
            x = torch.as_tensor(x, dtype=torch.float32)
            # the finiteness check reads the tensor back (a device round trip in front of every call): the same tensor
            # object at the same version was checked before and has not been written since
            seen = self.__dict__.get("_finite_x_seen")
            if self._check_finite_x and not (seen is not None and seen[0] is x and seen[1] == x._version):
                if not self._x_is_acceptable(x):
                    raise ValueError("x_o contains NaN or Inf values.")
                self._finite_x_seen = (x, x._version)
            return x.to(self._device)
        if self._x is None:
            raise ValueError(
                "Context `x` needed when a default has not been set. If you'd like to have a default, use the "
                "`.set_default_x()` method."
            )
        return self._x

    def to(self, device: Union[str, torch.device]) -> "DirectPosterior":
        self._device = process_device(device)
        self.posterior_estimator.to(self._device)
        if hasattr(self.prior, "to"):
            self.prior = self.prior.to(self._device)
        self.potential_fn.to(self._device)
        if self._x is not None:
            self._x = self._x.to(self._device)
        self._leakage_density_correction_factor = None
        return self

    # -- what is sampled and evaluated (NPE_A_Posterior puts the corrected mixture here) --
    def _candidate_sampler(self):
        """`f(sample_shape, condition=x) -> (*sample_shape, B, D)`: the draws that are then tested against the prior."""
        return self.posterior_estimator.sample

    def _estimator_log_prob(self, theta: Tensor, x: Tensor) -> Tensor:
        """(S, B, D), (B, ...) -> (S, B): the density before the support mask and the leakage correction."""
        return self.posterior_estimator.log_prob(theta, condition=x)

    # -- sampling -----------------------------------------------------------------------
    def _batch_cap(self, requested: Optional[int]) -> int:
        return self.max_sampling_batch_size if requested is None else requested

    def _draw(self, how_many: int, x: Tensor, batch_cap: int, show_progress_bars: bool, reject_outside_prior: bool,
              max_sampling_time: Optional[float], return_partial_on_timeout: bool) -> Tensor:
        """(<= how_many, B, D) draws for the B condition rows of `x`: candidates from the estimator (one launch of the
        sampling kernel per proposal batch, x never expanded), kept when inside the prior support
        (direct_posterior.py:177-213 -> rejection.py:230-457); without rejection the raw draws."""
        est = self.posterior_estimator
        if not reject_outside_prior:
            return self._candidate_sampler()(torch.Size([how_many]), condition=x)
        def inside_prior(candidates: Tensor) -> Tensor:
            return within_support(self.prior, candidates)

        # a box prior's support check is lo <= theta <= hi on every coordinate: the compaction kernel evaluates it on
        # the candidates as it reads them (no mask tensor, no separate launches)
        from sbi_amd.utils.torchutils import BoxUniform

        if isinstance(self.prior, BoxUniform) and self.prior.low.ndim == 1:
            inside_prior.box_bounds = (self.prior.low.to(torch.float32).contiguous(),
                                       self.prior.high.to(torch.float32).contiguous())
        else:
            # an unbounded prior (Gaussian, ...): torch's `real` support check is `value == value` on every coordinate --
            # exactly the box (-inf, +inf), which only a NaN fails
            from torch.distributions import constraints

            sup = getattr(self.prior, "support", None)
            if getattr(sup, "base_constraint", sup) is constraints.real and getattr(sup, "reinterpreted_batch_ndims", 1) == 1:
                d_ev = int(est.input_shape[-1]) if len(getattr(est, "input_shape", ())) == 1 else None
                if d_ev is not None:
                    cached = self.__dict__.get("_real_box")
                    if cached is None or cached[0].numel() != d_ev or cached[0].device != x.device:
                        cached = self._real_box = (torch.full((d_ev,), float("-inf"), device=x.device),
                                                   torch.full((d_ev,), float("inf"), device=x.device))
                    inside_prior.box_bounds = cached
        kept, _acceptance = rejection.accept_reject_sample(
            self._candidate_sampler(), inside_prior, how_many,
            show_progress_bars=show_progress_bars, max_sampling_batch_size=batch_cap,
            proposal_sampling_kwargs=dict(condition=x), alternative_method="build_posterior(..., sample_with='mcmc')",
            max_sampling_time=max_sampling_time, return_partial_on_timeout=return_partial_on_timeout,
            acceptance_on_device=False)       # (not used here: spares the host-to-device copy of one float per call)
        return kept

    def sample(self, sample_shape=torch.Size(), x: Optional[Tensor] = None, max_sampling_batch_size: int = 10_000,
               show_progress_bars: bool = True, reject_outside_prior: bool = True,
               max_sampling_time: Optional[float] = None, return_partial_on_timeout: bool = False) -> Tensor:
        shape = torch.Size(sample_shape)
        x_o = reshape_to_batch_event(self._x_else_default_x(x), event_shape=self.posterior_estimator.condition_shape)
        if len(x_o) != 1:
            raise ValueError(
                ".sample() supports only `batchsize == 1`. If you intend to sample multiple observations, use "
                "`.sample_batched()`. If you intend to sample i.i.d. observations, set up the posterior density "
                "estimator with an appropriate permutation invariant embedding net.")
        drawn = self._draw(shape.numel(), x_o, self._batch_cap(max_sampling_batch_size), show_progress_bars,
                           reject_outside_prior, max_sampling_time, return_partial_on_timeout)[:, 0]
        if not reject_outside_prior:
            warn_if_outside_prior_support(self.prior, drawn)
        # (a timeout may hand back fewer rows than asked for: those stay a flat batch)
        return drawn.reshape(*shape, *drawn.shape[1:]) if len(drawn) == shape.numel() else drawn

    def sample_batched(self, sample_shape, x: Tensor, max_sampling_batch_size: int = 10_000,
                       show_progress_bars: bool = True, reject_outside_prior: bool = True,
                       max_sampling_time: Optional[float] = None, return_partial_on_timeout: bool = False) -> Tensor:
        shape = torch.Size(sample_shape)
        xs = reshape_to_batch_event(self._x_else_default_x(x), self.posterior_estimator.condition_shape)
        n_obs, per_obs = len(xs), shape.numel()
        if n_obs * per_obs > 2**21:
            warnings.warn(f"Note that for batched sampling, the direct posterior sampling generates {n_obs} * {per_obs} = "
                          f"{n_obs * per_obs} samples. This can be slow and memory-intensive.", stacklevel=2)
        cap = self._batch_cap(max_sampling_batch_size)
        if cap * n_obs > 100_000:        # candidates are drawn for every observation at once
            smaller = max(1, 100_000 // n_obs)
            warnings.warn(f"Capping max_sampling_batch_size from {cap} to {smaller} to avoid excessive memory usage.",
                          stacklevel=2)
            cap = smaller
        drawn = self._draw(per_obs, xs, cap, show_progress_bars, reject_outside_prior, max_sampling_time,
                           return_partial_on_timeout)
        return drawn.reshape(*shape, n_obs, *drawn.shape[2:])

    # -- density ------------------------------------------------------------------------
    def log_prob(self, theta: Tensor, x: Optional[Tensor] = None, norm_posterior: bool = True,
                 track_gradients: bool = False,
                 leakage_correction_params: Optional[dict] = None) -> Tensor:
        x = self._x_else_default_x(x)
        theta = ensure_theta_batched(torch.as_tensor(theta)).to(self._device)
        est = self.posterior_estimator
        theta_sbe = reshape_to_sample_batch_event(theta, event_shape=theta.shape[1:], leading_is_sample=True)
        x_be = reshape_to_batch_event(x, event_shape=est.condition_shape)
        if x_be.shape[0] > 1:
            raise ValueError(".log_prob() supports only `batchsize == 1`. Use `.log_prob_batched()` for many "
                             "observations.")
        with torch.set_grad_enabled(track_gradients):
            unnorm = self._estimator_log_prob(theta_sbe, x_be).squeeze(1)
            in_support = within_support(self.prior, theta)
            masked = torch.where(in_support, unnorm,
                                 torch.tensor(float("-inf"), dtype=torch.float32, device=self._device))
            if leakage_correction_params is None:
                leakage_correction_params = {}
            log_factor = (torch.log(self.leakage_correction(x=x, **leakage_correction_params))
                          if norm_posterior else 0)
            return masked - log_factor

    def log_prob_batched(self, theta: Tensor, x: Tensor, norm_posterior: bool = True, track_gradients: bool = False,
                         leakage_correction_params: Optional[dict] = None) -> Tensor:
        """theta (S, B, D) (or (B,D)), x (B, C) -> (S, B)."""
        est = self.posterior_estimator
        theta = torch.as_tensor(theta).to(self._device)
        theta = reshape_to_sample_batch_event(theta, event_shape=est.input_shape, leading_is_sample=True) \
            if theta.dim() == len(est.input_shape) + 2 else theta.unsqueeze(0)
        x = reshape_to_batch_event(self._x_else_default_x(x), event_shape=est.condition_shape)
        with torch.set_grad_enabled(track_gradients):
            unnorm = self._estimator_log_prob(theta, x)
            in_support = within_support(self.prior, theta)
            masked = torch.where(in_support, unnorm,
                                 torch.tensor(float("-inf"), dtype=torch.float32, device=self._device))
            if leakage_correction_params is None:
                leakage_correction_params = {}
            log_factor = (torch.log(self.leakage_correction(x=x, **leakage_correction_params))
                          if norm_posterior else 0)
            return masked - log_factor

    @torch.no_grad()
    def leakage_correction(self, x: Tensor, num_rejection_samples: int = 10_000, force_update: bool = False,
                           show_progress_bars: bool = False, rejection_sampling_batch_size: int = 10_000) -> Tensor:
        """Acceptance probability of estimator draws under the prior support, estimated by
        rejection sampling once per x and cached (direct_posterior.py:466-523)."""
        x = reshape_to_batch_event(x, self.posterior_estimator.condition_shape)

        def acceptance_at(x_: Tensor) -> Tensor:
            return rejection.accept_reject_sample(
                proposal=self._candidate_sampler(),
                accept_reject_fn=lambda theta: within_support(self.prior, theta),
                num_samples=num_rejection_samples, show_progress_bars=show_progress_bars,
                sample_for_correction_factor=True, max_sampling_batch_size=rejection_sampling_batch_size,
                proposal_sampling_kwargs={"condition": x_},
            )[1]

        is_new_x = self._leakage_x is None or self._leakage_x.shape != x.shape or not torch.equal(self._leakage_x, x)
        if self._leakage_density_correction_factor is None or is_new_x or force_update:
            self._leakage_density_correction_factor = acceptance_at(x).to(self._device)
            self._leakage_x = x.clone()
        return self._leakage_density_correction_factor

    def potential(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False) -> Tensor:
        self.potential_fn.set_x(self._x_else_default_x(x))
        return self.potential_fn(ensure_theta_batched(torch.as_tensor(theta)).to(self._device),
                                 track_gradients=track_gradients)

    def map(self, x: Optional[Tensor] = None, num_iter: int = 1_000, num_to_optimize: int = 100,
            learning_rate: float = 0.01, num_init_samples: int = 1_000, show_progress_bars: bool = False) -> Tensor:
        """Maximum-a-posteriori estimate by Adam ascent on the potential from the best of
        ``num_init_samples`` posterior draws (base_posterior.py:216-323; sbiutils.py:1160-1286).
        Needs d log_prob / d theta, which the fused backward kernel provides."""
        x = self._x_else_default_x(x)
        self.potential_fn.set_x(x)
        inits = self.sample((num_init_samples,), x=x, show_progress_bars=False)
        with torch.no_grad():
            p0 = self.potential_fn(inits, track_gradients=False)
        top = inits[torch.topk(p0, min(num_to_optimize, num_init_samples)).indices].clone().requires_grad_(True)
        opt = torch.optim.Adam([top], lr=learning_rate)
        best, best_val = top.detach()[0].clone(), torch.tensor(float("-inf"), device=top.device)
        for _ in range(num_iter):
            opt.zero_grad()
            pot = self.potential_fn(top, track_gradients=True)
            finite = torch.isfinite(pot)
            (-(pot[finite]).sum()).backward()
            opt.step()
            with torch.no_grad():
                v, i = torch.max(torch.where(finite, pot, torch.full_like(pot, float("-inf"))), dim=0)
                if v > best_val:
                    best_val, best = v.clone(), top.detach()[i].clone()
        self._map = best
        return best
