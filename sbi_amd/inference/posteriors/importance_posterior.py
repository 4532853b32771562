"""``ImportanceSamplingPosterior`` -- importance sampling and SIR over a potential and a proposal.

Mirror of sbi/inference/posteriors/importance_posterior.py:18-380 (constructor, attributes, ``sample`` with its two
methods, the importance-sampled normalisation constant behind a NORMALISED ``log_prob``, ``map``, ``to``).  The
candidates, the potential and the proposal's log-density are the kernels of whatever estimator sits underneath; the
selection step of SIR is one launch of ``sbi_amd_sir_resample`` (samplers/importance/sir.py).

Beyond the reference: ``sample_batched`` works -- every (observation, draw) pair is a row of one SIR pass, with the
potential evaluated pairwise (``set_x(x_repeated, x_is_iid=False)``) -- so ``run_sbc`` / ``run_tarp`` take this
posterior without their per-observation loop.  ``estimate_normalization_constant`` is
``exp(logsumexp(lw) - log N)``: where the reference's ``mean(exp(lw))`` is finite the two agree to rounding, and
this one does not overflow.
"""

from __future__ import annotations

import math
from functools import partial
from typing import Any, Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from sbi_amd.samplers.importance.importance_sampling import importance_sample
from sbi_amd.samplers.importance.sir import live_first, sampling_importance_resampling, sir_select
from sbi_amd.utils.sbiutils import gradient_ascent, mcmc_transform
from sbi_amd.utils.torchutils import ensure_theta_batched, process_device


def _takes_paired_x(potential_fn) -> bool:
    """The potentials whose `set_x(x, x_is_iid=False)` pairs row i of theta with row i of x."""
    from sbi_amd.inference.potentials.likelihood_based_potential import LikelihoodBasedPotential
    from sbi_amd.inference.potentials.posterior_based_potential import PosteriorBasedPotential
    from sbi_amd.inference.potentials.ratio_based_potential import RatioBasedPotential

    return isinstance(potential_fn, (LikelihoodBasedPotential, RatioBasedPotential, PosteriorBasedPotential))


class ImportanceSamplingPosterior:
    def __init__(self, potential_fn: Callable, proposal: Any, theta_transform=None, method: str = "sir",
                 oversampling_factor: int = 32, max_sampling_batch_size: int = 10_000,
                 device: Optional[Union[str, torch.device]] = None, x_shape: Optional[torch.Size] = None):
        if not callable(potential_fn):
            raise TypeError("potential_fn must be a callable potential (BasePotential / CustomPotential role).")
        self.potential_fn = potential_fn
        if device is None:
            device = getattr(potential_fn, "device", "cpu")
        self._device = process_device(device)
        self.proposal = proposal
        self._normalization_constant: Optional[Tensor] = None
        self.method = method
        self.theta_transform = theta_transform
        self.oversampling_factor = oversampling_factor
        self.max_sampling_batch_size = max_sampling_batch_size
        self.x_shape = x_shape
        self._x: Optional[Tensor] = None
        self._map: Optional[Tensor] = None
        self._purpose = ("It provides sampling-importance resampling (SIR) to .sample() from the posterior and can "
                         "evaluate the _unnormalized_ posterior density with .log_prob().")

    # -- x_o handling (base_posterior.py:170-214) ------------------------------------------------------
    @property
    def default_x(self) -> Optional[Tensor]:
        return self._x

    def set_default_x(self, x: Tensor) -> "ImportanceSamplingPosterior":
        x = torch.as_tensor(x, dtype=torch.float32)
        if not torch.isfinite(x).all():
            raise ValueError("x_o contains NaN or Inf values.")
        self._x = x.reshape(1, -1).to(self._device) if x.dim() <= 1 else x.to(self._device)
        self._map = None
        self._normalization_constant = None
        return self

    def _x_else_default_x(self, x: Optional[Tensor]) -> Tensor:
        if x is not None:
            x = torch.as_tensor(x, dtype=torch.float32)
            return (x.reshape(1, -1) if x.dim() <= 1 else x).to(self._device)
        if self._x is None:
            raise ValueError("Context `x` needed when a default has not been set. If you'd like to have a default, "
                             "use the `.set_default_x()` method.")
        return self._x

    def to(self, device: Union[str, torch.device]) -> None:
        """Move the potential, the proposal and x_o; the transform is rebuilt from the proposal on the new device."""
        device = process_device(device)
        self._device = device
        self.potential_fn.to(device)
        if hasattr(self.proposal, "to"):
            self.proposal = self.proposal.to(device) or self.proposal
        self.theta_transform = mcmc_transform(self.proposal, device=device)
        if self._x is not None:
            self._x = self._x.to(device)
        if self._normalization_constant is not None:
            self._normalization_constant = self._normalization_constant.to(device)

    # -- evaluation ---------------------------------------------------------------------------------------
    def potential(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False) -> Tensor:
        self.potential_fn.set_x(self._x_else_default_x(x))
        theta = ensure_theta_batched(torch.as_tensor(theta))
        return self.potential_fn(theta.to(self._device), track_gradients=track_gradients)

    def log_prob(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False,
                 normalization_constant_params: Optional[dict] = None) -> Tensor:
        """The NORMALISED posterior log-density: potential - log Z, Z estimated by importance sampling."""
        x = self._x_else_default_x(x)
        self.potential_fn.set_x(x)
        theta = ensure_theta_batched(torch.as_tensor(theta))
        with torch.set_grad_enabled(track_gradients):
            potential_values = self.potential_fn(theta.to(self._device), track_gradients=track_gradients)
            constant = self.estimate_normalization_constant(x, **(normalization_constant_params or {}))
            return (potential_values - torch.log(constant).to(potential_values.device)).to(self._device)

    @torch.no_grad()
    def estimate_normalization_constant(self, x: Tensor, num_samples: int = 10_000,
                                        force_update: bool = False) -> Tensor:
        """Z = mean of the importance weights, as exp(logsumexp(lw) - log N).  Cached at the default x only."""
        default = self.default_x
        is_new_x = default is None or (x is not default and (
            tuple(torch.as_tensor(x).shape) != tuple(default.shape)
            or bool((torch.as_tensor(x).to(default.device) != default).any())))

        def estimate() -> Tensor:
            self.potential_fn.set_x(self._x_else_default_x(x))      # (the weights are those of THIS x)
            _, lw = importance_sample(self.potential_fn, proposal=self.proposal, num_samples=num_samples)
            return torch.exp(torch.logsumexp(lw.reshape(-1), dim=0) - math.log(num_samples))

        if is_new_x:                   # at this x only: nothing is kept
            return estimate().to(self._device)
        if self._normalization_constant is None or force_update:
            self._normalization_constant = estimate()
        return self._normalization_constant.to(self._device)

    # -- sampling -----------------------------------------------------------------------------------------
    def sample(self, sample_shape=torch.Size(), x: Optional[Tensor] = None, method: Optional[str] = None,
               oversampling_factor: int = 32, max_sampling_batch_size: int = 10_000,
               show_progress_bars: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """`method="sir"`: samples; `method="importance"`: (proposal samples, log importance weights)."""
        method = self.method if method is None else method
        self.potential_fn.set_x(self._x_else_default_x(x))
        if method == "sir":
            return self._sir_sample(sample_shape, oversampling_factor=oversampling_factor,
                                    max_sampling_batch_size=max_sampling_batch_size,
                                    show_progress_bars=show_progress_bars)
        if method == "importance":
            return self._importance_sample(sample_shape)
        raise NameError

    def _importance_sample(self, sample_shape=torch.Size(), show_progress_bars: bool = False) -> Tuple[Tensor, Tensor]:
        shape = torch.Size(sample_shape)
        samples, log_weights = importance_sample(self.potential_fn, proposal=self.proposal, num_samples=shape.numel(),
                                                 show_progress_bars=show_progress_bars)
        return samples.reshape((*shape, -1)).to(self._device), log_weights.to(self._device)

    def _sir_sample(self, sample_shape=torch.Size(), oversampling_factor: Optional[int] = 32,
                    max_sampling_batch_size: Optional[int] = 10_000, show_progress_bars: bool = False) -> Tensor:
        if oversampling_factor is None:
            oversampling_factor = self.oversampling_factor
        if max_sampling_batch_size is None:
            max_sampling_batch_size = self.max_sampling_batch_size
        shape = torch.Size(sample_shape)
        samples = sampling_importance_resampling(
            self.potential_fn, proposal=self.proposal, num_samples=shape.numel(),
            num_candidate_samples=oversampling_factor, show_progress_bars=show_progress_bars,
            max_sampling_batch_size=max_sampling_batch_size, device=self._device)
        return samples.reshape((*shape, -1)).to(self._device)

    @torch.no_grad()
    def sample_batched(self, sample_shape, x: Tensor, max_sampling_batch_size: int = 10_000,
                       show_progress_bars: bool = True, oversampling_factor: Optional[int] = None) -> Tensor:
        """SIR draws of p(theta | x_b) for every row of `x`, shape (*sample_shape, B, D).  (The reference raises here.)
        Row s * B + b of a pass is draw s of observation b; its `oversampling_factor` candidates are weighted by the
        potential at x_b (one paired evaluation of all candidates of the pass) over the proposal.  At most
        `max_sampling_batch_size` rows per pass; rows without a normalisable weight are drawn again.  Potentials
        that do not pair theta rows with x rows raise NotImplementedError, which `get_posterior_samples_on_batch`
        turns into its per-observation loop."""
        if not _takes_paired_x(self.potential_fn):
            raise NotImplementedError(
                "Batched sampling of an ImportanceSamplingPosterior needs a potential that pairs theta rows with x "
                "rows (`set_x(x, x_is_iid=False)`: the likelihood-, ratio- and posterior-based potentials). "
                "Alternatively you can use `sample` in a loop [posterior.sample(theta, x_o) for x_o in x].")
        K = self.oversampling_factor if oversampling_factor is None else oversampling_factor
        shape = torch.Size(sample_shape)
        x = torch.as_tensor(x, dtype=torch.float32).to(self._device)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        num_x, n = x.shape[0], shape.numel()
        if num_x == 0 or n == 0:
            raise ValueError("sample_batched needs at least one observation and one sample per observation.")
        total = n * num_x
        pending = torch.arange(total, device=self._device)            # rows still to draw; observation = row % num_x
        out: Optional[Tensor] = None
        seed: Optional[int] = None
        row_offset = 0
        while pending.numel() > 0:
            rows = pending[:max_sampling_batch_size]
            R = rows.numel()
            try:
                theta = self.proposal.sample((R * K,), show_progress_bar=False)
            except TypeError:
                theta = self.proposal.sample((R * K,))
            theta = theta.reshape(R * K, -1).to(self._device)
            self.potential_fn.set_x(x[rows % num_x].repeat_interleave(K, dim=0), x_is_iid=False)
            log_weights = (self.potential_fn(theta) - self.proposal.log_prob(theta)).reshape(R, K)
            cand = theta.reshape(R, K, -1)
            if seed is None and log_weights.is_cuda:
                seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
            winners, idx, n_dead = sir_select(log_weights, None, cand, None, seed or 0, row_offset)
            row_offset += R
            dead = int(n_dead.item())                                # the ONE host read of the pass
            if out is None:
                out = torch.empty((total, winners.shape[-1]), dtype=winners.dtype, device=winners.device)
            rows = rows.to(winners.device)
            rest = pending[max_sampling_batch_size:]
            if dead > 0:
                live_pos, dead_pos = live_first(idx, dead)           # (known sizes: no second synchronisation)
                out[rows[live_pos]] = winners[live_pos]
                pending = torch.cat([rows[dead_pos].to(pending.device), rest])
            else:
                out[rows] = winners
                pending = rest
        assert out is not None
        return out.reshape((*shape, num_x, -1)).to(self._device)

    def map(self, x: Optional[Tensor] = None, num_iter: int = 1_000, num_to_optimize: int = 100,
            learning_rate: float = 0.01, init_method: Union[str, Tensor] = "proposal", num_init_samples: int = 1_000,
            save_best_every: int = 10, show_progress_bars: bool = False, force_update: bool = False) -> Tensor:
        """base_posterior.py:216-323: gradient ascent on the potential from proposal (or posterior) draws."""
        if x is None and self._map is not None and not force_update:
            return self._map
        self.potential_fn.set_x(self._x_else_default_x(x))
        if isinstance(init_method, Tensor):
            starts = init_method
        elif init_method in ("proposal", "posterior"):
            starts = (self.proposal.sample((num_init_samples,)) if init_method == "proposal"
                      else self.sample((num_init_samples,), x=x, show_progress_bars=False))
        else:
            raise ValueError("init_method must be 'posterior', 'proposal' or a tensor of initial parameters.")
        best, _ = gradient_ascent(partial(self.potential_fn, track_gradients=True), starts.to(self._device),
                                  self.theta_transform, num_iter, num_to_optimize, learning_rate, save_best_every,
                                  show_progress_bars)
        self._map = best
        return best
