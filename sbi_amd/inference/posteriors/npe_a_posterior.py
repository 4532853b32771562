"""``NPE_A_Posterior`` -- the NPE-A posterior: the MDN's mixture corrected in closed form for the proposal.

Mirror of sbi/inference/posteriors/npe_a_posterior.py:  p(theta | x) ~ q(theta | x) prior(theta) / proposal(theta)
with every factor a mixture of Gaussians (in the estimator's z-scored theta space), so the posterior is again a
mixture with L K components.  A first-round posterior (no proposal) behaves as a ``DirectPosterior``.  Sampling
rejects draws outside the prior support through ``accept_reject_sample``; ``log_prob`` is -inf outside the support and
divided by the acceptance rate (``leakage_correction``), both on the corrected mixture.

Deliberate departure from the reference: ``sample_batched`` / ``log_prob_batched`` apply the correction per
observation (B density rows against the one proposal in a single ``sbi_amd_mog_correct`` call, then one mixture per
row).  The reference inherits ``DirectPosterior``'s versions, which silently skip the correction; with it ``run_sbc``,
``run_tarp`` and ``LC2ST`` see the posterior that ``sample`` draws from.

``map()`` on a corrected posterior raises ``NotImplementedError`` (the corrected mixture has no theta-gradient path).
"""

from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.inference.posteriors.direct_posterior import DirectPosterior
from sbi_amd.neural_nets.estimators import mog_ops
from sbi_amd.neural_nets.estimators.mdn import MixtureDensityEstimator, MoG


class NPE_A_Posterior(DirectPosterior):
    def __init__(self, posterior_estimator: MixtureDensityEstimator, prior: Distribution,
                 proposal_mog: Optional[MoG] = None, prior_mog: Optional[MoG] = None,
                 max_sampling_batch_size: int = 10_000, device: Optional[Union[str, torch.device]] = None,
                 enable_transform: bool = True):
        """proposal_mog: the previous round's posterior at x_o as a mixture (None in the first round: no correction);
        prior_mog: the prior as a one-component mixture in z-scored space (None for a uniform prior)."""
        super().__init__(posterior_estimator=posterior_estimator, prior=prior,
                         max_sampling_batch_size=max_sampling_batch_size, device=device,
                         enable_transform=enable_transform)
        self._proposal_mog = proposal_mog.to(self._device).detach() if proposal_mog is not None else None
        self._prior_mog = prior_mog.to(self._device).detach() if prior_mog is not None else None
        self._apply_correction = proposal_mog is not None

    def to(self, device) -> "NPE_A_Posterior":
        super().to(device)
        if self._proposal_mog is not None:
            self._proposal_mog = self._proposal_mog.to(self._device)
        if self._prior_mog is not None:
            self._prior_mog = self._prior_mog.to(self._device)
        return self

    # -- the corrected mixture ------------------------------------------------------------------------------
    def get_mog_params(self, x: Tensor) -> MoG:
        """The (corrected, from the second round on) mixture of every row of x (B, ...), in z-scored theta space: what
        the next round uses as its proposal."""
        return self._get_corrected_mog(x)

    def _get_corrected_mog(self, x: Tensor) -> MoG:
        density_mog = self.posterior_estimator.get_uncorrected_mog(x)
        if not self._apply_correction:
            return density_mog
        return mog_ops.correct_for_proposal(density_mog, self._proposal_mog, self._prior_mog)

    def _z_score(self, like: Tensor):
        """(shift, scale) of the estimator's theta z-scoring on `like`'s device."""
        net = self.posterior_estimator.net
        D = net.hyper.D
        z = net.zstats.detach().to(like.device)
        return z[:D].contiguous(), z[D : 2 * D].contiguous()

    def _corrected_sample(self, sample_shape: torch.Size, condition: Tensor) -> Tensor:
        """(*sample_shape, B, D) draws of the corrected mixtures of the B rows of `condition`."""
        shape = torch.Size(sample_shape)
        mog = self._get_corrected_mog(condition)
        B, D, n = mog.logits.shape[0], mog.dim, shape.numel()
        u = torch.rand(n * B, device=mog.device, dtype=mog.dtype)
        zeta = torch.randn(n * B, D, device=mog.device, dtype=mog.dtype)
        shift, scale = self._z_score(zeta)
        out = mog_ops.mog_sample(mog.logits, mog.means, mog.precision_factors, zeta, u=u, shift=shift, scale=scale)
        return out.reshape(*shape, B, D)

    def _corrected_log_prob(self, theta: Tensor, condition: Tensor) -> Tensor:
        """(S, B, D), (B, ...) -> (S, B), the z-score Jacobian included."""
        mog = self._get_corrected_mog(condition)
        S, B, D = theta.shape
        theta = theta.to(mog.device, mog.dtype)
        shift, scale = self._z_score(theta)
        return mog_ops.mog_log_prob(mog.logits, mog.means, mog.precisions, mog.precision_factors,
                                    theta.reshape(S * B, D), shift=shift, scale=scale).reshape(S, B)

    # -- DirectPosterior's hooks ---------------------------------------------------------------------------
    def _candidate_sampler(self):
        return self._corrected_sample if self._apply_correction else super()._candidate_sampler()

    def _estimator_log_prob(self, theta: Tensor, x: Tensor) -> Tensor:
        if not self._apply_correction:
            return super()._estimator_log_prob(theta, x)
        if theta.requires_grad:
            raise NotImplementedError("sbi_amd: the corrected NPE-A mixture has no gradient with respect to theta")
        return self._corrected_log_prob(theta, x)

    def map(self, *args, **kwargs) -> Tensor:
        if self._apply_correction:
            raise NotImplementedError("sbi_amd: map() on a corrected NPE-A posterior is not implemented (no "
                                      "theta-gradient of the corrected mixture); a first-round posterior has it")
        return super().map(*args, **kwargs)
