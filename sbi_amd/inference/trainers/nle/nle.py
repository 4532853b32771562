"""Neural Likelihood Estimation on the NSF kernels.

API mirror of sbi's ``NLE`` (= ``NLE_A``, sbi/inference/trainers/nle/nle_base.py): the same estimator and training loop
as NPE with the roles swapped -- the flow models q(x | theta), x is its input and theta its condition -- so training is
NPE's device-resident loop and ``FusedTrainStep`` on the pairs (x, theta).  Later rounds train on every round's data
with the plain likelihood loss (no proposal correction); ``discard_prior_samples`` drops round 0.  The posterior is
sampled by MCMC (or rejection) on the potential sum_i log q(x_i | theta) + log p(theta) over the iid trials of x_o
(``LikelihoodBasedPotential``: one trials-kernel pass per evaluation).
"""

from __future__ import annotations

import warnings
from copy import deepcopy
from typing import Any, Callable, Dict, Optional, Tuple, Union

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.inference.trainers.npe.npe import (ImproperEmpirical, PosteriorEstimatorTrainer, check_estimator_arg,
                                                validate_theta_and_x)
from sbi_amd.neural_nets.estimators.base import ConditionalDensityEstimator
from sbi_amd.neural_nets.factory import likelihood_nn
from sbi_amd.neural_nets.net_builders.estimator_configs import MAFConfig, NSFConfig, ZukoNSFConfig
from sbi_amd.utils.sbiutils import handle_invalid_x, mcmc_transform, warn_on_invalid_x
from sbi_amd.utils.torchutils import check_if_prior_on_device


class NLE_A(PosteriorEstimatorTrainer):
    def __init__(self, prior: Optional[Distribution] = None,
                 density_estimator: Union[str, NSFConfig, Callable, None] = None, device: str = "cpu",
                 logging_level: Union[int, str] = "WARNING", summary_writer=None, tracker=None,
                 show_progress_bars: bool = True):
        if density_estimator is None:
            raise NotImplementedError(
                "NLE's default likelihood estimator is sbi's affine MAF, which sbi_amd does not implement. Pass "
                "density_estimator='nsf' or density_estimator=likelihood_nn('nsf', ...)."
            )
        check_estimator_arg(density_estimator)
        if isinstance(density_estimator, ZukoNSFConfig):
            raise NotImplementedError("The zuko flows are not available as likelihood estimators here; pass "
                                      "density_estimator='nsf' or likelihood_nn('nsf', ...).")
        super().__init__(prior=prior, density_estimator=NSFConfig(), device=device, logging_level=logging_level,
                         summary_writer=summary_writer, tracker=tracker, show_progress_bars=show_progress_bars)
        # every builder is called as build(batch_theta, batch_x) and returns q(x | theta) (nle_base.py:413-444)
        if isinstance(density_estimator, str):
            self._build_neural_net = likelihood_nn(model=density_estimator)
        elif isinstance(density_estimator, (NSFConfig, MAFConfig)):
            cfg = density_estimator
            self._build_neural_net = lambda batch_theta, batch_x: cfg.build(batch_x, batch_theta)
        else:
            self._build_neural_net = density_estimator

    def _input_condition(self, theta: Tensor, x: Tensor) -> Tuple[Tensor, Tensor]:
        return x, theta

    def append_simulations(self, theta: Tensor, x: Tensor, exclude_invalid_x: bool = False, from_round: int = 0,
                           data_device: Optional[str] = None) -> "NLE_A":
        """nle_base.py:138-188 / base.py:343-404: invalid x are kept unless `exclude_invalid_x`; `from_round` tags the
        data (round 0 = drawn from the prior, which `train(discard_prior_samples=True)` drops in later rounds)."""
        if data_device is None:
            data_device = self._device
        theta, x = validate_theta_and_x(theta, x, data_device=data_device, training_device=self._device)
        is_valid_x, num_nans, num_infs = handle_invalid_x(x, exclude_invalid_x=exclude_invalid_x)
        x, theta = x[is_valid_x], theta[is_valid_x]
        warn_on_invalid_x(num_nans, num_infs, exclude_invalid_x)
        self._data_round_index.append(int(from_round))
        self._theta_roundwise.append(theta)
        self._x_roundwise.append(x)
        self._prior_masks.append(torch.full((theta.shape[0], 1), int(from_round) == 0, dtype=torch.bool))
        self._proposal_roundwise.append(None)
        if self._prior is None or isinstance(self._prior, ImproperEmpirical):
            self._prior = ImproperEmpirical(self.get_simulations()[0].to(self._device))
        return self

    def train(self, training_batch_size: int = 200, learning_rate: float = 5e-4, validation_fraction: float = 0.1,
              stop_after_epochs: int = 20, max_num_epochs: int = 2**31 - 1, clip_max_norm: Optional[float] = 5.0,
              resume_training: bool = False, discard_prior_samples: bool = False, retrain_from_scratch: bool = False,
              show_train_summary: bool = False, dataloader_kwargs: Optional[dict] = None) -> ConditionalDensityEstimator:
        """nle_base.py:190-272: maximum likelihood of x given theta on all rounds (no proposal correction)."""
        return super().train(training_batch_size=training_batch_size, learning_rate=learning_rate,
                             validation_fraction=validation_fraction, stop_after_epochs=stop_after_epochs,
                             max_num_epochs=max_num_epochs, clip_max_norm=clip_max_norm,
                             resume_training=resume_training, force_first_round_loss=True,
                             discard_prior_samples=discard_prior_samples, retrain_from_scratch=retrain_from_scratch,
                             show_train_summary=show_train_summary, dataloader_kwargs=dataloader_kwargs)

    def build_posterior(self, density_estimator: Optional[ConditionalDensityEstimator] = None,
                        prior: Optional[Distribution] = None, sample_with: str = "mcmc",
                        mcmc_method: str = "slice_np_vectorized", mcmc_parameters: Optional[Dict[str, Any]] = None,
                        rejection_sampling_parameters: Optional[Dict[str, Any]] = None, **kwargs):
        """nle_base.py:274-354: MCMC (default) or rejection sampling on the likelihood-based potential."""
        if sample_with not in ("mcmc", "rejection"):
            raise NotImplementedError(
                f"sample_with={sample_with!r}: VI / importance posteriors are outside the accelerated path; NLE "
                "samples with 'mcmc' or 'rejection'."
            )
        from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential

        if prior is None:
            if self._prior is None:
                raise ValueError("You did not pass a prior. You have to pass the prior either at initialization "
                                 "`inference = NLE(prior)` or to `.build_posterior(prior=prior)`.")
            prior = self._prior
        else:
            check_if_prior_on_device(self._device, prior)
        if density_estimator is None:
            if self._neural_net is None:
                raise ValueError("No trained estimator: call .train() first or pass density_estimator=...")
            estimator = deepcopy(self._neural_net)
            device = self._device
        else:
            estimator = density_estimator
            device = str(next(density_estimator.parameters()).device)
        if sample_with == "mcmc":
            from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior

            mcmc_parameters = dict(mcmc_parameters or {})
            enable_transform = mcmc_parameters.pop("enable_transform", True)
            potential_fn, theta_transform = likelihood_estimator_based_potential(estimator, prior, x_o=None,
                                                                                 enable_transform=enable_transform)
            self._posterior = MCMCPosterior(potential_fn=potential_fn, proposal=prior, theta_transform=theta_transform,
                                            method=mcmc_method, device=device, **mcmc_parameters)
            return deepcopy(self._posterior)
        from sbi_amd.inference.posteriors.rejection_posterior import RejectionPosterior

        params = dict(rejection_sampling_parameters or {})
        unknown = set(params) - {"max_sampling_batch_size", "num_samples_to_find_max", "num_iter_to_find_max", "m"}
        if unknown:
            raise TypeError(f"unexpected rejection_sampling_parameters: {sorted(unknown)}")
        potential_fn, _ = likelihood_estimator_based_potential(estimator, prior, x_o=None)
        self._posterior = RejectionPosterior(potential_fn=potential_fn, proposal=prior,
                                             theta_transform=mcmc_transform(prior, device=device), device=device,
                                             **params)
        return deepcopy(self._posterior)


NLE = NLE_A    # sbi/inference/__init__.py
SNLE = NLE_A
