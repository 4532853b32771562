"""Mixed Neural Likelihood Estimation (Boelts et al. 2022) on the MNLE kernels.

API mirror of sbi's ``MNLE`` (sbi/inference/trainers/nle/mnle.py): NLE whose estimator is a ``MixedDensityEstimator``
over x = [continuous column, categorical columns] given theta.  Training is the device-resident loop of NPE / NLE with
``FusedMNLEStep`` on the flat parameter buffer (single device); the posterior is MCMC or rejection sampling on
``LikelihoodBasedPotential``, whose iid-trial sum is one pass of sbi_amd_mnle_log_prob_trials.
"""

from __future__ import annotations

import warnings
from typing import Any, Callable, Dict, Optional, Union

import torch
from torch import nn
from torch.distributions import Distribution

from sbi_amd.inference.trainers.nle.nle import NLE_A
from sbi_amd.neural_nets.estimators.mixed_density_estimator import MixedDensityEstimator
from sbi_amd.neural_nets.factory import likelihood_nn
from sbi_amd.neural_nets.net_builders.estimator_configs import MixedConfig, NSFConfig


class MNLE(NLE_A):
    def __init__(self, prior: Optional[Distribution] = None,
                 density_estimator: Union[str, MixedConfig, Callable, None] = None, device: str = "cpu",
                 logging_level: Union[int, str] = "WARNING", summary_writer=None, tracker=None,
                 show_progress_bars: bool = True):
        if density_estimator is None:
            density_estimator = MixedConfig()
        elif isinstance(density_estimator, str):
            if density_estimator != "mnle":
                raise ValueError("MNLE supports only the preconfigured 'mnle' density estimator, "
                                 f"not {density_estimator!r}.")
            warnings.warn("Passing a string for `density_estimator` is deprecated. Use MixedConfig(...) instead, "
                          "e.g. `from sbi_amd.neural_nets import MixedConfig`.", FutureWarning, stacklevel=2)
            density_estimator = likelihood_nn(model="mnle")
        elif not (isinstance(density_estimator, MixedConfig) or callable(density_estimator)):
            raise TypeError("density_estimator must be None, 'mnle', a MixedConfig or a builder function, got "
                            f"{type(density_estimator).__name__}")
        super().__init__(prior=prior, density_estimator=NSFConfig(), device=device, logging_level=logging_level,
                         summary_writer=summary_writer, tracker=tracker, show_progress_bars=show_progress_bars)
        if isinstance(density_estimator, MixedConfig):
            cfg = density_estimator
            self._build_neural_net = lambda batch_theta, batch_x: cfg.build(batch_x, batch_theta)
        else:
            self._build_neural_net = density_estimator

    # -- hooks of the epoch loop
    def _fused_training(self, net: nn.Module, calibration_kernel, emb_trainable: bool, atomic: bool) -> bool:
        return (isinstance(net, MixedDensityEstimator) and torch.device(self._device).type == "cuda"
                and calibration_kernel is None and not emb_trainable and not atomic)

    def _make_stepper(self, net: nn.Module, cfg, dist_mod):
        from sbi_amd.inference.trainers.fused import FusedMNLEStep

        if dist_mod is not None:
            raise NotImplementedError("sbi_amd: multi-GPU training of MNLE is not implemented; train it on one device")
        return FusedMNLEStep(net, lr=cfg.learning_rate, clip_max_norm=cfg.clip_max_norm)

    def train(self, *args, **kwargs) -> MixedDensityEstimator:
        if torch.device(self._device).type == "cuda" and self._dist() is not None:
            raise NotImplementedError("sbi_amd: multi-GPU training of MNLE is not implemented; train it on one device")
        est = super().train(*args, **kwargs)
        assert isinstance(est, MixedDensityEstimator), \
            f"Internal net must be of type MixedDensityEstimator but is {type(est)}."
        return est

    def build_posterior(self, density_estimator: Optional[MixedDensityEstimator] = None,
                        prior: Optional[Distribution] = None, sample_with: str = "mcmc",
                        mcmc_method: str = "slice_np_vectorized", mcmc_parameters: Optional[Dict[str, Any]] = None,
                        rejection_sampling_parameters: Optional[Dict[str, Any]] = None, **kwargs):
        if sample_with in ("vi", "importance"):
            raise NotImplementedError(f"sample_with={sample_with!r}: VI / importance posteriors are outside the "
                                      "accelerated path; MNLE samples with 'mcmc' or 'rejection'.")
        if density_estimator is not None:
            assert isinstance(density_estimator, MixedDensityEstimator), \
                f"net must be of type MixedDensityEstimator but is {type(density_estimator)}."
        return super().build_posterior(density_estimator=density_estimator, prior=prior, sample_with=sample_with,
                                       mcmc_method=mcmc_method, mcmc_parameters=mcmc_parameters,
                                       rejection_sampling_parameters=rejection_sampling_parameters, **kwargs)
