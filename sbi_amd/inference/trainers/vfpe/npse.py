"""Neural Posterior Score Estimation with the device-resident training loop of the FMPE trainer.

API mirror of sbi's ``NPSE`` (sbi/inference/trainers/vfpe/npse.py:25-330) on ``VectorFieldTrainer.train``
(sbi/inference/trainers/vfpe/base_vf_inference.py:206-350): the loop, the validation at fixed times with the nugget, the
exponential moving averages and the convergence rule are those of ``FMPE`` (fmpe.py in this package); a training step is
the fused denoising-score-matching forward + backward + clip / Adam (``FusedNPSEStep``).  The posterior samples with the
fused Euler-Maruyama kernel (``sample_with="sde"``, the default as in sbi) or the probability-flow ODE.
"""

from __future__ import annotations

import warnings
from copy import deepcopy
from typing import Callable, Optional, Union

from torch import Tensor

from sbi_amd.inference.trainers.vfpe.fmpe import FMPE
from sbi_amd.neural_nets.estimators.score_estimator import ConditionalScoreEstimator

_REFUSED_MODELS = ("ada_mlp", "transformer", "transformer_cross_attn")


def posterior_score_nn(sde_type: str = "ve", model: str = "mlp", z_score_theta: Optional[str] = "independent",
                       z_score_x: Optional[str] = "independent", hidden_features: int = 100, num_layers: int = 5,
                       t_embedding_dim: int = 32, **kwargs) -> Callable:
    """sbi/neural_nets/factory.py ``posterior_score_nn`` for the default MLP.  The returned builder carries its
    ``sde_type`` (the role ``VectorFieldEstimatorBuilder.sde_type`` plays in sbi's conflict rule)."""
    if model != "mlp":
        known = " (one of sbi's other score networks)" if model in _REFUSED_MODELS else ""
        raise NotImplementedError(f"sbi_amd NPSE implements model='mlp' only, got {model!r}{known}")
    if sde_type not in ("ve", "vp", "subvp"):
        raise ValueError(f"Unknown SDE type: {sde_type}")

    def build_fn(batch_theta: Tensor, batch_x: Tensor) -> ConditionalScoreEstimator:
        from sbi_amd.neural_nets.estimators.score_estimator import build_score_matching_estimator

        return build_score_matching_estimator(batch_theta, batch_x, sde_type=sde_type, z_score_theta=z_score_theta,
                                              z_score_x=z_score_x, hidden_features=hidden_features,
                                              num_layers=num_layers, time_embedding_dim=t_embedding_dim, **kwargs)

    build_fn.sde_type = sde_type
    return build_fn


class NPSE(FMPE):
    def __init__(self, prior=None, vf_estimator: Union[str, Callable, None] = None,
                 score_estimator: Union[str, Callable, None] = None, density_estimator: Optional[Callable] = None,
                 sde_type: Optional[str] = None, device: str = "cpu", logging_level: Union[int, str] = "WARNING",
                 summary_writer=None, tracker=None, show_progress_bars: bool = True):
        for name, old in (("score_estimator", score_estimator), ("density_estimator", density_estimator)):
            if old is None:
                continue
            if vf_estimator is not None:
                raise ValueError(f"Cannot pass both `{name}` and `vf_estimator`. Use `vf_estimator` only; `{name}` is "
                                 "deprecated.")
            warnings.warn(f"`{name}` is deprecated and will be removed in a future release. Use `vf_estimator` "
                          "instead.", FutureWarning, stacklevel=2)
            vf_estimator = old
        # the builder owns sde_type: refuse only when both are given and disagree (npse.py:160-173)
        built_sde = getattr(vf_estimator, "sde_type", None) if callable(vf_estimator) else None
        if sde_type is not None and built_sde is not None and sde_type != built_sde:
            raise ValueError(f"Conflicting `sde_type`: trainer received {sde_type!r} but the builder has {built_sde!r}. "
                             f"Set `sde_type` on the builder only: posterior_score_nn(sde_type={sde_type!r}).")
        resolved = sde_type if sde_type is not None else "ve"
        if vf_estimator is None:
            builder = posterior_score_nn(sde_type=resolved)
        elif isinstance(vf_estimator, str):
            warnings.warn("Passing a string for `vf_estimator` is deprecated. Use "
                          "posterior_score_nn(model=...) instead.", FutureWarning, stacklevel=2)
            builder = posterior_score_nn(sde_type=resolved, model=vf_estimator)
        else:
            builder = vf_estimator
        super().__init__(prior=prior, vf_estimator=builder, device=device, logging_level=logging_level,
                         summary_writer=summary_writer, tracker=tracker, show_progress_bars=show_progress_bars)

    def append_simulations(self, theta, x, proposal=None, exclude_invalid_x=None, data_device=None):
        if proposal is not None and proposal is not self._prior:
            raise NotImplementedError("Multi-round NPSE with arbitrary proposals is not implemented")
        return super().append_simulations(theta, x, None, exclude_invalid_x, data_device)

    @staticmethod
    def _fused_step_cls(net):
        if isinstance(net, ConditionalScoreEstimator):
            from sbi_amd.inference.trainers.fused import FusedNPSEStep

            return FusedNPSEStep
        return None

    def build_posterior(self, vector_field_estimator: Optional[ConditionalScoreEstimator] = None, prior=None,
                        sample_with: str = "sde", **kwargs):
        from sbi_amd.inference.posteriors.vector_field_posterior import VectorFieldPosterior

        if sample_with not in ("sde", "ode"):
            raise ValueError(f"sample_with must be 'ode' or 'sde', but is {sample_with}.")
        est = vector_field_estimator if vector_field_estimator is not None else self._neural_net
        if est is None:
            raise ValueError("train() first or pass a vector_field_estimator")
        prior = prior if prior is not None else self._prior
        self._posterior = VectorFieldPosterior(deepcopy(est).to(self._device), prior, device=str(self._device),
                                               sample_with=sample_with, **kwargs)
        return self._posterior
