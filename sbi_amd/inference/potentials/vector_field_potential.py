"""Potential of a score-based posterior: its gradient is the (composed) score the SDE sampler follows.

Mirror of sbi's ``VectorFieldBasedPotential`` and ``vector_field_estimator_based_potential``
(sbi/inference/potentials/vector_field_potential.py:23-330) for what runs on the HIP kernels: ``gradient(theta, time)`` is
the score of one observation (``sbi_amd_npse_score``) or, with ``x_is_iid`` and several observations, the iid composition
of ``vector_field_adaptor`` (``sbi_amd_npse_score_iid``).  ``__call__`` (the log-probability through the probability-flow
ODE) is refused for score estimators exactly as ``VectorFieldPosterior.log_prob`` refuses it.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch
from torch import Tensor

from sbi_amd.inference.potentials.vector_field_adaptor import get_iid_method


class VectorFieldBasedPotential:
    def __init__(self, vector_field_estimator, prior, x_o: Optional[Tensor] = None, iid_method: str = "auto_gauss",
                 iid_params: Optional[Dict[str, Any]] = None, device: str = "cpu"):
        from sbi_amd.neural_nets.estimators.score_estimator import ConditionalScoreEstimator

        if not isinstance(vector_field_estimator, ConditionalScoreEstimator):
            raise NotImplementedError("sbi_amd: VectorFieldBasedPotential runs score estimators (NPSE); the FMPE "
                                      "posterior samples and evaluates through its probability-flow ODE")
        self.vector_field_estimator = vector_field_estimator
        self.prior = prior
        self.device = device
        self.x_is_iid = False
        self.iid_method = iid_method
        self.iid_params = iid_params
        self._x_o: Optional[Tensor] = None
        self._iid_fn = None
        if x_o is not None:
            self.set_x(x_o)

    @property
    def x_o(self) -> Tensor:
        if self._x_o is None:
            raise ValueError("No observed data x_o is available. Use `potential_fn.set_x(x_o)`.")
        return self._x_o

    def set_x(self, x_o: Optional[Tensor], x_is_iid: Optional[bool] = False, iid_method: str = "auto_gauss",
              iid_params: Optional[Dict[str, Any]] = None, **unsupported) -> None:
        """vector_field_potential.py:80-118 (guidance and ODE arguments are outside the HIP path)."""
        unsupported = {k: v for k, v in unsupported.items() if v is not None}
        if unsupported:
            raise NotImplementedError(f"sbi_amd NPSE: {sorted(unsupported)} (guidance, ODE settings) are not implemented; "
                                      "what runs: the score of one observation and the fnpe / gauss / auto_gauss "
                                      "composition of iid observations")
        cshape = self.vector_field_estimator.condition_shape
        x = None if x_o is None else torch.as_tensor(x_o, dtype=torch.float32).reshape(-1, *cshape)
        self.x_is_iid = bool(x_is_iid)
        self.iid_method, self.iid_params = iid_method, iid_params
        self._iid_fn = None
        if x is not None and x.shape[0] > 1:
            if not self.x_is_iid:
                raise ValueError("several observations need x_is_iid=True (sample_batched handles independent ones)")
            self._iid_fn = get_iid_method(iid_method)(self.vector_field_estimator, self.prior, device=self.device,
                                                      **(iid_params or {}))
        self._x_o = None if x is None else x.to(self.device)

    def __call__(self, theta: Tensor, track_gradients: bool = True) -> Tensor:
        raise NotImplementedError("sbi_amd NPSE: log_prob of a score-based posterior is not implemented (it needs the "
                                  "divergence of ode_fn, and for iid observations a flow per observation); sample with "
                                  "'sde'")

    @torch.no_grad()
    def gradient(self, theta: Tensor, time: Optional[Tensor] = None, track_gradients: bool = False) -> Tensor:
        """Score at (theta, time): theta (b, D) -> (b, D); time defaults to t_min."""
        if track_gradients:
            raise NotImplementedError("sbi_amd NPSE: the score does not track gradients with respect to theta")
        est = self.vector_field_estimator
        if time is None:
            time = torch.tensor([est.t_min])
        time = torch.as_tensor(time, dtype=torch.float32).reshape(-1)[:1].to(self.device)
        theta = torch.as_tensor(theta, dtype=torch.float32).to(self.device)
        D = est.input_shape[0]
        flat = theta.reshape(-1, D)
        if self._iid_fn is None:
            return est.score(flat, self.x_o[:1], time).reshape(theta.shape)
        return self._iid_fn(flat.unsqueeze(1), self.x_o, time).reshape(theta.shape)


def vector_field_estimator_based_potential(vector_field_estimator, prior, x_o: Optional[Tensor] = None,
                                           enable_transform: bool = False, **kwargs) -> Tuple[VectorFieldBasedPotential, Any]:
    """(potential, identity transform), vector_field_potential.py:23-58.  sbi defaults ``enable_transform`` to True and
    hands the transform to its MAP search; the SDE sampler here runs in theta space and nothing consumes a transform, so
    the default is False and True is refused rather than ignored."""
    if enable_transform:
        raise NotImplementedError("sbi_amd NPSE: enable_transform is not implemented (the SDE runs in theta space)")
    device = str(next(vector_field_estimator.parameters()).device)
    potential = VectorFieldBasedPotential(vector_field_estimator, prior, x_o, device=device, **kwargs)
    return potential, torch.distributions.transforms.identity_transform
