"""CPU restatement (plain PyTorch, eager) of sbi's default density estimator, the affine MAF that ``build_maf``
assembles (sbi/neural_nets/net_builders/flow.py:115-209) -- TEST INFRASTRUCTURE, never the product path.

PARITY UNPINNED at the nflows boundary, with the caveat of oracle/maf_oracle.py (nflows 0.14 is not importable
here): ``MaskedAffineAutoregressiveTransform`` below restates the published nflows algorithm on that file's ``MADE``
(``output_multiplier=2``) and ``RandomPermutation``:
  * ``params.view(-1, D, 2)``: ``[..., 0]`` the unconstrained scale, ``[..., 1]`` the shift;
  * ``scale = softplus(unconstrained_scale) + 1e-3``; forward ``scale * x + shift``, logabsdet ``sum log scale``;
    inverse ``(y - shift) / scale`` over D passes from zeros, logabsdet ``-sum log scale``.
Module / attribute names follow nflows so that ``state_dict()`` keys match a real ``NFlowsFlow(build_maf(...))``.
"""

from __future__ import annotations

from typing import List

import torch
from torch import Tensor, nn
from torch.nn import functional as F

from oracle.maf_oracle import MADE, RandomPermutation
from oracle.nsf_oracle import (CompositeTransform, Flow, NSFOracle, PointwiseAffineTransform, StandardNormal,
                               Standardize, sum_except_batch, z_standardization)


class MaskedAffineAutoregressiveTransform(nn.Module):
    def __init__(self, features, hidden_features, context_features, num_blocks=2, epsilon=1e-3):
        super().__init__()
        self.features = features
        self._epsilon = epsilon
        self.autoregressive_net = MADE(features, hidden_features, context_features, num_blocks, output_multiplier=2)

    def _unconstrained_scale_and_shift(self, params: Tensor):
        p = params.view(-1, self.features, 2)
        return p[..., 0], p[..., 1]

    def scale_and_shift(self, inputs, context=None):
        u, shift = self._unconstrained_scale_and_shift(self.autoregressive_net(inputs, context))
        return F.softplus(u) + self._epsilon, shift

    def forward(self, inputs, context=None):
        scale, shift = self.scale_and_shift(inputs, context)
        return scale * inputs + shift, sum_except_batch(torch.log(scale))

    def inverse(self, inputs, context=None):
        outputs = torch.zeros_like(inputs)
        logabsdet = None
        for _ in range(inputs.shape[1]):                 # one more dimension becomes exact per pass
            scale, shift = self.scale_and_shift(outputs, context)
            outputs = (inputs - shift) / scale
            logabsdet = -sum_except_batch(torch.log(scale))
        return outputs, logabsdet


class MAFOracle(NSFOracle):
    """What ``NFlowsFlow(build_maf(batch_x=theta, batch_y=x, ...))`` computes; the NFlowsFlow surface
    (log_prob / loss / sample / inverse_transform / sample_from_noise) is inherited."""

    def __init__(self, batch_theta: Tensor, batch_x: Tensor, z_score_theta="independent", z_score_x="independent",
                 hidden_features=50, num_transforms=5, num_blocks=2, epsilon=1e-3):
        nn.Module.__init__(self)
        D, C = batch_theta[0].numel(), batch_x[0].numel()
        self.input_shape, self.condition_shape = batch_theta[0].shape, batch_x[0].shape
        transforms: List[nn.Module] = []
        for _ in range(num_transforms):                  # flow.py:175-190
            transforms.append(MaskedAffineAutoregressiveTransform(D, hidden_features, C, num_blocks=num_blocks,
                                                                  epsilon=epsilon))
            transforms.append(RandomPermutation(D))
        if z_score_theta in ("independent", "structured"):
            mean, std = z_standardization(batch_theta, z_score_theta == "structured", 1e-14)
            transforms = [PointwiseAffineTransform(shift=-mean / std, scale=1 / std)] + transforms
        if z_score_x in ("independent", "structured"):
            if len(batch_x) > 1:
                mean, std = z_standardization(batch_x, z_score_x == "structured", 1e-7)
            else:
                mean, std = torch.mean(batch_x, dim=0), torch.ones(1)
            embedding = nn.Sequential(Standardize(mean, std), nn.Identity())
        else:
            embedding = nn.Identity()
        dist = StandardNormal((D,))
        dist._log_z = dist._log_z.to(torch.float32)
        self.net = Flow(CompositeTransform(transforms), dist, embedding)
