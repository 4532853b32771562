"""``build_mdn`` -- builds the mixture-density-network estimator for p(x|y) (= p(theta|x) in NPE).

Drop-in for sbi/neural_nets/net_builders/mdn.py restricted to what the HIP path implements: the default two-layer
ReLU hidden net, z-scoring of both sides (the condition's through the ``standardizing_net`` in front of the embedding,
as ``build_nsf`` does it), an optional frozen / parameter-free embedding net.  Unsupported options raise instead of
silently degrading.
"""

from __future__ import annotations

import warnings
from typing import Optional

from torch import Tensor, nn

from sbi_amd.neural_nets.estimators.mdn import ENVELOPE, MDNHyper, MDNNet, MixtureDensityEstimator
from sbi_amd.neural_nets.net_builders.flow import _flow_inputs, check_data_device
from sbi_amd.utils.sbiutils import z_score_parser, z_standardization


def build_mdn(
    batch_x: Tensor,
    batch_y: Tensor,
    z_score_x: Optional[str] = "independent",
    z_score_y: Optional[str] = "independent",
    hidden_features: int = 50,
    num_components: int = 10,
    embedding_net: nn.Module = nn.Identity(),
    **kwargs,
) -> MixtureDensityEstimator:
    """Same signature and meaning as the reference ``build_mdn``; unknown kwargs are ignored as there."""
    check_data_device(batch_x, batch_y)
    if z_score_x == "transform_to_unconstrained":
        raise NotImplementedError("sbi_amd.build_mdn: z_score_x='transform_to_unconstrained' (the prior's support "
                                  "transform in front of the mixture) is not implemented. Use one of 'none', "
                                  "'independent', 'structured'.")
    if kwargs.get("hidden_net") is not None:
        raise NotImplementedError("sbi_amd.build_mdn: a custom hidden_net is not implemented (the kernels run the "
                                  "default Linear-ReLU-Linear-ReLU hidden net)")
    if kwargs.get("x_dist") is not None:
        warnings.warn("sbi_amd.build_mdn: x_dist is only used by z_score_x='transform_to_unconstrained' and is ignored",
                      stacklevel=2)
    D, C, zstats, zx, zy, embedding = _flow_inputs(batch_x, batch_y, z_score_x, z_score_y, embedding_net, "build_mdn")
    if zx:
        # _flow_inputs keeps theta's z-scoring as the flows' multiplicative pair (-mean/std, 1/std); the mixture's
        # buffers are the reference's `_transform_shift` = mean and `_transform_scale` = std
        mean, std = z_standardization(batch_x.detach().cpu().float(), z_score_parser(z_score_x)[1])
        zstats[:D] = mean.expand(D)
        zstats[D : 2 * D] = std.expand(D)
    hyper = MDNHyper(D=D, C=C, hidden_features=int(hidden_features), num_components=int(num_components))
    if not hyper.in_envelope():
        from sbi_amd import _lib

        raise RuntimeError(f"sbi_amd: mixture density network with theta-dim {D}, x-dim {C}, hidden_features "
                           f"{hyper.hidden_features}, num_components {hyper.num_components}: configuration not "
                           f"supported by the HIP kernels ({ENVELOPE}; error {_lib.E_UNSUPPORTED})")
    net = MDNNet(hyper, zstats, z_score_theta=zx, z_score_x=zy)
    return MixtureDensityEstimator(net, input_shape=batch_x[0].shape, condition_shape=batch_y[0].shape,
                                   embedding_net=embedding)
