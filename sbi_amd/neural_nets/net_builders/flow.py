"""``build_nsf`` -- builds the NSF estimator for p(x|y) (= p(theta|x) in NPE).

Drop-in for sbi/neural_nets/net_builders/flow.py:333-460 restricted to what the
HIP path implements: ResidualNet-conditioned RQ-spline couplings with linear
tails + LULinear, alternating masks, z-scoring of both sides, optional embedding
net in front (plain PyTorch; the kernels return the gradient wrt its output).
Unsupported options raise instead of silently degrading.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from sbi_amd.neural_nets.estimators.nsf_flow import NSFFlow, NSFHyper, NSFNet
from sbi_amd.utils.sbiutils import (
    assert_transform_to_unconstrained_supported,
    standardizing_stats,
    z_score_parser,
    z_standardization,
)


def check_data_device(datum_1: Tensor, datum_2: Tensor) -> None:
    """sbi/utils/torchutils.py `check_data_device`: both batches on one device."""
    if datum_1.device != datum_2.device:
        raise AssertionError(
            "Mismatch in fed data's device: "
            f"datum_1 has device '{datum_1.device}' whereas datum_2 has device '{datum_2.device}'. "
            "Please use data from a common device."
        )


def _flow_inputs(batch_x: Tensor, batch_y: Tensor, z_score_x, z_score_y, embedding_net: nn.Module, builder: str):
    """Shared front end of the flow builders (flow.py:393-394, 441-452, 1395-1416): event sizes, the optional
    `standardizing_net -> embedding_net` module in front of the kernels, and the z-scoring buffers
    `zstats = [theta shift, theta scale, x mean, x std]`.  Returns (D, C, zstats, zx, zy, embedding | None)."""
    x_numel = batch_x[0].numel()
    y_numel = batch_y[0].numel()
    has_embedding = not isinstance(embedding_net, nn.Identity)
    if batch_x[0].dim() != 1 or (batch_y[0].dim() != 1 and not has_embedding):
        raise NotImplementedError(f"sbi_amd.{builder}: theta events must be 1-D (and x events too unless an "
                                  "embedding net maps them to feature vectors)")
    embedding = None
    if has_embedding:
        # flow.py:1395-1416 (`get_embedding_net`): standardizing_net(batch_y) -> embedding_net runs in front of
        # the flow as ordinary PyTorch modules; the kernels see the embedded features and hand back d loss / d
        # features (grad_x_out) so the embedding trains through autograd.  No second z-scoring in the kernel.
        zy, structured_y = z_score_parser(z_score_y)
        mods = []
        if zy:
            mean, std = standardizing_stats(batch_y.detach().cpu().float(), structured_y)
            mods.append(Standardize(mean, std))
        mods.append(embedding_net)
        embedding = nn.Sequential(*mods)
        with torch.no_grad():
            emb_out = embedding.to(batch_y.device)(batch_y[:2].float())
        if emb_out.dim() != 2:
            raise ValueError(f"The embedding net must return (batch, features); got shape {tuple(emb_out.shape)}")
        y_numel = emb_out.shape[1]          # get_numel(batch_y, embedding_net=...) (nn_utils.py:17-47)
        z_score_y = "none"

    D, C = x_numel, y_numel
    zstats = torch.cat([torch.zeros(D), torch.ones(D), torch.zeros(C), torch.ones(C)])
    zx, structured_x = z_score_parser(z_score_x)
    if zx:
        mean, std = z_standardization(batch_x.detach().cpu().float(), structured_x)
        # PointwiseAffineTransform(shift=-mean/std, scale=1/std)  (sbiutils.py:247)
        zstats[:D] = (-mean / std).expand(D)
        zstats[D : 2 * D] = (1 / std).expand(D)
    zy, structured_y = z_score_parser(z_score_y)
    if zy:
        mean, std = standardizing_stats(batch_y.detach().cpu().float(), structured_y)
        zstats[2 * D : 2 * D + C] = mean.expand(C)
        zstats[2 * D + C :] = std.expand(C)

    return D, C, zstats, zx, zy, embedding


def build_nsf(
    batch_x: Tensor,
    batch_y: Tensor,
    z_score_x: Optional[str] = "independent",
    z_score_y: Optional[str] = "independent",
    hidden_features: int = 50,
    num_transforms: int = 5,
    num_bins: int = 10,
    embedding_net: nn.Module = nn.Identity(),
    tail_bound: float = 3.0,
    hidden_layers_spline_context: int = 1,
    num_blocks: int = 2,
    dropout_probability: float = 0.0,
    use_batch_norm: bool = False,
    **kwargs,
) -> NSFFlow:
    """Same signature and meaning as the reference ``build_nsf`` (flow.py:333-352)."""
    check_data_device(batch_x, batch_y)
    assert_transform_to_unconstrained_supported(
        z_score_x, "build_nsf",
        "Use one of 'none', 'independent', 'structured'.",
    )
    if dropout_probability != 0.0 or use_batch_norm:
        raise NotImplementedError("sbi_amd.build_nsf: dropout / batch norm are not implemented in the HIP path")
    x_numel = batch_x[0].numel()
    if x_numel == 1 and not 0 <= int(hidden_layers_spline_context) <= 4:
        raise NotImplementedError(
            "sbi_amd.build_nsf: the 1-D theta conditioner (ContextSplineMap, flow.py:1419-1478) is implemented "
            "for hidden_layers_spline_context = 0 ... 4 (applications of its one shared hidden layer); "
            f"got {hidden_layers_spline_context}."
        )
    D, C, zstats, zx, zy, embedding = _flow_inputs(batch_x, batch_y, z_score_x, z_score_y, embedding_net, "build_nsf")

    hyper = NSFHyper(D=D, C=C, hidden_features=hidden_features, num_transforms=num_transforms,
                     num_bins=num_bins, num_blocks=num_blocks, tail_bound=float(tail_bound),
                     hidden_layers_spline_context=int(hidden_layers_spline_context) if D == 1 else 1)
    net = NSFNet(hyper, zstats, z_score_theta=zx, z_score_x=zy, dtype=kwargs.get("dtype", torch.float32))
    return NSFFlow(net, input_shape=batch_x[0].shape, condition_shape=batch_y[0].shape, embedding_net=embedding)


class Standardize(nn.Module):
    """sbi/utils/sbiutils.py:418-428."""

    def __init__(self, mean: Tensor, std: Tensor):
        super().__init__()
        self.register_buffer("_mean", torch.as_tensor(mean, dtype=torch.float32))
        self.register_buffer("_std", torch.as_tensor(std, dtype=torch.float32))

    def forward(self, tensor: Tensor) -> Tensor:
        return (tensor - self._mean) / self._std


def build_maf_rqs(
    batch_x: Tensor,
    batch_y: Tensor,
    z_score_x: Optional[str] = "independent",
    z_score_y: Optional[str] = "independent",
    hidden_features: int = 50,
    num_transforms: int = 5,
    embedding_net: nn.Module = nn.Identity(),
    num_blocks: int = 2,
    num_bins: int = 10,
    tails: Optional[str] = "linear",
    tail_bound: float = 3.0,
    dropout_probability: float = 0.0,
    use_batch_norm: bool = False,
    min_bin_width: float = 1e-3,
    min_bin_height: float = 1e-3,
    min_derivative: float = 1e-3,
    **kwargs,
):
    """Same signature and meaning as the reference ``build_maf_rqs`` (flow.py:212-330): num_transforms x
    [MaskedPiecewiseRationalQuadraticAutoregressiveTransform(hidden_features, num_blocks feed-forward blocks, tanh,
    linear tails), RandomPermutation], z-scoring of both sides.  Runs on the maf_rqs HIP kernels
    (include/sbi_amd_maf.h); unsupported options raise instead of degrading."""
    from sbi_amd.neural_nets.estimators.maf_flow import MAFHyper, MAFNet, MAFRQSFlow

    check_data_device(batch_x, batch_y)
    assert_transform_to_unconstrained_supported(
        z_score_x, "build_maf_rqs",
        "Use one of 'none', 'independent', 'structured'.",
    )
    if dropout_probability != 0.0 or use_batch_norm:
        raise NotImplementedError("sbi_amd.build_maf_rqs: dropout / batch norm are not implemented in the HIP path")
    if tails != "linear":
        raise NotImplementedError("sbi_amd.build_maf_rqs: only tails='linear' (sbi's default) is implemented")
    if batch_x[0].numel() == 1:
        import warnings

        warnings.warn("In one-dimensional output space, this flow is limited to Gaussians", stacklevel=2)
    D, C, zstats, zx, zy, embedding = _flow_inputs(batch_x, batch_y, z_score_x, z_score_y, embedding_net,
                                                  "build_maf_rqs")
    hyper = MAFHyper(D=D, C=C, hidden_features=hidden_features, num_transforms=num_transforms, num_bins=num_bins,
                     num_blocks=num_blocks, tail_bound=float(tail_bound), min_bin_width=float(min_bin_width),
                     min_bin_height=float(min_bin_height), min_derivative=float(min_derivative))
    net = MAFNet(hyper, zstats, z_score_theta=zx, z_score_x=zy, dtype=kwargs.get("dtype", torch.float32))
    return MAFRQSFlow(net, input_shape=batch_x[0].shape, condition_shape=batch_y[0].shape, embedding_net=embedding)


def build_maf(
    batch_x: Tensor,
    batch_y: Tensor,
    z_score_x: Optional[str] = "independent",
    z_score_y: Optional[str] = "independent",
    hidden_features: int = 50,
    num_transforms: int = 5,
    embedding_net: nn.Module = nn.Identity(),
    num_blocks: int = 2,
    dropout_probability: float = 0.0,
    use_batch_norm: bool = False,
    **kwargs,
):
    """Same signature and meaning as the reference ``build_maf`` (flow.py:115-209), sbi's default density estimator:
    num_transforms x [MaskedAffineAutoregressiveTransform(hidden_features, num_blocks feed-forward blocks, tanh),
    RandomPermutation], z-scoring of both sides.  Runs on the affine MAF HIP kernels
    (include/sbi_amd_maf_affine.h); unsupported options raise instead of degrading, unrelated kwargs are ignored."""
    from sbi_amd.neural_nets.estimators.maf_affine_flow import MAFAffineHyper, MAFAffineNet, MAFFlow

    check_data_device(batch_x, batch_y)
    assert_transform_to_unconstrained_supported(
        z_score_x, "build_maf",
        "Use one of 'none', 'independent', 'structured'.",
    )
    if dropout_probability != 0.0:
        raise NotImplementedError("sbi_amd.build_maf: dropout is not implemented in the HIP path; use "
                                  "dropout_probability=0.0")
    if use_batch_norm:
        raise NotImplementedError("sbi_amd.build_maf: batch norm is not implemented in the HIP path; use "
                                  "use_batch_norm=False (sbi's recommendation)")
    if batch_x[0].numel() == 1:
        import warnings

        warnings.warn("In one-dimensional output space, this flow is limited to Gaussians", stacklevel=2)
    D, C, zstats, zx, zy, embedding = _flow_inputs(batch_x, batch_y, z_score_x, z_score_y, embedding_net, "build_maf")
    hyper = MAFAffineHyper(D=D, C=C, hidden_features=hidden_features, num_transforms=num_transforms,
                           num_blocks=num_blocks)
    net = MAFAffineNet(hyper, zstats, z_score_theta=zx, z_score_x=zy, dtype=kwargs.get("dtype", torch.float32))
    return MAFFlow(net, input_shape=batch_x[0].shape, condition_shape=batch_y[0].shape, embedding_net=embedding)


def build_zuko_nsf(
    batch_x: Tensor,
    batch_y: Tensor,
    z_score_x: Optional[str] = "independent",
    z_score_y: Optional[str] = "independent",
    hidden_features=50,
    num_transforms: int = 5,
    embedding_net: nn.Module = nn.Identity(),
    num_bins: int = 10,
    **kwargs,
):
    """Same signature and meaning as the reference ``build_zuko_nsf`` (flow.py:578-640 -> build_zuko_flow
    :1082-1173 -> zuko.flows.NSF): fully autoregressive spline flow, hyper-nets with
    ``[hidden_features] * num_transforms`` hidden layers (sbi's convention), spline domain [-5, 5].  Runs on the maf
    kernels in their zuko configuration; zuko keyword arguments that change the architecture (``passes``,
    ``randperm``, ``residual``, ``activation``) and ``z_score_x="transform_to_unconstrained"`` are refused."""
    from sbi_amd.neural_nets.estimators.zuko_flow import ZukoHyper, ZukoNSFFlow, ZukoNSFNet

    check_data_device(batch_x, batch_y)
    if z_score_x == "transform_to_unconstrained":
        raise NotImplementedError("sbi_amd.build_zuko_nsf: z_score_x='transform_to_unconstrained' (prior-support "
                                  "bijection in front of the flow) is not implemented in the HIP path")
    nflow_specific = {"num_blocks", "dropout_probability", "use_batch_norm", "tail_bound", "tails",
                      "hidden_layers_spline_context", "num_components", "dtype", "min_bin_width", "min_bin_height",
                      "min_derivative"}                      # build_zuko_flow drops these (flow.py:1140)
    extra = {k: v for k, v in kwargs.items() if k not in nflow_specific}
    if extra:
        raise NotImplementedError(f"sbi_amd.build_zuko_nsf: zuko keyword arguments {sorted(extra)} are not "
                                  "implemented in the HIP path")
    hidden = [hidden_features] * num_transforms if isinstance(hidden_features, int) else list(hidden_features)
    if len(set(hidden)) != 1 or not 1 <= len(hidden) <= 5:
        raise NotImplementedError("sbi_amd.build_zuko_nsf: the hyper-net needs 1..5 hidden layers of one width "
                                  f"(got {hidden}); note that sbi passes [hidden_features] * num_transforms")
    D, C, zstats, zx, zy, embedding = _flow_inputs(batch_x, batch_y, z_score_x, z_score_y, embedding_net,
                                                  "build_zuko_nsf")
    hyper = ZukoHyper(D=D, C=C, hidden_features=int(hidden[0]), num_transforms=num_transforms, num_bins=num_bins,
                      num_hidden_layers=len(hidden))
    net = ZukoNSFNet(hyper, zstats, z_score_theta=zx, z_score_x=zy)
    return ZukoNSFFlow(net, input_shape=batch_x[0].shape, condition_shape=batch_y[0].shape, embedding_net=embedding)
