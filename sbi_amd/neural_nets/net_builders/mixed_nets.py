"""``build_mnle``: sbi's mixed neural likelihood estimator (sbi/neural_nets/net_builders/mixed_nets.py) on the MNLE
kernels, for x = [one continuous column, then 1..4 categorical columns]."""

from __future__ import annotations

import warnings
from typing import Optional

import torch
from torch import Tensor, nn

from sbi_amd.neural_nets.estimators.mixed_density_estimator import (ENVELOPE, MAX_CATEGORIES, MixedDensityEstimator,
                                                                    MNLEHyper, MNLENet)
from sbi_amd.neural_nets.net_builders.categorial import _is_discrete, infer_categories
from sbi_amd.neural_nets.net_builders.flow import check_data_device
from sbi_amd.utils.sbiutils import standardizing_stats, z_score_parser, z_standardization


def _build_mixed_density_estimator(batch_x: Tensor, batch_y: Tensor, z_score_x: Optional[str] = "independent",
                                   z_score_y: Optional[str] = "independent", flow_model: str = "nsf",
                                   continuous_config=None, num_categories_per_variable: Optional[Tensor] = None,
                                   embedding_net: nn.Module = nn.Identity(),
                                   combined_embedding_net: Optional[nn.Module] = None, num_transforms: int = 5,
                                   num_bins: int = 10, hidden_features: int = 50, tail_bound: float = 10.0,
                                   log_transform_x: bool = False, discrete_hidden_features: Optional[int] = None,
                                   discrete_hidden_layers: int = 2, combined_embedding_features: Optional[int] = None,
                                   dropout_probability: float = 0.0, continuous_hidden_features: Optional[int] = None,
                                   hidden_layers_spline_context: int = 1, **kwargs) -> MixedDensityEstimator:
    from sbi_amd.neural_nets.net_builders.estimator_configs import NSFConfig

    check_data_device(batch_x, batch_y)
    if continuous_config is not None:
        if type(continuous_config) is not NSFConfig:
            raise NotImplementedError(f"sbi_amd MNLE: the continuous part is the NSF only (got "
                                      f"{type(continuous_config).__name__}); use continuous=NSFConfig(...)")
        cc = continuous_config
        z_score_x, num_transforms, num_bins = cc.z_score_input, cc.num_transforms, cc.num_bins
        tail_bound, cont_hf = cc.tail_bound, cc.hidden_features
        hidden_layers_spline_context = getattr(cc, "hidden_layers_spline_context", hidden_layers_spline_context)
    else:
        if flow_model != "nsf":
            raise NotImplementedError(f"sbi_amd MNLE: the continuous part is the NSF only (got flow_model="
                                      f"{flow_model!r}); use flow_model='nsf'")
        cont_hf = continuous_hidden_features or hidden_features
    if kwargs:
        warnings.warn(f"Unknown kwargs {sorted(kwargs)} are ignored by build_mnle.", UserWarning, stacklevel=2)
    disc_hf = discrete_hidden_features if discrete_hidden_features is not None else \
        (cont_hf if continuous_config is not None else hidden_features)
    emb_f = combined_embedding_features if combined_embedding_features is not None else cont_hf
    if dropout_probability > 0:
        raise NotImplementedError("sbi_amd MNLE: dropout_probability > 0 is not implemented; use 0.0")
    if combined_embedding_net is not None:
        raise NotImplementedError("sbi_amd MNLE: a custom combined_embedding_net is not implemented; the built-in "
                                  "two-layer ReLU MLP (combined_embedding_features) runs on the kernels")
    warnings.warn("The mixed neural density estimator assumes that inferred variable contains continuous data in the "
                  "first n-k columns and categorical data in the last k columns.", stacklevel=2)
    if num_categories_per_variable is None:
        num_disc = int(torch.sum(_is_discrete(batch_x)))
    else:
        num_disc = len(num_categories_per_variable)
    n_cont = batch_x.shape[1] - num_disc
    if n_cont != 1:
        raise NotImplementedError(f"sbi_amd MNLE: exactly one continuous column followed by the discrete columns is "
                                  f"implemented (found {n_cont} continuous, {num_disc} discrete); for purely "
                                  "continuous data use NLE with likelihood_nn('nsf')")
    if not 1 <= num_disc <= 4:
        raise NotImplementedError(f"sbi_amd MNLE: 1..4 discrete columns are implemented (found {num_disc}); merge "
                                  "columns into one categorical variable or use NLE")
    cont_x, disc_x = batch_x[:, :1], batch_x[:, 1:]
    cats, values = infer_categories(disc_x, num_categories_per_variable)
    if max(cats) > MAX_CATEGORIES:
        raise NotImplementedError(f"sbi_amd MNLE: at most {MAX_CATEGORIES} categories per variable are implemented "
                                  f"(found {max(cats)}); bin the variable more coarsely")
    emb = None if isinstance(embedding_net, nn.Identity) else embedding_net
    with torch.no_grad():
        emb_y = batch_y if emb is None else emb(batch_y)
    C = emb_y[0].numel()
    if emb is not None and C > 64 and any(p.requires_grad for p in emb.parameters()):
        raise NotImplementedError("sbi_amd MNLE: a trainable theta embedding_net wider than 64 outputs is not "
                                  "implemented; reduce its output to <= 64 features")
    hyper = MNLEHyper(num_categories=tuple(cats), C=C, discrete_hidden=int(disc_hf),
                      discrete_blocks=int(discrete_hidden_layers), embedding=int(emb_f), hidden=int(cont_hf),
                      num_bins=int(num_bins), num_transforms=int(num_transforms),
                      context_layers=int(hidden_layers_spline_context), tail_bound=float(tail_bound),
                      log_transform=bool(log_transform_x), z_score_x=z_score_parser(z_score_x)[0])
    if not hyper.in_envelope():
        raise NotImplementedError(f"sbi_amd MNLE: configuration outside the kernels' envelope ({ENVELOPE})")
    # z-scoring: the condition as the reference's standardizing_net (in front of the embedding, which the kernels
    # cannot do for a non-identity embedding: there the embedded batch is standardised instead), the continuous column
    # as the flow's first affine transform z = x * scale + shift
    zy, structured_y = z_score_parser(z_score_y)
    if zy:
        mean_c, std_c = standardizing_stats(emb_y.reshape(len(emb_y), -1), structured_y)
        mean_c, std_c = mean_c.reshape(-1).expand(C), std_c.reshape(-1).expand(C)
    else:
        mean_c, std_c = torch.zeros(C), torch.ones(C)
    cx = torch.log(cont_x + 1e-10) if log_transform_x else cont_x
    zx, structured_x = z_score_parser(z_score_x)
    if zx:
        m, s = z_standardization(cx, structured_x)
        shift, scale = (-m / s).reshape(-1)[:1], (1 / s).reshape(-1)[:1]
    else:
        shift, scale = torch.zeros(1), torch.ones(1)
    lookup = torch.zeros(hyper.V, MAX_CATEGORIES)
    for i, v in enumerate(values):
        lookup[i, : v.numel()] = torch.sort(v).values
    zstats = torch.cat([shift.float(), scale.float(), mean_c.float(), std_c.float(), lookup.reshape(-1)])
    net = MNLENet(hyper, zstats)
    return MixedDensityEstimator(net, input_shape=batch_x[0].shape, condition_shape=batch_y[0].shape,
                                 embedding_net=emb, log_transform_input=bool(log_transform_x))


def build_mnle(batch_x: Tensor, batch_y: Tensor, log_transform_x: bool = False, **kwargs) -> MixedDensityEstimator:
    """Mixed neural likelihood estimator p(x | theta): batch_x = data, batch_y = parameters."""
    return _build_mixed_density_estimator(batch_x=batch_x, batch_y=batch_y, log_transform_x=log_transform_x, **kwargs)


def build_mnpe(*args, **kwargs):
    raise NotImplementedError("sbi_amd: MNPE (mixed posterior estimation) is not implemented; MNLE (build_mnle) is, "
                              "and NPE covers continuous parameters")
