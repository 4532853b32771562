"""``posterior_nn`` / ``likelihood_nn`` factories for the accelerated path.

Same call signature and behaviours as sbi/neural_nets/factory.py:323-430 for
``model="nsf"``: returns ``build_fn(batch_theta, batch_x)``; unknown kwargs warn
and are forwarded (factory_config_test.py:68-70); other model names are accepted
at factory time and raise ``NotImplementedError`` when the net is built
(:179-183) -- they are other estimator families, outside this path.
"""

from __future__ import annotations

import warnings
from typing import Any, Callable, Optional

from torch import Tensor, nn

from sbi_amd.neural_nets.net_builders.estimator_configs import (MAFRQSConfig, MDNConfig, NSFConfig,
                                                                ResNetClassifierConfig, ZukoNSFConfig)

_NSF_FIELDS = {"hidden_features", "num_transforms", "num_bins", "num_blocks", "dropout_probability",
               "use_batch_norm", "tail_bound", "hidden_layers_spline_context", "dtype"}
_MAF_RQS_FIELDS = (_NSF_FIELDS - {"hidden_layers_spline_context"}) | {"tails", "min_bin_width", "min_bin_height",
                                                                        "min_derivative"}
_MODELS = {"nsf": (NSFConfig, _NSF_FIELDS), "maf_rqs": (MAFRQSConfig, _MAF_RQS_FIELDS)}
_MDN_FIELDS = {"num_components"}


def posterior_nn(
    model: str = "nsf",
    z_score_theta: Optional[str] = "independent",
    z_score_x: Optional[str] = "independent",
    hidden_features: int = 50,
    num_transforms: int = 5,
    num_bins: int = 10,
    embedding_net: nn.Module = nn.Identity(),
    **kwargs: Any,
) -> Callable[[Tensor, Tensor], nn.Module]:
    """Return a function that builds the posterior density estimator from (theta, x) batches."""
    model_fields = _MDN_FIELDS if model == "mdn" else _MODELS.get(model, _MODELS["nsf"])[1]
    known = {k: v for k, v in kwargs.items() if k in model_fields}
    unknown = {k: v for k, v in kwargs.items() if k not in model_fields}
    if unknown:
        warnings.warn(f"Unknown kwargs {sorted(unknown)} are forwarded to the builder.", UserWarning, stacklevel=2)

    def build_fn(batch_theta: Tensor, batch_x: Tensor):
        if model == "zuko_nsf":
            return ZukoNSFConfig(z_score_input=z_score_theta, z_score_condition=z_score_x,
                                 embedding_net=None if isinstance(embedding_net, nn.Identity) else embedding_net,
                                 hidden_features=hidden_features, num_transforms=num_transforms, num_bins=num_bins,
                                 extra_kwargs={**known, **unknown}).build(batch_theta, batch_x)
        if model == "mdn":
            if z_score_theta == "transform_to_unconstrained":
                raise NotImplementedError("sbi_amd: posterior_nn('mdn', z_score_theta='transform_to_unconstrained') is "
                                          "not implemented. Use one of 'none', 'independent', 'structured'.")
            return MDNConfig(z_score_input=z_score_theta, z_score_condition=z_score_x,
                             embedding_net=None if isinstance(embedding_net, nn.Identity) else embedding_net,
                             hidden_features=hidden_features, extra_kwargs=unknown, **known).build(batch_theta, batch_x)
        if model == "mdn_snpe_a":
            raise NotImplementedError("sbi_amd: 'mdn_snpe_a' (the mixture density network of NPE-A, whose last layer is "
                                      "trained with more components in the final round) is not implemented; NPE-A "
                                      "itself is not either. Use posterior_nn('mdn') with single-round NPE.")
        if model == "made":
            raise NotImplementedError("sbi_amd: 'made' (MADE with a mixture-of-Gaussians output, MADE-MoG) is not "
                                      "implemented. Use 'mdn', 'nsf', 'maf_rqs' or 'zuko_nsf'.")
        if model not in _MODELS:
            raise NotImplementedError(
                f"sbi_amd implements the 'nsf', 'maf_rqs', 'zuko_nsf' and 'mdn' posterior estimators (got model={model!r}); other "
                "model families are outside the accelerated path."
            )
        cfg = _MODELS[model][0](
            z_score_input=z_score_theta, z_score_condition=z_score_x,
            embedding_net=None if isinstance(embedding_net, nn.Identity) else embedding_net,
            hidden_features=hidden_features, num_transforms=num_transforms, num_bins=num_bins,
            extra_kwargs=unknown, **known,
        )
        return cfg.build(batch_theta, batch_x)

    return build_fn


def likelihood_nn(
    model: str,
    z_score_theta: Optional[str] = "independent",
    z_score_x: Optional[str] = "independent",
    hidden_features: int = 50,
    num_transforms: int = 5,
    num_bins: int = 10,
    embedding_net: nn.Module = nn.Identity(),
    **kwargs: Any,
) -> Callable[[Tensor, Tensor], nn.Module]:
    """Return ``build_fn(batch_theta, batch_x)`` for a LIKELIHOOD estimator q(x | theta) (sbi/neural_nets/factory.py:
    244-315): the NSF with x as the flow input and theta as the condition (z_score_x z-scores the input,
    z_score_theta the condition, `embedding_net` embeds theta).  Only ``model="nsf"`` runs on the kernels; sbi's other
    likelihood models (its default affine "maf", "mdn", "made", "maf_rqs", the zuko flows) are refused here."""
    if model == "mnle":      # mixed discrete / continuous data (factory.py: model_builders["mnle"] = build_mnle)
        from sbi_amd.neural_nets.net_builders.mixed_nets import build_mnle

        mixed_kwargs = dict(kwargs)

        def build_mixed(batch_theta: Tensor, batch_x: Tensor):
            return build_mnle(batch_x=batch_x, batch_y=batch_theta, z_score_x=z_score_x, z_score_y=z_score_theta,
                              hidden_features=hidden_features, num_transforms=num_transforms, num_bins=num_bins,
                              embedding_net=embedding_net, **mixed_kwargs)

        return build_mixed
    if model != "nsf":
        raise NotImplementedError(
            f"sbi_amd implements the 'nsf' likelihood estimator only (got model={model!r}); other model families are "
            "outside the accelerated path. Use likelihood_nn('nsf')."
        )
    known = {k: v for k, v in kwargs.items() if k in _NSF_FIELDS}
    unknown = {k: v for k, v in kwargs.items() if k not in _NSF_FIELDS}
    if unknown:
        warnings.warn(f"Unknown kwargs {sorted(unknown)} are forwarded to the builder.", UserWarning, stacklevel=2)

    def build_fn(batch_theta: Tensor, batch_x: Tensor):
        cfg = NSFConfig(
            z_score_input=z_score_x, z_score_condition=z_score_theta,
            embedding_net=None if isinstance(embedding_net, nn.Identity) else embedding_net,
            hidden_features=hidden_features, num_transforms=num_transforms, num_bins=num_bins,
            extra_kwargs=unknown, **known,
        )
        return cfg.build(batch_x, batch_theta)

    return build_fn


def posterior_flow_nn(*args, **kwargs):
    """``sbi.neural_nets.posterior_flow_nn`` (factory.py:531-620) for the FMPE path; see
    ``sbi_amd.inference.trainers.vfpe.fmpe.posterior_flow_nn`` (imported lazily: it needs the trainer package)."""
    from sbi_amd.inference.trainers.vfpe.fmpe import posterior_flow_nn as _impl

    return _impl(*args, **kwargs)


def posterior_score_nn(*args, **kwargs):
    """``sbi.neural_nets.posterior_score_nn`` for the NPSE path (default MLP; ``sde_type`` "ve" | "vp" | "subvp"); see
    ``sbi_amd.inference.trainers.vfpe.npse.posterior_score_nn`` (imported lazily: it needs the trainer package)."""
    from sbi_amd.inference.trainers.vfpe.npse import posterior_score_nn as _impl

    return _impl(*args, **kwargs)


def build_score_matching_estimator(*args, **kwargs):
    """``build_vector_field_estimator(..., estimator_type="score")`` for the configuration family the kernels run."""
    from sbi_amd.neural_nets.estimators.score_estimator import build_score_matching_estimator as _impl

    return _impl(*args, **kwargs)


_RESNET_FIELDS = {"num_blocks", "dropout_probability", "use_batch_norm"}


def classifier_nn(
    model: str,
    z_score_theta: Optional[str] = "independent",
    z_score_x: Optional[str] = "independent",
    hidden_features: int = 50,
    embedding_net_theta: nn.Module = nn.Identity(),
    embedding_net_x: nn.Module = nn.Identity(),
    **kwargs: Any,
) -> Callable[[Tensor, Tensor], nn.Module]:
    """Return ``build_fn(batch_theta, batch_x)`` for NRE's ratio classifier (sbi/neural_nets/factory.py:174-235).  Only
    ``model="resnet"`` (sbi's default, ``ResNetClassifierConfig``) runs on the kernels; "linear" and "mlp", dropout,
    batch norm and non-identity embedding nets are refused with ``NotImplementedError``."""
    if model != "resnet":
        raise NotImplementedError(
            f"sbi_amd implements the 'resnet' ratio classifier only (got model={model!r}); the 'linear' and 'mlp' "
            "classifiers are outside the accelerated path. Use classifier_nn('resnet')."
        )
    known = {k: v for k, v in kwargs.items() if k in _RESNET_FIELDS}
    unknown = {k: v for k, v in kwargs.items() if k not in _RESNET_FIELDS}
    if unknown:
        warnings.warn(f"Unknown kwargs {sorted(unknown)} are ignored by the 'resnet' classifier.", UserWarning,
                      stacklevel=2)
    cfg = ResNetClassifierConfig(
        z_score_input=z_score_theta, z_score_condition=z_score_x,
        embedding_net_theta=None if isinstance(embedding_net_theta, nn.Identity) else embedding_net_theta,
        embedding_net_x=None if isinstance(embedding_net_x, nn.Identity) else embedding_net_x,
        hidden_features=hidden_features, **known,
    )
    return cfg.build
