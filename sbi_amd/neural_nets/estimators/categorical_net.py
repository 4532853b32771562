"""Categorical part of the mixed estimator (sbi/neural_nets/estimators/categorical_net.py).

``CategoricalMassEstimator`` here is the discrete VIEW of a ``MixedDensityEstimator``: log_prob / sample of the
``CategoricalMADE`` term alone, evaluated by the MNLE kernels with the discrete bit of their ``parts`` mask
(include/sbi_amd_mnle.h).  A stand-alone categorical estimator is not built by this package: build the mixed estimator
(``build_mnle``) and use its ``.discrete_net``."""

from sbi_amd.neural_nets.estimators.mixed_density_estimator import (MAX_CATEGORIES, _PartView as CategoricalMassEstimator,
                                                                    map_values_to_indices)

__all__ = ["CategoricalMassEstimator", "MAX_CATEGORIES", "map_values_to_indices"]
