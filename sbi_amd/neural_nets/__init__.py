from sbi_amd.neural_nets.factory import (build_score_matching_estimator, classifier_nn, likelihood_nn,  # noqa: F401
                                          posterior_flow_nn, posterior_nn, posterior_score_nn)
from sbi_amd.neural_nets.net_builders.estimator_configs import (MAFRQSConfig, MDNConfig, MixedConfig,  # noqa: F401
                                                                NSFConfig,
                                                                ResNetClassifierConfig, ZukoNSFConfig)
