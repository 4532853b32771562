from sbi_amd.samplers.vi.vi_divergence_optimizers import (DivergenceOptimizer, ElboOptimizer,  # noqa: F401
                                                          ForwardKLOptimizer, IWElboOptimizer,
                                                          RenyiDivergenceOptimizer, get_default_VI_method,
                                                          get_VI_method)
from sbi_amd.samplers.vi.vi_quality_control import basic_checks, get_quality_metric  # noqa: F401
from sbi_amd.samplers.vi.vi_utils import (AdaptedVariationalDistribution, LearnableGaussian,  # noqa: F401
                                          link_descriptor)
