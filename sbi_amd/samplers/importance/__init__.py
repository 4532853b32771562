from sbi_amd.samplers.importance.importance_sampling import (exponentiate_weights, gpdfit, importance_sample,  # noqa: F401
                                                               largest_weight_indices)  # noqa: F401
from sbi_amd.samplers.importance.sir import sampling_importance_resampling, sir_select  # noqa: F401
