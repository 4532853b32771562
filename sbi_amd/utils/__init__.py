from sbi_amd.utils.torchutils import BoxUniform  # noqa: F401
from sbi_amd.utils.restriction_estimator import RestrictedPrior, get_density_thresholder  # noqa: F401
