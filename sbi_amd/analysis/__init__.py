"""Posterior analysis (sbi.analysis): conditional densities and correlations.  Plotting is not part of this package."""

from sbi_amd.analysis.conditional_density import (ConditionedMDN, conditional_corrcoeff, conditional_density_grids,
                                                  conditional_potential, eval_conditional_density)

__all__ = ["ConditionedMDN", "conditional_corrcoeff", "conditional_density_grids", "conditional_potential",
           "eval_conditional_density"]
