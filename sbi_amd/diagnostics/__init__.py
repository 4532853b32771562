"""Calibration diagnostics of a trained posterior: simulation-based calibration / expected coverage and TARP."""

from sbi_amd.diagnostics.sbc import (  # noqa: F401
    check_prior_vs_dap,
    check_sbc,
    check_uniformity_c2st,
    check_uniformity_frequentist,
    get_nltp,
    run_sbc,
)
from sbi_amd.diagnostics.tarp import check_tarp, get_tarp_references, run_tarp  # noqa: F401
