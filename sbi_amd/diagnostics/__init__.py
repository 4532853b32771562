"""Calibration diagnostics of a trained posterior: simulation-based calibration / expected coverage, TARP and the local
classifier two-sample test (L-C2ST); and of the simulator against the data: the misspecification tests."""

from sbi_amd.diagnostics.lc2st import LC2ST, LC2ST_NF, LC2STScores, LC2STState, permute_data  # noqa: F401
from sbi_amd.diagnostics.misspecification import (  # noqa: F401
    calc_misspecification_logprob,
    calc_misspecification_mmd,
    calculate_baseline_mmd,
    calculate_p_misspecification,
    compute_rbf_mmd,
    compute_rbf_mmd_median_heuristic,
    median_heuristic,
    rbf_kernel,
)
from sbi_amd.diagnostics.sbc import (  # noqa: F401
    check_prior_vs_dap,
    check_sbc,
    check_uniformity_c2st,
    check_uniformity_frequentist,
    get_nltp,
    run_sbc,
)
from sbi_amd.diagnostics.tarp import check_tarp, get_tarp_references, run_tarp  # noqa: F401
