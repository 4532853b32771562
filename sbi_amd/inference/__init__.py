from sbi_amd.inference.posteriors.direct_posterior import DirectPosterior  # noqa: F401
from sbi_amd.inference.posteriors.importance_posterior import ImportanceSamplingPosterior  # noqa: F401
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior  # noqa: F401
from sbi_amd.inference.posteriors.npe_a_posterior import NPE_A_Posterior  # noqa: F401
from sbi_amd.inference.posteriors.rejection_posterior import RejectionPosterior  # noqa: F401
from sbi_amd.inference.posteriors.vi_posterior import VIPosterior  # noqa: F401
from sbi_amd.inference.trainers.nle.mnle import MNLE  # noqa: F401
from sbi_amd.inference.trainers.nle.nle import NLE, NLE_A, SNLE  # noqa: F401
from sbi_amd.inference.trainers.npe.npe import NPE, NPE_C, SNPE  # noqa: F401
from sbi_amd.inference.trainers.npe.npe_a import NPE_A, SNPE_A  # noqa: F401
from sbi_amd.inference.trainers.nre.nre import (AALR, BNRE, CNRE, NRE, NRE_A, NRE_B, NRE_C, SNRE, SNRE_A,  # noqa: F401
                                                SNRE_B, SNRE_C, SRE)
from sbi_amd.inference.trainers.vfpe.fmpe import FMPE, posterior_flow_nn  # noqa: F401
from sbi_amd.inference.trainers.vfpe.npse import NPSE, posterior_score_nn  # noqa: F401
from sbi_amd.inference.abc import MCABC, SMCABC  # noqa: F401
