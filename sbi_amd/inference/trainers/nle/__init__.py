from sbi_amd.inference.trainers.nle.nle import NLE, NLE_A, SNLE  # noqa: F401
