from sbi_amd.inference.posteriors.vi_posterior import VIPosterior  # noqa: F401
