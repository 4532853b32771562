from sbi_amd.inference.abc.mcabc import MCABC  # noqa: F401
from sbi_amd.inference.abc.smcabc import SMCABC  # noqa: F401
