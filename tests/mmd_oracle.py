"""fp64 oracle of the RBF two-sample sums and the MMD estimators (TEST INFRASTRUCTURE: only tests import this).

The written formula -- cdist -> median -> exp -> sums / means -- evaluated in float64 on the rows it is given.  The real
sbi.diagnostics.misspecification cannot be imported where this suite is built (skorch is missing), so no golden comes
from a run of the reference; this restatement is the yardstick."""
import math

import torch

from tests.shuffle_restatement import prp

M64 = 0xFFFFFFFFFFFFFFFF


def key(seed: int, t: int) -> int:
    """key(seed, t) of include/sbi_amd_mmd.h (splitmix64's output function), in Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (t + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def split_rows(N: int, M: int, seed: int, s: int):
    """The pool rows of split s, one Python `prp` call per position."""
    k = key(seed, s)
    return [prp(j, N, k) for j in range(M)]


def _lower(d):
    ix = torch.tril_indices(d.shape[0], d.shape[1], offset=-1)
    return d[ix[0], ix[1]]


def sums(rows: torch.Tensor, n_a: int, pair_set: int, median_set: int, bandwidth=None, bw_floor: float = 0.0):
    """[bw, S_aa, S_bb, S_ab] in float64 (a (4,) tensor) for one split's rows (M, D)."""
    r = rows.detach().cpu().double()
    a, b = r[:n_a], r[n_a:]
    # (distances from differences also here: through the Gram form a float64 diagonal is sqrt(rounding noise), not 0)
    cd = lambda x, y: torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist")
    dab, daa, dbb = cd(a, b).reshape(-1), cd(a, a), cd(b, b)
    daa = _lower(daa) if pair_set else daa.reshape(-1)
    dbb = _lower(dbb) if pair_set else dbb.reshape(-1)
    if bandwidth is None:
        pop = torch.cat((dab, daa, dbb)) if median_set else dab
        bw = max(bw_floor, torch.median(pop).item())
    else:
        bw = float(bandwidth)
    k = lambda d: torch.exp(-(d**2) / (2.0 * bw**2)).sum().item()
    return torch.tensor([bw, k(daa), k(dbb), k(dab)], dtype=torch.float64)


def mmd_from_sums(s, n_a: int, n_b: int, mode: str) -> float:
    """sbi/diagnostics/misspecification.py's compute_rbf_mmd from sums that include the diagonals."""
    if mode == "biased":
        return float(s[1] / n_a**2 + s[2] / n_b**2 - 2 * s[3] / (n_a * n_b))
    return float(s[1] / (n_a * (n_a - 1)) + s[2] / (n_b * (n_b - 1)) - 2 * s[3] / (n_a * n_b))


def misspecification_mmd(a: torch.Tensor, b: torch.Tensor, mode: str = "biased") -> float:
    """compute_rbf_mmd_median_heuristic in float64."""
    s = sums(torch.cat((a, b)), a.shape[0], 0, 0)
    return mmd_from_sums(s, a.shape[0], b.shape[0], mode)


def biased_mmd(x, y, scale=None) -> float:
    nx, ny = x.shape[0], y.shape[0]
    s = sums(torch.cat((x, y)), nx, 0, 1, bandwidth=scale)
    return math.sqrt(float(s[1] / nx**2 - 2 * s[3] / (nx * ny) + s[2] / ny**2))


def unbiased_mmd_squared(x, y, scale=None) -> float:
    nx, ny = x.shape[0], y.shape[0]
    s = sums(torch.cat((x, y)), nx, 1, 1, bandwidth=None if scale is None else max(scale, 1e-8), bw_floor=1e-8)
    return float(2 * (s[1] / (nx * (nx - 1)) + s[2] / (ny * (ny - 1)) - s[3] / (nx * ny)))
