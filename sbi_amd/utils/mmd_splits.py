"""RBF-kernel sums of S two-sample problems ("splits") over one pool of rows: the engine under the misspecification
test (sbi_amd/diagnostics/misspecification.py) and the MMD metrics (sbi_amd/utils/metrics.py).

`rbf_splits` returns, per split, `[bw, S_aa, S_bb, S_ab]` as include/sbi_amd_mmd.h defines them.  A pool on a ROCm
device inside the kernel's envelope is ONE launch of `sbi_amd_mmd_rbf_splits` for all splits.  Everything else -- host
tensors, or a shape the kernel refuses (M * (D | 1) > 15 360 floats of LDS staging) -- runs `rbf_splits_torch`, the same
splits as an eager-torch composition of the formula, with distances from differences as in the kernel.  The splits are
selected by the kernel's keyed permutation (csrc/shuffle_prp.h), evaluated here for all (split, position) pairs at once,
so a seed picks the same rows on both routes.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

STAGE_FLOATS = 15_360       # SBI_AMD_MMD_STAGE_FLOATS of include/sbi_amd_mmd.h
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def split_key(seed: int, t: int) -> int:
    """key(seed, t) of include/sbi_amd_mmd.h: splitmix64's output function on seed + (t + 1) * golden."""
    z = (seed + 0x9E3779B97F4A7C15 * (t + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _half_bits(n: int) -> int:
    bits = 2
    while bits < 32 and (1 << bits) < n:
        bits += 1
    return (bits + 1) // 2


def _mul32(v: Tensor, c: int) -> Tensor:
    """(v * c) mod 2^32 for 0 <= v < 2^32 held in int64, without leaving the int64 range."""
    lo = (v & 0xFFFF) * c
    hi = (((v >> 16) * c) & 0xFFFF) << 16
    return (lo + hi) & _M32


def _mix(v: Tensor) -> Tensor:
    v = v ^ (v >> 16)
    v = _mul32(v, 0x85EBCA6B)
    v = v ^ (v >> 13)
    v = _mul32(v, 0xC2B2AE35)
    return v ^ (v >> 16)


def split_indices(N: int, M: int, seed: int, S: int, split_offset: int = 0, device=None) -> Tensor:
    """(S, M) int64: row j of split s is shf_prp(j, N, key(seed, s + split_offset)) -- the first M positions of a keyed
    permutation of [0, N), so the M rows of a split are distinct.  Vectorised over all S * M entries; the cycle walk
    repeats the network on the entries that still sit outside [0, N)."""
    if M > N:
        raise ValueError(f"a split of {M} rows cannot be drawn from a pool of {N}")
    hb = _half_bits(N)
    mask = (1 << hb) - 1
    keys = [split_key(seed, s + split_offset) for s in range(S)]
    k0 = torch.tensor([k & _M32 for k in keys], dtype=torch.int64, device=device).reshape(S, 1)
    k1 = torch.tensor([(k >> 32) & _M32 for k in keys], dtype=torch.int64, device=device).reshape(S, 1)
    v = torch.arange(M, dtype=torch.int64, device=device).reshape(1, M).expand(S, M).clone()
    pending = torch.ones((S, M), dtype=torch.bool, device=device)
    while True:
        l, r = v >> hb, v & mask
        for rnd in range(6):
            c = (0x9E3779B9 * (rnd + 1)) & _M32
            f = _mix((r + c + (k1 if rnd & 1 else k0)) & _M32) & mask
            l, r = r, l ^ f
        v = torch.where(pending, (l << hb) | r, v)
        pending = pending & (v >= N)
        if not bool(pending.any()):
            return v


def _dist(x: Tensor, y: Tensor) -> Tensor:
    # Euclidean distances from differences (never the |a|^2 + |b|^2 - 2 a.b form cdist switches to above 25 rows)
    return torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist")


def _lower(d: Tensor) -> Tensor:
    ix = torch.tril_indices(d.shape[0], d.shape[1], offset=-1, device=d.device)
    return d[ix[0], ix[1]]


def rbf_splits_torch(pool: Tensor, idx: Tensor, n_a: int, pair_set: int, median_set: int,
                     bandwidth: Optional[Tensor] = None, bw_floor: float = 0.0) -> Tensor:
    """The fallback: (S, 4) `[bw, S_aa, S_bb, S_ab]` for the splits `pool[idx[s]]`, one eager-torch evaluation of the
    written formula per split, in the pool's dtype, with the kernel's rules (lower median, non-finite rows give NaN,
    sums accumulated in fp64)."""
    S = idx.shape[0]
    out = torch.empty((S, 4), dtype=pool.dtype, device=pool.device)
    for s in range(S):
        rows = pool[idx[s]]
        if not bool(torch.isfinite(rows).all()):
            out[s] = float("nan")
            continue
        a, b = rows[:n_a], rows[n_a:]
        dab, daa, dbb = _dist(a, b).reshape(-1), _dist(a, a), _dist(b, b)
        daa = _lower(daa) if pair_set else daa.reshape(-1)
        dbb = _lower(dbb) if pair_set else dbb.reshape(-1)
        if bandwidth is not None:
            bw = bandwidth[s].to(pool.dtype)
        else:
            population = torch.cat((dab, daa, dbb)) if median_set else dab
            bw = torch.clamp(torch.median(population), min=bw_floor)
        inv = 1.0 / (2.0 * bw * bw)
        out[s, 0] = bw
        for k, d in enumerate((daa, dbb, dab)):
            out[s, k + 1] = torch.exp(-(d * d) * inv).sum(dtype=torch.float64).to(pool.dtype)
    return out


def rbf_splits(pool: Tensor, S: int, M: int, n_a: int, pair_set: int, median_set: int, idx: Optional[Tensor] = None,
               seed: int = 0, split_offset: int = 0, bandwidth: Optional[Tensor] = None,
               bw_floor: float = 0.0, force_fallback: bool = False) -> Tensor:
    """(S, 4) fp32 `[bw, S_aa, S_bb, S_ab]` on the pool's device.  pool (N, D); split s uses the rows idx[s] ((S, M)
    integers) or, with idx None, the keyed permutation of (seed, s + split_offset).  bandwidth: (S,) or None."""
    if pool.dim() != 2:
        raise ValueError(f"expected a (N, D) pool, got shape {tuple(pool.shape)}")
    N, D = pool.shape
    if not (M >= 2 and 1 <= n_a < M and D >= 1 and S >= 0):
        raise ValueError(f"need M >= 2, 1 <= n_a < M, D >= 1, S >= 0; got M={M}, n_a={n_a}, D={D}, S={S}")
    pool = pool.detach().to(torch.float32).contiguous()
    if bandwidth is not None:
        bandwidth = bandwidth.detach().to(device=pool.device, dtype=torch.float32).reshape(S).contiguous()
    if pool.is_cuda and not force_fallback and M * (D | 1) <= STAGE_FLOATS:
        from sbi_amd import _lib

        lib = _lib.load()
        idx32 = None if idx is None else idx.to(device=pool.device, dtype=torch.int32).reshape(S, M).contiguous()
        dev = _lib.require_device(pool, bandwidth)
        out = torch.empty((S, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.sbi_amd_mmd_rbf_splits(_lib.ptr(pool), N, D, _lib.ptr(idx32), int(seed) & _M64,
                                            int(split_offset), S, M, n_a, pair_set, median_set, _lib.ptr(bandwidth),
                                            float(bw_floor), _lib.ptr(out), _lib.current_stream(dev))
        if rc != _lib.E_UNSUPPORTED:
            _lib.check(rc, "mmd_rbf_splits")
            return out
    if idx is None:
        idx = split_indices(N, M, int(seed) & _M64, S, split_offset, device=pool.device)
    return rbf_splits_torch(pool, idx.to(device=pool.device, dtype=torch.int64).reshape(S, M), n_a, pair_set,
                            median_set, bandwidth, bw_floor)
