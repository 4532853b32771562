"""Sampling-importance-resampling (SIR).

Same loop as sbi/samplers/importance/sir.py:13-71: per iteration `batch_size x num_candidate_samples` proposal draws
with their log importance weights, one winner per row drawn in proportion to the weights, until `num_samples` winners
exist.  Rows whose weights cannot be normalised (a NaN, a +inf, or all -inf: the reference's softmax is all-NaN there
and its mask selects nothing) are dropped and the loop goes on.

MI355X-first: with candidates and weights on a ROCm device the selection -- subtract, softmax, cumsum, rand, compare,
second cumsum and a boolean-mask gather that synchronises, about nine launches -- is ONE launch of
`sbi_amd_sir_resample` (include/sbi_amd_sir.h).  The uniforms are drawn in the kernel (Philox keyed by a seed from
torch's generator, one stream position per row, advancing over the loop) and the only host read per iteration is the
dead-row count: in an iteration that had dead rows the live winners are gathered through a stable argsort of the dead
flag, cut at the count the host already knows (a boolean-mask gather would synchronise a second time).  A row of more
than 40 960 candidates does not fit the kernel's LDS staging and is refused.  Host tensors take the same steps as torch
operations (`_select_torch`), with the kernel's semantics.

Two deliberate departures from the reference's `cumsum(softmax) >= u`: a candidate of weight zero is never selected,
and a live row always selects (the reference can select nothing when rounding leaves the last cumulative weight below
u).  Both differ only for u exactly on a boundary.
"""

from __future__ import annotations

from typing import Any, Callable, Optional, Tuple

import torch
from torch import Tensor

from sbi_amd.samplers.importance.importance_sampling import importance_sample

MAX_DEVICE_CANDIDATES = 40_960      # SIR_LDS_MAX_K of csrc/sir.hip: a row is staged in one workgroup's LDS


def live_first(idx: Tensor, n_dead: int) -> Tuple[Tensor, Tensor]:
    """(positions of the live rows, positions of the dead rows), each in row order, from `idx` (-1 = dead) and the
    dead-row count the host already holds: sizes are known, so nothing here waits for the device."""
    order = torch.argsort((idx < 0).to(torch.int8), stable=True)
    n_live = idx.shape[0] - n_dead
    return order[:n_live], order[n_live:]


def _select_torch(log_weights: Tensor, candidates: Tensor, u: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """The kernel's selection rule as torch operations (any device): (winners (B, D), idx (B,) int32 with -1 for a dead
    row, row_lse (B,)).  Dead rows keep zeros in `winners`."""
    lw = log_weights
    B, K = lw.shape
    nan_row = torch.isnan(lw).any(dim=-1)
    m = torch.where(torch.isnan(lw), torch.full_like(lw, float("-inf")), lw).max(dim=-1).values
    dead = nan_row | torch.isinf(m)
    safe_m = torch.where(dead, torch.zeros_like(m), m)
    e = torch.exp(torch.where(dead.unsqueeze(-1), torch.full_like(lw, float("-inf")), lw) - safe_m.unsqueeze(-1))
    P = torch.cumsum(e, dim=-1)
    S = P[:, -1]
    pos = e > 0
    hit = pos & (P > (u.reshape(B).to(P.dtype) * S).unsqueeze(-1))
    first_hit = torch.argmax(hit.to(torch.int8), dim=-1)
    last_pos = K - 1 - torch.argmax(pos.flip(-1).to(torch.int8), dim=-1)
    idx = torch.where(hit.any(dim=-1), first_hit, last_pos)
    idx = torch.where(dead, torch.full_like(idx, -1), idx)
    gather = idx.clamp(min=0).reshape(B, 1, 1).expand(B, 1, candidates.shape[-1])
    winners = torch.gather(candidates, 1, gather).squeeze(1)
    winners = torch.where(dead.unsqueeze(-1), torch.zeros_like(winners), winners)
    row_lse = torch.where(dead, torch.where(nan_row, torch.full_like(m, float("nan")), m), m + torch.log(S))
    return winners, idx.to(torch.int32), row_lse


def sir_select(log_p: Tensor, log_q: Optional[Tensor], candidates: Tensor, u: Optional[Tensor] = None, seed: int = 0,
               row_offset: int = 0, return_lse: bool = False):
    """One winner per row.  log_p, log_q (or None = 0): (B, K); candidates: (B, K, D).  Returns
    (winners (B, D), idx (B,) int32 with -1 for a dead row, n_dead (a 1-element int32 tensor, not read here)[, row_lse]).
    The winners' rows of dead rows hold nothing meaningful: filter with `idx >= 0`.
    On a ROCm device this is one launch; `u` None draws the uniforms in the kernel from (seed, row + row_offset).  Host
    tensors run `_select_torch` and draw `u` with `torch.rand` when it is not given."""
    B, K = log_p.shape
    D = candidates.shape[-1]
    if candidates.shape[:2] != (B, K):
        raise ValueError(f"candidates must be (B, K, D) = ({B}, {K}, D); got {tuple(candidates.shape)}")
    if not log_p.is_cuda:
        lw = log_p if log_q is None else log_p - log_q
        if u is None:
            u = torch.rand(B)
        winners, idx, lse = _select_torch(lw.to(torch.float32), candidates, u.to(lw.device))
        n_dead = (idx < 0).sum().to(torch.int32).reshape(1)
        return (winners, idx, n_dead, lse) if return_lse else (winners, idx, n_dead)
    if K > MAX_DEVICE_CANDIDATES:
        raise NotImplementedError(f"sbi_amd: the SIR kernel takes at most {MAX_DEVICE_CANDIDATES} candidates per row "
                                  f"(a row is staged in LDS); got {K}. Use fewer candidates per draw.")
    from sbi_amd import _lib

    lib = _lib.load()
    log_p = log_p.to(torch.float32).contiguous()
    log_q = None if log_q is None else log_q.to(torch.float32).contiguous()
    cand = candidates.to(torch.float32).contiguous()
    u = None if u is None else u.to(torch.float32).reshape(B).contiguous()
    dev = _lib.require_device(log_p, log_q, cand, u)
    out = torch.empty((B, D), dtype=torch.float32, device=dev)        # (rows of dead rows are left unwritten)
    ints = torch.zeros(B + 1, dtype=torch.int32, device=dev)          # [idx (B) | n_dead]
    lse = torch.empty(B, dtype=torch.float32, device=dev) if return_lse else None
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_sir_resample(_lib.ptr(log_p), _lib.ptr(log_q), _lib.ptr(cand), B, K, D, _lib.ptr(u),
                                      int(seed), int(row_offset), _lib.ptr(out), _lib.ptr(ints),
                                      _lib.ptr(lse), ints[B:].data_ptr(), _lib.current_stream(dev))
    _lib.check(rc, "sir_resample")
    return (out, ints[:B], ints[B:], lse) if return_lse else (out, ints[:B], ints[B:])


def sampling_importance_resampling(potential_fn: Callable, proposal: Any, num_samples: int = 1,
                                   num_candidate_samples: int = 32, max_sampling_batch_size: int = 10_000,
                                   show_progress_bars: bool = False, device: str = "cpu", **kwargs) -> Tensor:
    """`num_samples` draws, each the winner among `num_candidate_samples` proposal draws, selected in proportion to
    `exp(potential_fn - proposal.log_prob)`; shape (num_samples, *event).  `device` is kept for signature compatibility
    only (the reference draws its uniforms there): the work happens where the proposal's draws and the weights live."""
    selected = []
    sampling_batch_size = min(num_samples, max_sampling_batch_size)
    num_remaining = num_samples
    seed: Optional[int] = None
    row_offset = 0
    pbar = None
    if show_progress_bars:
        try:
            from tqdm.auto import tqdm

            pbar = tqdm(total=num_samples, desc=f"Drawing {num_samples} posterior samples")
        except ImportError:
            pbar = None
    while num_remaining > 0:
        batch_size = min(sampling_batch_size, num_remaining)
        with torch.no_grad():
            thetas, log_weights = importance_sample(potential_fn, proposal=proposal,
                                                    num_samples=batch_size * num_candidate_samples)
            log_weights = log_weights.reshape(batch_size, num_candidate_samples)
            cand = thetas.reshape(batch_size, num_candidate_samples, -1)
            if cand.device != log_weights.device:
                cand = cand.to(log_weights.device)
            if seed is None and log_weights.is_cuda:      # (as the MCMC samplers: `torch.manual_seed` fixes the run)
                seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
            winners, idx, n_dead = sir_select(log_weights, None, cand, None, seed or 0, row_offset)
            row_offset += batch_size
            dead = int(n_dead.item())                        # the ONE host read of the iteration
            if dead > 0:
                winners = winners[live_first(idx, dead)[0]]
        selected.append(winners)
        num_remaining -= winners.shape[0]
        if pbar is not None:
            pbar.update(winners.shape[0])
    if pbar is not None:
        pbar.close()
    return torch.cat(selected) if selected else torch.empty(0)
