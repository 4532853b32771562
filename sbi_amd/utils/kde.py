"""Gaussian kernel density estimation for the ABC samplers (sbi/utils/kde.py `get_kde` / `KDEWrapper`), and the pairwise
mixture log-sum-exp all of ABC's density sums go through.

`mixture_lse` is the engine: on a ROCm device inside the kernel's envelope (D <= 32, H <= 16) ONE launch of
`sbi_amd_mixture_lse` (include/sbi_amd_abc.h); for host tensors and shapes outside the envelope `mixture_lse_torch`, the
eager composition of the same formula (distances from differences, points whitened once after the common offset).
Its users: the SMC-ABC weight update (sbi_amd/inference/abc/smcabc.py), `GaussianKDE.score_samples`, and the
cross-validated bandwidth search, where all points are queries and centres, the groups are fold ids and the H scales are
the 10 bandwidths of one zoom repetition -- one launch instead of 200 scikit-learn fits and scores.

The density is scikit-learn's convention for KernelDensity(kernel="gaussian"):
    log p(x) = logsumexp_j(log w_j - |x - c_j|^2 / (2 h^2)) - log sum_j w_j - D log h - (D / 2) log 2 pi.
There is no scikit-learn dependency at run time.
"""

from __future__ import annotations

import math
from typing import Optional, Union

import numpy as np
import torch
from torch import Tensor
from torch.distributions.transforms import IndependentTransform, identity_transform

MAX_D, MAX_H = 32, 16          # SBI_AMD_MLSE_MAX_D / SBI_AMD_MLSE_MAX_H of include/sbi_amd_abc.h
_LOG_2PI = math.log(2.0 * math.pi)


def mixture_lse_torch(q: Tensor, c: Tensor, log_w: Optional[Tensor] = None, whiten: Optional[Tensor] = None,
                      half_width: Optional[Tensor] = None, scale: Optional[Tensor] = None,
                      q_group: Optional[Tensor] = None, c_group: Optional[Tensor] = None) -> Tensor:
    """The fallback: (H, M) in q's dtype, the written formula as an eager-torch composition, queries in chunks."""
    M, D = q.shape
    N = c.shape[0]
    lw = torch.zeros(N, dtype=q.dtype, device=q.device) if log_w is None else log_w.to(q.dtype)
    grouped = q_group is not None and c_group is not None
    box = half_width is not None
    if box:
        zq, zc, H = q, c, 1
        lo, hi = c - half_width, c + half_width
    else:
        zq, zc = q - c[0], c - c[0]
        if whiten is not None:
            zq, zc = zq @ whiten.T, zc @ whiten.T
        H = scale.shape[0]
    out = torch.empty((H, M), dtype=q.dtype, device=q.device)
    chunk = max(1, (1 << 22) // max(1, N * D))
    for s in range(0, M, chunk):
        e = min(M, s + chunk)
        if box:
            qq = zq[s:e, None, :]
            inside = ((lo[None] <= qq) & (qq < hi[None])).all(-1)
            t = torch.where(inside, lw[None, :], torch.full_like(lw, -math.inf)[None, :])[None]
            t = torch.where(torch.isnan(zq[s:e]).any(-1)[None, :, None], torch.full_like(t, math.nan), t)
        else:
            d2 = ((zq[s:e, None, :] - zc[None, :, :]) ** 2).sum(-1)
            t = lw[None, None, :] - 0.5 * scale.to(q.dtype)[:, None, None] * d2[None]
        if grouped:
            same = q_group[s:e, None] == c_group[None, :]
            t = torch.where(same[None] & ~torch.isnan(t), torch.full_like(t, -math.inf), t)
        out[:, s:e] = torch.logsumexp(t, dim=-1)
    return out


def mixture_lse(q: Tensor, c: Tensor, log_w: Optional[Tensor] = None, whiten: Optional[Tensor] = None,
                half_width: Optional[Tensor] = None, scale: Optional[Tensor] = None,
                q_group: Optional[Tensor] = None, c_group: Optional[Tensor] = None,
                force_fallback: bool = False) -> Tensor:
    """(H, M) fp32 on q's device: out[h, i] = log sum_j exp(log_w_j - scale_h |A (q_i - c_j)|^2 / 2) over the centres
    of another group than the query's (Gaussian mode), or log sum of exp(log_w_j) over the centres whose box
    [c_j - v, c_j + v) holds q_i (box mode, `half_width` = v).  q (M, D), c (N, D), scale (H,)."""
    if q.dim() != 2 or c.dim() != 2 or q.shape[1] != c.shape[1] or c.shape[0] < 1:
        raise ValueError(f"expected (M, D) queries and (N >= 1, D) centres, got {tuple(q.shape)} and {tuple(c.shape)}")
    dev = q.device

    def f32(t):
        return None if t is None else torch.as_tensor(t, device=dev).detach().to(torch.float32).contiguous()

    def i32(t):
        return None if t is None else torch.as_tensor(t, device=dev).to(torch.int32).contiguous()

    q, c, log_w, whiten, half_width, scale = (f32(t) for t in (q, c, log_w, whiten, half_width, scale))
    q_group, c_group = i32(q_group), i32(c_group)
    if half_width is None:
        if scale is None:
            raise ValueError("Gaussian mode needs `scale`")
        scale = scale.reshape(-1)
    M, D = q.shape
    H = 1 if half_width is not None else scale.shape[0]
    if q.is_cuda and not force_fallback and D <= MAX_D and H <= MAX_H:
        from sbi_amd import _lib

        lib = _lib.load()
        _lib.require_device(q, c, log_w, whiten, half_width, scale)
        out = torch.empty((H, M), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.sbi_amd_mixture_lse(_lib.ptr(q), M, _lib.ptr(c), c.shape[0], D, _lib.ptr(log_w), _lib.ptr(whiten),
                                         _lib.ptr(half_width), _lib.ptr(scale), H, _lib.ptr(q_group),
                                         _lib.ptr(c_group), _lib.ptr(out), _lib.current_stream(dev))
        if rc != _lib.E_UNSUPPORTED:
            _lib.check(rc, "mixture_lse")
            return out
    return mixture_lse_torch(q, c, log_w, whiten, half_width, scale, q_group, c_group)


class GaussianKDE:
    """A fitted Gaussian KDE: `.bandwidth`, `.score_samples(x)` (log-density, fp32, on x's device) and `.sample(n)`.
    What scikit-learn's KernelDensity(kernel="gaussian").fit(samples, sample_weight) provides, on the samples' device."""

    def __init__(self, samples: Tensor, bandwidth: float, sample_weights: Optional[Tensor] = None):
        if not float(bandwidth) > 0:
            raise ValueError("bandwidth must be positive")
        self.samples = samples.detach().to(torch.float32).contiguous()
        self.bandwidth = float(bandwidth)
        self.weights = None
        if sample_weights is not None:
            w = torch.as_tensor(sample_weights, device=self.samples.device).detach().to(torch.float32).reshape(-1)
            if w.shape[0] != self.samples.shape[0]:
                raise ValueError("sample_weights must have one entry per sample")
            if bool((w <= 0).any()):
                raise ValueError("sample_weight must have positive values")
            self.weights = w

    def score_samples(self, x: Tensor, force_fallback: bool = False) -> Tensor:
        x = torch.as_tensor(x, device=self.samples.device).to(torch.float32)
        N, D = self.samples.shape
        h = self.bandwidth
        scale = torch.tensor([1.0 / (h * h)], dtype=torch.float32, device=x.device)
        if self.weights is None:
            log_w, log_norm = None, math.log(N)
        else:
            log_w, log_norm = torch.log(self.weights), float(torch.log(self.weights.double().sum()))
        lse = mixture_lse(x.reshape(-1, D), self.samples, log_w=log_w, scale=scale, force_fallback=force_fallback)[0]
        return lse - (log_norm + D * math.log(h) + 0.5 * D * _LOG_2PI)

    def sample(self, n_samples: int = 1) -> Tensor:
        n = int(n_samples[0]) if isinstance(n_samples, (tuple, list, torch.Size)) else int(n_samples)
        N = self.samples.shape[0]
        if self.weights is None:
            idx = torch.randint(N, (n,), device=self.samples.device)
        else:
            idx = torch.multinomial(self.weights, n, replacement=True)
        return self.samples[idx] + self.bandwidth * torch.randn((n, self.samples.shape[1]), device=self.samples.device)


class KDEWrapper:
    """Sampling and evaluation with a KDE fitted on transformed parameters: the inverse transform on samples, the
    transform's log-abs-det Jacobian on log_prob."""

    def __init__(self, kde: GaussianKDE, transform):
        self.kde = kde
        self.transform = transform

    def sample(self, *args, **kwargs) -> Tensor:
        return self.transform.inv(self.kde.sample(*args, **kwargs))

    def log_prob(self, parameters_constrained: Tensor) -> Tensor:
        parameters_constrained = torch.as_tensor(parameters_constrained, device=self.kde.samples.device)
        parameters_unconstrained = self.transform(parameters_constrained)
        log_probs = self.kde.score_samples(parameters_unconstrained)
        log_probs = log_probs + self.transform.log_abs_det_jacobian(parameters_constrained, parameters_unconstrained)
        assert log_probs.numel() == parameters_constrained.shape[0], (
            "batch shape mismatch, log_abs_det_jacobian not summing over event dimensions?")
        return log_probs


def kfold_ids(n: int, k: int, device=None) -> Tensor:
    """(n,) int32 fold of every row for contiguous unshuffled folds as KFold(k) makes them: the first n % k folds hold
    n // k + 1 rows, the others n // k."""
    if not 2 <= k <= n:
        raise ValueError(f"Cannot have number of splits n_splits={k} greater than the number of samples: n_samples={n}."
                         if k > n else "k-fold cross-validation requires at least one train/test split")
    sizes = torch.full((k,), n // k, dtype=torch.int64)
    sizes[: n % k] += 1
    return torch.repeat_interleave(torch.arange(k, dtype=torch.int32), sizes).to(device)


def cv_score_table(samples: Tensor, bandwidths, num_partitions: int, force_fallback: bool = False) -> Tensor:
    """(H, k) fp64: entry (h, f) is the sum over the rows of fold f of their log-density under the unweighted KDE of
    bandwidth h fitted on the other folds.  A non-positive bandwidth (scikit-learn refuses it; the search then scores
    NaN) gives a row of NaN.  One `mixture_lse` call per 16 bandwidths."""
    x = samples.detach().to(torch.float32).contiguous()
    n, D = x.shape
    bw = torch.as_tensor(np.asarray(bandwidths, dtype=np.float64))
    ok = bw > 0
    folds = kfold_ids(n, num_partitions, device=x.device)
    sizes = torch.bincount(folds.long(), minlength=num_partitions)
    log_train = torch.log((n - sizes[folds.long()]).double())                       # (n,)
    h = torch.where(ok, bw, torch.ones_like(bw))
    table = torch.empty((bw.shape[0], num_partitions), dtype=torch.float64, device=x.device)
    for s in range(0, bw.shape[0], MAX_H):
        hh = h[s:s + MAX_H].to(x.device)
        lse = mixture_lse(x, x, scale=(1.0 / (hh * hh)).float(), q_group=folds, c_group=folds,
                          force_fallback=force_fallback).double()
        dens = lse - log_train[None, :] - D * torch.log(hh)[:, None] - 0.5 * D * _LOG_2PI
        part = torch.zeros((hh.shape[0], num_partitions), dtype=torch.float64, device=x.device)
        part.index_add_(1, folds.long(), dens)
        table[s:s + MAX_H] = part
    table[~ok.to(x.device)] = math.nan
    return table


def _ranks(scores: np.ndarray) -> np.ndarray:
    """Competition ("min") ranks of the scores, best first, NaN last -- GridSearchCV's rank_test_score."""
    s = np.asarray(scores, dtype=np.float64).copy()
    if np.isnan(s).all():
        return np.ones(len(s), dtype=np.int32)
    s[np.isnan(s)] = np.nanmin(s) - 1
    return np.array([1 + int((s > v).sum()) for v in s], dtype=np.int32)


def cv_bandwidth(samples: Tensor, num_cv_partitions: int = 20, num_cv_repetitions: int = 5,
                 force_fallback: bool = False, trace: Optional[list] = None) -> float:
    """The reference's zoom search as it behaves: 10 bandwidths between 0.1 and 0.5 standard deviations (of all
    entries), scored by k-fold cross-validation; zoom between the best and the second best; stop when the best score
    moves by no more than 1e-3.  At the lower end of the grid the reference re-centres on the best INDEX (0), not
    the best bandwidth, so the next grid runs from (upper - lower) / 10 down to its negative; the non-positive half
    scores NaN and ranks last.  The first best bandwidth of the last grid evaluated wins.  `trace` (tests, tools)
    collects (grid, mean scores) of every repetition."""
    std = float(samples.detach().cpu().double().std(unbiased=False))      # (on the host: the same grid on every route)
    steps = 10
    lower, upper = 0.1 * std, 0.5 * std
    current_best = -10000000.0
    selected = None
    for _ in range(num_cv_repetitions):
        grid = np.linspace(lower, upper, steps)
        mean_scores = cv_score_table(samples, grid, num_cv_partitions, force_fallback).mean(dim=1).cpu().numpy()
        if trace is not None:
            trace.append((grid, mean_scores))
        rank = _ranks(mean_scores)
        best = int(rank.argmin())
        selected = float(grid[best])
        if abs(current_best - mean_scores[best]) > 0.001:
            current_best = mean_scores[best]
        else:
            break
        second = list(rank).index(2)
        if best == 0 or best == steps:
            diff = (lower - upper) / steps
            lower, upper = best - diff, best + diff
        else:
            upper, lower = grid[second], grid[best]
            if upper < lower:
                upper, lower = lower, upper
    return selected


def get_kde(samples: Tensor, bandwidth: Union[float, str] = "cv", transform=None,
            sample_weights: Optional[Tensor] = None, num_cv_partitions: int = 20,
            num_cv_repetitions: int = 5) -> KDEWrapper:
    """KDE with the selected bandwidth: 'scott', 'silvermann', a positive float, or 'cv' (a cross-validated zoom
    search on the unweighted samples).  `transform` is applied before the KDE; `sample_weights` weight the samples of
    the final fit."""
    transform_ = identity_transform if transform is None else transform
    if transform_.event_dim == 0:     # the log-abs-det must sum over the parameter dimension
        transform_ = IndependentTransform(transform_, reinterpreted_batch_ndims=1)
    if isinstance(bandwidth, str):
        assert bandwidth in ["cv", "scott", "silvermann"], "invalid kde bandwidth name."
    transformed = transform_(samples)
    num_samples, dim_samples = transformed.shape
    if bandwidth == "scott":
        selected = num_samples ** (-1.0 / (dim_samples + 4))
    elif bandwidth == "silvermann":
        selected = (num_samples * (dim_samples + 2) / 4.0) ** (-1.0 / (dim_samples + 4))
    elif bandwidth == "cv":
        selected = cv_bandwidth(transformed, num_cv_partitions, num_cv_repetitions)
    elif float(bandwidth) > 0:
        selected = float(bandwidth)
    else:
        raise ValueError("bandwidth must be positive, 'scott', 'silvermann' or 'cv'")
    return KDEWrapper(GaussianKDE(transformed, selected, sample_weights), transform_)
