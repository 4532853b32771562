"""fp64 oracle of the ABC kernels and formulas (TEST INFRASTRUCTURE: only tests import this).

The real sbi does not import where this suite is built (nflows, zuko and pyro are missing), so no fixture can come from
a run of the reference.  These are restatements in float64, written from the published formulas, of: the pairwise
mixture log-density in both modes (include/sbi_amd_abc.h), the log-domain Sinkhorn iteration with per-problem freezing,
the SMC-ABC weight formula, scikit-learn's Gaussian KDE log-density and np.cov(aweights=)."""
import math

import torch


def mixture_lse(q, c, log_w=None, whiten=None, half_width=None, scale=None, q_group=None, c_group=None):
    """(H, M) float64.  Gaussian: log sum_j exp(log_w_j - scale_h |A (q_i - c_j)|^2 / 2).  Box: log sum over the centres
    with c_j - v <= q_i < c_j + v of exp(log_w_j), the bounds formed in float32 as the kernel's contract says (the test
    inputs lie on a dyadic grid, where float32 and float64 agree).  Leave-group-out when both groups are given."""
    q64, c64 = q.detach().cpu().double(), c.detach().cpu().double()
    M, N = q64.shape[0], c64.shape[0]
    lw = torch.zeros(N, dtype=torch.float64) if log_w is None else log_w.detach().cpu().double()
    if half_width is not None:
        v = half_width.detach().cpu().float()
        lo, hi = (c.detach().cpu().float() - v).double(), (c.detach().cpu().float() + v).double()
        inside = ((lo[None] <= q64[:, None]) & (q64[:, None] < hi[None])).all(-1)
        t = torch.where(inside, lw[None, :], torch.full((1, 1), -math.inf, dtype=torch.float64))[None]
    else:
        diff = q64[:, None, :] - c64[None, :, :]
        if whiten is not None:
            diff = diff @ whiten.detach().cpu().double().T
        d2 = (diff**2).sum(-1)
        t = lw[None, None, :] - 0.5 * scale.detach().cpu().double()[:, None, None] * d2[None]
    if q_group is not None and c_group is not None:
        same = q_group.cpu()[:, None] == c_group.cpu()[None, :]
        t = torch.where(same[None], torch.full((1, 1, 1), -math.inf, dtype=torch.float64), t)
    return torch.logsumexp(t, dim=-1)


def squared_distances(x, y):
    return ((x.double().unsqueeze(-2) - y.double().unsqueeze(-3)) ** 2).sum(-1)


def sinkhorn(cost, a, b, eps, max_iter, tol, dtype=torch.float64):
    """(f, g, w, iters) of B problems in `dtype`: f from the old g, g from the new f; a problem stops after the first
    iteration with max(sum |df|, sum |dg|) < tol (its update kept) or after max_iter; iters = iterations executed;
    w = sum exp(-(C - f - g) / eps) C."""
    cost, a, b = cost.to(dtype), a.to(dtype), b.to(dtype)
    f, g = torch.zeros_like(a), torch.zeros_like(b)
    la, lb = torch.log(a), torch.log(b)
    iters = torch.zeros(cost.shape[0], dtype=torch.int64)
    live = torch.ones(cost.shape[0], dtype=torch.bool)
    for _ in range(max_iter):
        fn = f + eps * (la - torch.logsumexp((f[:, :, None] + g[:, None, :] - cost) / eps, dim=2))
        gn = g + eps * (lb - torch.logsumexp((fn[:, :, None] + g[:, None, :] - cost) / eps, dim=1))
        err = torch.maximum((f - fn).abs().sum(1), (g - gn).abs().sum(1))
        f, g = torch.where(live[:, None], fn, f), torch.where(live[:, None], gn, g)      # a stopped problem is frozen
        iters += live
        live = live & ~(err < tol)
        if not live.any():
            break
    w = (torch.exp((f[:, :, None] + g[:, None, :] - cost) / eps) * cost).sum(dim=(1, 2))
    return f, g, w, iters


def gaussian_log_mixture(new, old, old_log_w, cov):
    """log sum_j w_j N(new_i; old_j, cov), float64, from the multivariate normal density itself."""
    new64, old64, cov64 = new.detach().cpu().double(), old.detach().cpu().double(), cov.detach().cpu().double()
    D = new64.shape[1]
    diff = new64[:, None, :] - old64[None, :, :]
    maha = torch.einsum("ijd,de,ije->ij", diff, torch.linalg.inv(cov64), diff)
    log_n = -0.5 * maha - 0.5 * torch.logdet(cov64) - 0.5 * D * math.log(2 * math.pi)
    return torch.logsumexp(old_log_w.detach().cpu().double()[None, :] + log_n, dim=1)


def uniform_log_mixture(new, old, old_log_w, half_width):
    """log sum_j w_j U(new_i; old_j - v, old_j + v), float64 (density 1 / prod 2 v on [low, high))."""
    v = half_width.detach().cpu().float()
    lo, hi = (old.detach().cpu().float() - v).double(), (old.detach().cpu().float() + v).double()
    n64 = new.detach().cpu().double()
    inside = ((lo[None] <= n64[:, None]) & (n64[:, None] < hi[None])).all(-1)
    t = torch.where(inside, old_log_w.detach().cpu().double()[None, :], torch.tensor(-math.inf, dtype=torch.float64))
    return torch.logsumexp(t, dim=1) - torch.log(2 * v.double()).sum()


def smc_log_weights(prior_log_prob, new, old, old_log_w, kernel_variance, kernel="gaussian"):
    """Normalised new log-weights: prior(new_i) / sum_j w_j K(new_i; old_j)."""
    mix = gaussian_log_mixture(new, old, old_log_w, kernel_variance) if kernel == "gaussian" else \
        uniform_log_mixture(new, old, old_log_w, kernel_variance)
    lw = prior_log_prob.detach().cpu().double() - mix
    return lw - torch.logsumexp(lw, dim=0)


def kde_log_density(x, samples, bandwidth, weights=None):
    """scikit-learn's KernelDensity(kernel="gaussian", bandwidth=h).fit(samples, sample_weight).score_samples(x)."""
    x64, s64 = x.detach().cpu().double(), samples.detach().cpu().double()
    N, D = s64.shape
    w = torch.ones(N, dtype=torch.float64) if weights is None else weights.detach().cpu().double()
    d2 = ((x64[:, None, :] - s64[None, :, :]) ** 2).sum(-1)
    return (torch.logsumexp(torch.log(w)[None, :] - d2 / (2 * bandwidth**2), dim=1) - torch.log(w.sum())
            - D * math.log(bandwidth) - 0.5 * D * math.log(2 * math.pi))


def fold_bounds(n, k):
    """[(start, stop)] of KFold(k)'s contiguous unshuffled folds: the first n % k one longer."""
    out, start = [], 0
    for f in range(k):
        size = n // k + (1 if f < n % k else 0)
        out.append((start, start + size))
        start += size
    return out


def cv_score_table(samples, bandwidths, k):
    """(H, k) float64: the held-out sum of log-densities per (bandwidth, fold), fold by fold from kde_log_density."""
    n = samples.shape[0]
    table = torch.empty((len(bandwidths), k), dtype=torch.float64)
    for f, (s, e) in enumerate(fold_bounds(n, k)):
        train = torch.cat((samples[:s], samples[e:]))
        for h, bw in enumerate(bandwidths):
            table[h, f] = kde_log_density(samples[s:e], train, float(bw)).sum()
    return table


def weighted_covariance(x, w):
    """np.cov(x, rowvar=False, aweights=w) in float64, through numpy itself."""
    import numpy as np

    return torch.from_numpy(np.atleast_2d(np.cov(x.detach().cpu().double().numpy(), rowvar=False,
                                                 aweights=w.detach().cpu().double().numpy())))
