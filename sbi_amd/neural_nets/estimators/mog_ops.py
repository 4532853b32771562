"""Mixture-of-Gaussians algebra behind NPE-A: the analytic proposal correction, ``log_prob`` and ``sample`` of an
arbitrary mixture (include/sbi_amd_mog.h).

Routing: float32 tensors on a ROCm device inside the kernels' envelope (theta-dim <= 16, <= 65 536 components per
mixture row) go to ``sbi_amd_mog_correct`` / ``sbi_amd_mog_log_prob`` / ``sbi_amd_mog_sample``; host tensors, other
dtypes and anything outside the envelope run the same formulas as eager torch (the ``*_eager`` functions, which the
tests and ``tools/bench_npe_a.py`` also call directly).

Formulas (Papamakarios & Murray 2016, Eqs. 23-26; sbi's ``_correct_for_proposal`` / ``_compute_posterior_logits``),
component j = l K + k pairing proposal component l with density component k:

    S     = P_d - P_p (+ P_0)
    m     = (S + eps I)^-1 (P_d m_d - P_p m_p (+ P_0 m_0))
    logit = logit_d - logit_p + (-logdet(S + eps I) - logdet P_p + logdet P_d) / 2
            - (m_d^T P_d m_d - m_p^T P_p m_p - m^T S m) / 2
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from sbi_amd import _lib

CORRECTION_EPSILON = 1e-6       # sbi's _CORRECTION_EPSILON
MAX_DIM, MAX_COMPONENTS = 16, 65536
ENVELOPE = "MoG kernels: 1 <= theta-dim <= 16, 1 <= components per mixture row <= 65 536"
NOT_PD = ("Posterior precision matrix is not positive definite. This is a known issue with NPE-A when the proposal "
          "and density estimator don't align well. Try different hyperparameters. ")


def in_envelope(dim: int, num_components: int) -> bool:
    return 1 <= dim <= MAX_DIM and 1 <= num_components <= MAX_COMPONENTS


def _on_kernels(dim: int, num_components: int, *tensors: Optional[Tensor]) -> bool:
    ts = [t for t in tensors if t is not None]
    return (in_envelope(dim, num_components) and all(t.is_cuda and t.dtype == torch.float32 for t in ts)
            and not any(t.requires_grad for t in ts))


def _c(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.contiguous()


# ------------------------------------------------------------------------------------------------ correction
def correct_eager(d_logits: Tensor, d_means: Tensor, d_prec: Tensor, p_logits: Tensor, p_means: Tensor,
                  p_prec: Tensor, prior_mean: Optional[Tensor] = None, prior_prec: Optional[Tensor] = None,
                  eps: float = CORRECTION_EPSILON) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(logits (B, M), means (B, M, D), S + eps I (B, M, D, D), upper factors (B, M, D, D), status (B) int32) in the
    dtype of the inputs.  Density rows (B, K, ...), proposal rows (1 or B, L, ...)."""
    B, K, D = d_means.shape
    L = p_means.shape[1]

    def rep_p(t):      # proposal component l -> j = l K + k
        return t.repeat_interleave(K, dim=1)

    def rep_d(t):
        return t.repeat(1, L, *([1] * (t.dim() - 2)))

    S = rep_d(d_prec) - rep_p(p_prec)
    pm_d = torch.einsum("bkij,bkj->bki", d_prec, d_means)
    pm_p = torch.einsum("bkij,bkj->bki", p_prec, p_means)
    rhs = rep_d(pm_d) - rep_p(pm_p)
    if prior_prec is not None:
        S = S + prior_prec
        rhs = rhs + prior_prec @ prior_mean
    eye = torch.eye(D, dtype=S.dtype, device=S.device)
    S_stab = S + eps * eye
    Lf, info = torch.linalg.cholesky_ex(S_stab)
    failed = info > 0
    if failed.any():      # (keep the failed components finite: they are reported through `status`, not as NaN)
        Lf = torch.where(failed[..., None, None], eye.expand_as(Lf), Lf)
    U = Lf.transpose(-1, -2)
    m = torch.cholesky_solve(rhs.unsqueeze(-1), Lf).squeeze(-1)
    ld_post = 2.0 * torch.log(torch.diagonal(U, dim1=-2, dim2=-1)).sum(-1)
    ld_d = torch.linalg.slogdet(d_prec)[1]
    ld_p = torch.linalg.slogdet(p_prec)[1]
    q_d = (d_means * pm_d).sum(-1)
    q_p = (p_means * pm_p).sum(-1)
    q_post = (m * torch.einsum("bmij,bmj->bmi", S, m)).sum(-1)
    logits = (rep_d(d_logits) - rep_p(p_logits) + 0.5 * (-ld_post - rep_p(ld_p) + rep_d(ld_d))
              - 0.5 * (rep_d(q_d) - rep_p(q_p) - q_post))
    failed = failed | ~torch.isfinite(logits)
    first = torch.where(failed, torch.arange(1, K * L + 1, device=S.device).expand(B, -1),
                        torch.full((B, K * L), K * L + 1, device=S.device)).min(dim=1).values
    status = torch.where(first > K * L, torch.zeros_like(first), first).to(torch.int32)
    if failed.any():
        logits = torch.where(failed, torch.zeros_like(logits), logits)
        m = torch.where(failed[..., None], torch.zeros_like(m), m)
        U = torch.where(failed[..., None, None], torch.zeros_like(U), U)
    return logits, m, S_stab.expand(B, -1, -1, -1).contiguous(), U.contiguous(), status


def correct_kernel(d_logits: Tensor, d_means: Tensor, d_prec: Tensor, p_logits: Tensor, p_means: Tensor,
                   p_prec: Tensor, prior_mean: Optional[Tensor] = None, prior_prec: Optional[Tensor] = None,
                   eps: float = CORRECTION_EPSILON) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """`correct_eager` on ``sbi_amd_mog_correct`` (fp64 inside, fp32 in and out)."""
    d_logits, d_means, d_prec, p_logits, p_means, p_prec, prior_mean, prior_prec = map(
        _c, (d_logits, d_means, d_prec, p_logits, p_means, p_prec, prior_mean, prior_prec))
    dev = _lib.require_device(d_logits, d_means, d_prec, p_logits, p_means, p_prec, prior_mean, prior_prec)
    B, K, D = d_means.shape
    rows, L = p_means.shape[:2]
    M = K * L
    lib = _lib.load()
    need = lib.sbi_amd_mog_correct_workspace_bytes(B, K, L, D, rows)
    if need < 0:
        _lib.check(int(need), f"mog_correct ({ENVELOPE})")
    logits = torch.empty(B, M, dtype=torch.float32, device=dev)
    means = torch.empty(B, M, D, dtype=torch.float32, device=dev)
    prec = torch.empty(B, M, D, D, dtype=torch.float32, device=dev)
    factors = torch.empty(B, M, D, D, dtype=torch.float32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    if B:
        ws = torch.empty(max(int(need) // 8, 1), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = lib.sbi_amd_mog_correct(_lib.ptr(d_logits), _lib.ptr(d_means), _lib.ptr(d_prec), B, K,
                                         _lib.ptr(p_logits), _lib.ptr(p_means), _lib.ptr(p_prec), rows, L, D,
                                         _lib.ptr(prior_mean), _lib.ptr(prior_prec), float(eps), _lib.ptr(logits),
                                         _lib.ptr(means), _lib.ptr(prec), _lib.ptr(factors), status.data_ptr(),
                                         ws.data_ptr(), _lib.current_stream(dev))
        _lib.check(rc, "mog_correct")
    return logits, means, prec, factors, status


def correct_for_proposal(density_mog, proposal_mog, prior_mog=None):
    """The corrected posterior mixture (L K components) of sbi's ``_correct_for_proposal``; ``prior_mog`` is a
    one-component MoG (Gaussian prior) or None (uniform prior, its term is omitted).  Raises sbi's ValueError when a
    corrected precision is not positive definite."""
    from sbi_amd.neural_nets.estimators.mdn import MoG

    B = density_mog.logits.shape[0]
    rows = proposal_mog.logits.shape[0]
    if rows not in (1, B):
        raise ValueError(f"proposal_mog has {rows} rows; the density mixture has {B} (need 1 or {B})")
    p0_mean = p0_prec = None
    if prior_mog is not None:
        p0_mean, p0_prec = prior_mog.means[0, 0], prior_mog.precisions[0, 0]
    args = (density_mog.logits, density_mog.means, density_mog.precisions, proposal_mog.logits, proposal_mog.means,
            proposal_mog.precisions, p0_mean, p0_prec)
    M = density_mog.num_components * proposal_mog.num_components
    fn = correct_kernel if _on_kernels(density_mog.dim, M, *args) else correct_eager
    logits, means, prec, factors, status = fn(*args, eps=CORRECTION_EPSILON)
    bad = torch.nonzero(status)
    if bad.numel():
        b = int(bad[0])
        raise ValueError(NOT_PD + f"Original error: component {int(status[b]) - 1} of mixture row {b} has a "
                                  "non-positive pivot in its Cholesky factorisation.")
    return MoG(logits=logits, means=means, precisions=prec, precision_factors=factors)


# ------------------------------------------------------------------------------------------------ log_prob
def _affine(theta: Tensor, shift: Optional[Tensor], scale: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    if shift is None:
        return theta, torch.zeros((), dtype=theta.dtype, device=theta.device)
    return (theta - shift) / scale, torch.log(scale).sum()


def log_prob_eager(logits: Tensor, means: Tensor, prec: Tensor, factors: Tensor, theta: Tensor,
                   shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> Tensor:
    """out (n,): row i of theta (n, D) under mixture row i % mog_rows (``MoG.log_prob`` plus the z-score Jacobian);
    never materialises an (n, M, D, D) broadcast."""
    R, M, D = means.shape
    n = theta.shape[0]
    z, log_jac = _affine(theta, shift, scale)
    const = (torch.log_softmax(logits, dim=-1) - 0.5 * D * math.log(2 * math.pi)
             + torch.log(torch.diagonal(factors, dim1=-2, dim2=-1)).sum(-1))          # (R, M)
    out = torch.empty(n, dtype=theta.dtype, device=theta.device)
    if R == 1:
        step = max(1, (1 << 24) // (M * D))
        for lo in range(0, n, step):
            d = z[lo : lo + step, None, :] - means[0]                                  # (c, M, D)
            q = (torch.einsum("nmd,mde->nme", d, prec[0]) * d).sum(-1)
            out[lo : lo + step] = torch.logsumexp(const[0] - 0.5 * q, dim=-1)
        return out - log_jac
    if n % R == 0:
        d = z.reshape(n // R, R, 1, D) - means                                         # (S, R, M, D)
        q = (torch.einsum("srmd,rmde->srme", d, prec) * d).sum(-1)
        return torch.logsumexp(const - 0.5 * q, dim=-1).reshape(n) - log_jac
    idx = torch.arange(n, device=theta.device) % R
    d = z[:, None, :] - means[idx]
    q = (torch.einsum("nmd,nmde->nme", d, prec[idx]) * d).sum(-1)
    return torch.logsumexp(const[idx] - 0.5 * q, dim=-1) - log_jac


def log_prob_kernel(logits: Tensor, means: Tensor, prec: Tensor, factors: Tensor, theta: Tensor,
                    shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> Tensor:
    logits, means, prec, factors, theta, shift, scale = map(_c, (logits, means, prec, factors, theta, shift, scale))
    dev = _lib.require_device(logits, means, prec, factors, theta, shift, scale)
    R, M, D = means.shape
    n = theta.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_mog_log_prob(_lib.ptr(logits), _lib.ptr(means), _lib.ptr(prec), _lib.ptr(factors), R, M,
                                              D, _lib.ptr(theta), n, _lib.ptr(shift), _lib.ptr(scale), _lib.ptr(out),
                                              _lib.current_stream(dev))
    _lib.check(rc, f"mog_log_prob ({ENVELOPE})")
    return out


def mog_log_prob(logits: Tensor, means: Tensor, prec: Tensor, factors: Tensor, theta: Tensor,
                 shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> Tensor:
    fn = log_prob_kernel if _on_kernels(means.shape[2], means.shape[1], logits, means, prec, factors, theta, shift,
                                        scale) else log_prob_eager
    return fn(logits, means, prec, factors, theta, shift, scale)


# ------------------------------------------------------------------------------------------------ sample
def select_components(logits: Tensor, u: Tensor) -> Tensor:
    """k (n,) int64: the number of cumulative normalised weights <= u[i] of mixture row i % rows, clamped to M - 1
    (fp64 table, as the kernel builds it)."""
    R, M = logits.shape
    cdf = torch.softmax(logits.double(), dim=-1).cumsum(-1)
    cdf = cdf / cdf[:, -1:]
    if R == 1:
        k = torch.searchsorted(cdf[0], u.double(), right=True)
    else:
        idx = torch.arange(u.shape[0], device=u.device) % R
        k = torch.searchsorted(cdf[idx], u.double().unsqueeze(-1), right=True).squeeze(-1)
    return k.clamp_(max=M - 1)


def sample_eager(logits: Tensor, means: Tensor, factors: Tensor, zeta: Tensor, u: Optional[Tensor] = None,
                 comp: Optional[Tensor] = None, shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> Tensor:
    """theta (n, D) = (m_k + U_k^-1 zeta_i) * scale + shift from mixture row i % rows; k = comp[i] or from u[i]."""
    R, M, D = means.shape
    n = zeta.shape[0]
    k = comp.long() if comp is not None else select_components(logits, u)
    row = torch.arange(n, device=zeta.device) % R
    x = torch.linalg.solve_triangular(factors[row, k], zeta.unsqueeze(-1), upper=True).squeeze(-1)
    out = means[row, k] + x
    return out if shift is None else out * scale + shift


def sample_kernel(logits: Tensor, means: Tensor, factors: Tensor, zeta: Tensor, u: Optional[Tensor] = None,
                  comp: Optional[Tensor] = None, shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> Tensor:
    logits, means, factors, zeta, u, shift, scale = map(_c, (logits, means, factors, zeta, u, shift, scale))
    dev = _lib.require_device(logits, means, factors, zeta, u, shift, scale)
    if u is None and comp is None:
        raise ValueError("sbi_amd: mog sampling needs `u` or `comp`")
    if comp is not None:
        comp = comp.to(dev, torch.int32).contiguous()
    R, M, D = means.shape
    n = zeta.shape[0]
    out = torch.empty(n, D, dtype=torch.float32, device=dev)
    ws = torch.empty(R * M, dtype=torch.float64, device=dev) if comp is None else None
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_mog_sample(_lib.ptr(logits), _lib.ptr(means), _lib.ptr(factors), R, M, D, _lib.ptr(u),
                                            _lib.ptr(comp), _lib.ptr(zeta), n, _lib.ptr(shift), _lib.ptr(scale),
                                            _lib.ptr(out), _lib.ptr(ws), _lib.current_stream(dev))
    _lib.check(rc, f"mog_sample ({ENVELOPE})")
    return out


def mog_sample(logits: Tensor, means: Tensor, factors: Tensor, zeta: Tensor, u: Optional[Tensor] = None,
               comp: Optional[Tensor] = None, shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> Tensor:
    fn = sample_kernel if _on_kernels(means.shape[2], means.shape[1], logits, means, factors, zeta, u, shift,
                                      scale) else sample_eager
    return fn(logits, means, factors, zeta, u, comp, shift, scale)
