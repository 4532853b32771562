"""fp64 restatement of the three NPE-A mixture formulas (correction, log_prob, sample) for shapes the golden file does
not carry, and the input recipe of the GPU tests.  Written against the paper's Eqs. 23-26 with inverses and
log-determinants (no shared code with sbi_amd/neural_nets/estimators/mog_ops.py, which factorises)."""

import math

import torch


def mixture(g, B, K, D, lo, hi, mean_scale, diag_scale=1.0):
    """(logits (B, K), means (B, K, D), precisions, factors (B, K, D, D)) float32: factor diagonal U(lo, hi) (times
    diag_scale), strict upper (0.5 lo / D) N(0, 1), means mean_scale N(0, 1)."""
    A = torch.triu(torch.randn(B, K, D, D, generator=g), 1) * (0.5 * lo / D)
    i = torch.arange(D)
    A[..., i, i] = (torch.rand(B, K, D, generator=g) * (hi - lo) + lo) * diag_scale
    return torch.randn(B, K, generator=g), mean_scale * torch.randn(B, K, D, generator=g), A.transpose(-1, -2) @ A, A


def recipe(D, K, L, B, prop_rows, prior, seed=0):
    """Density factor diagonal (2, 4), proposal (0.5, 1), prior (0.2, 0.3): every corrected precision is positive
    definite with a wide margin."""
    g = torch.Generator().manual_seed(seed + 1000 * D + 10 * K + L)
    d = mixture(g, B, K, D, 2.0, 4.0, 0.5)
    p = mixture(g, prop_rows, L, D, 0.5, 1.0, 0.5)
    m0 = P0 = None
    if prior:
        _, m, P, _ = mixture(g, 1, 1, D, 0.2, 0.3, 0.1)
        m0, P0 = m[0, 0].contiguous(), P[0, 0].contiguous()
    return d, p, m0, P0


def min_eigenvalue(d, p, prior_prec=None):
    """Smallest eigenvalue over every unstabilised corrected precision S = P_d - P_p (+ P_0), fp64."""
    dP, pP = d[2].double(), p[2].double()
    K, L = dP.shape[1], pP.shape[1]
    S = dP[:, torch.arange(K * L) % K] - pP[:, torch.arange(K * L) // K]
    if prior_prec is not None:
        S = S + prior_prec.double()
    return float(torch.linalg.eigvalsh(S).min())


def correct(d, p, prior_mean=None, prior_prec=None, eps=1e-6):
    """(logits (B, M), means (B, M, D), S + eps I, upper Cholesky factor) in fp64; component j = l K + k."""
    dl, dm, dP = (t.double() for t in d[:3])
    pl, pm, pP = (t.double() for t in p[:3])
    B, K, D = dm.shape
    L = pm.shape[1]
    k = torch.arange(K * L) % K           # density component of j = l K + k
    l = torch.arange(K * L) // K          # proposal component
    S = dP[:, k] - pP[:, l]
    rhs = torch.einsum("bmij,bmj->bmi", dP[:, k], dm[:, k]) - torch.einsum("bmij,bmj->bmi", pP[:, l], pm[:, l])
    if prior_prec is not None:
        S = S + prior_prec.double()
        rhs = rhs + prior_prec.double() @ prior_mean.double()
    Ss = S + eps * torch.eye(D, dtype=torch.float64)
    m = torch.einsum("bmij,bmj->bmi", torch.linalg.inv(Ss), rhs)

    def quad(P, v):
        return torch.einsum("bmi,bmij,bmj->bm", v, P, v)

    logits = (dl[:, k] - pl[:, l]
              + 0.5 * (-torch.linalg.slogdet(Ss)[1] - torch.linalg.slogdet(pP)[1][:, l] + torch.linalg.slogdet(dP)[1][:, k])
              - 0.5 * (quad(dP, dm)[:, k] - quad(pP, pm)[:, l] - quad(S, m)))
    return logits, m, Ss.expand(B, -1, -1, -1), torch.linalg.cholesky(Ss, upper=True).expand(B, -1, -1, -1)


def log_prob(logits, means, prec, factors, theta, shift=None, scale=None):
    """(n,) fp64: row i under mixture row i % rows."""
    logits, means, prec, factors, theta = (t.double() for t in (logits, means, prec, factors, theta))
    R, M, D = means.shape
    z, jac = theta, 0.0
    if shift is not None:
        z = (theta - shift.double()) / scale.double()
        jac = torch.log(scale.double()).sum()
    logw = torch.log_softmax(logits, dim=-1)
    row = torch.arange(theta.shape[0]) % R
    sld = torch.log(torch.diagonal(factors, dim1=-2, dim2=-1)).sum(-1)
    out = torch.empty(theta.shape[0], dtype=torch.float64)
    for r in range(R):
        mine = row == r
        d = z[mine][:, None, :] - means[r]                             # (n_r, M, D)
        q = torch.einsum("nmd,mde,nme->nm", d, prec[r], d)
        out[mine] = torch.logsumexp(logw[r] - 0.5 * D * math.log(2 * math.pi) + sld[r] - 0.5 * q, dim=-1) - jac
    return out


def select(logits, u):
    """k (n,): the number of cumulative normalised weights <= u[i] (fp64 cumulative sum), clamped to M - 1; also the
    distance of u[i] from the nearest boundary."""
    R, M = logits.shape
    cdf = torch.softmax(logits.double(), dim=-1).cumsum(-1)
    idx = torch.arange(u.shape[0]) % R
    c = cdf[idx]
    k = (c <= u.double()[:, None]).sum(-1).clamp(max=M - 1)
    return k, (c - u.double()[:, None]).abs().min(-1).values


def sample(means, factors, comp, zeta, shift=None, scale=None):
    means, factors, zeta = means.double(), factors.double(), zeta.double()
    R = means.shape[0]
    row = torch.arange(zeta.shape[0]) % R
    x = torch.linalg.solve_triangular(factors[row, comp.long()], zeta.unsqueeze(-1), upper=True).squeeze(-1)
    out = means[row, comp.long()] + x
    return out if shift is None else out * scale.double() + shift.double()
