"""CPU restatement of sbi's iid score composition on top of tests/npse_oracle.py -- TEST INFRASTRUCTURE ONLY.

Restates, per call and in the dtype of its inputs, what IIDScoreFunction.__call__ computes
(sbi/inference/potentials/vector_field_adaptor.py:774-813 fnpe, :962-1031 gauss family, :1357-1410
ensure_lam_positive_definite) for a Gaussian prior: prior score, denoised prior precision, marginal posterior precisions,
the PSD correction with its dense (eigh) and element-wise branches, and the final SOLVE -- i.e. NOT the tabulated form
`sbi_amd` evaluates, so it checks the tables' algebra as well.  tests/test_npse_iid_host_cpu.py pins it in fp64 to the
outputs of the real classes (tests/golden/npse_iid_reference.pt).
"""

from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor
from torch.distributions import Independent, MultivariateNormal, Normal

GOLD = os.path.join(os.path.dirname(__file__), "golden", "npse_iid_reference.pt")
IID_CASES = ["ve_mvn", "ve_indep", "vp_mvn", "vp_indep"]
METHODS = ["fnpe", "gauss", "auto_gauss"]
_fixture = None


def load_iid_case(name):
    global _fixture
    if _fixture is None:
        _fixture = torch.load(GOLD, weights_only=False)
    return _fixture[name]


def make_prior(kind: str, spec: dict, dtype=torch.float32, device="cpu"):
    if kind == "mvn":
        return MultivariateNormal(spec["loc"].to(device=device, dtype=dtype),
                                  covariance_matrix=spec["cov"].to(device=device, dtype=dtype))
    return Independent(Normal(spec["loc"].to(device=device, dtype=dtype), spec["scale"].to(device=device, dtype=dtype)), 1)


def random_prior_spec(D: int, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(seed)
    B = torch.randn(D, D, generator=g) * 0.4
    return dict(loc=torch.linspace(-0.5, 0.7, D), cov=B @ B.T + torch.eye(D), scale=torch.linspace(0.8, 1.6, D))


def _dense(a: Tensor) -> Tensor:        # (..., D) diagonal -> (..., D, D)
    return torch.diag_embed(a)


def _add(a: Tensor, a_diag: bool, b: Tensor, b_diag: bool):
    if a_diag == b_diag:
        return a + b, a_diag
    return (_dense(a) if a_diag else a) + (_dense(b) if b_diag else b), False


def _mv(a: Tensor, a_diag: bool, v: Tensor) -> Tensor:
    return a * v if a_diag else torch.einsum("...ij,...j->...i", a, v)


def iid_score(o, method: str, kind: str, spec: dict, theta: Tensor, xs: Tensor, t: float, prec: Optional[Tensor] = None,
              psd: Optional[bool] = None, nugget: float = 0.01, scale: float = 2.0, s: Optional[Tensor] = None) -> Tensor:
    """Composed score (n, D) at theta (n, D) given xs (N, C) at time t.  `o` is an NPSEOracle in theta's dtype; prec
    (N, D) or (N, D, D) replaces the estimated precisions of auto_gauss; psd None = the method's default."""
    dt = theta.dtype
    n, D = theta.shape
    N = xs.shape[0]
    dev = theta.device
    tt = torch.full((n * N,), t, dtype=dt, device=dev)
    if s is None:
        s = o.score(theta.repeat_interleave(N, 0), xs.to(dt).repeat(n, 1), tt).reshape(n, N, D)
    m, sd = o.mean_t(tt[:1])[0], o.std_t(tt[:1])[0]
    spec = {k: v.to(dev) for k, v in spec.items()}
    mu0 = spec["loc"].to(dt)
    prior_diag = kind != "mvn"
    sigma0 = spec["cov"].to(dt) if kind == "mvn" else torch.diag(spec["scale"].to(dt) ** 2)
    eye = torch.eye(D, dtype=dt, device=dev)
    if method == "fnpe":
        w = (o.t_max - t) / o.t_max
        prior_score = -(theta - mu0) @ torch.linalg.inv(sigma0).T
        return (1 - N) * w * prior_score + s.sum(1)
    if psd is None:
        psd = method == "auto_gauss"
    prior_score = -(theta - m * mu0) @ torch.linalg.inv(m**2 * sigma0 + sd**2 * eye).T
    c = m**2 / sd**2
    if prior_diag:
        P0 = 1 / spec["scale"].to(dt) ** 2 + c
    else:
        P0 = torch.linalg.inv(torch.linalg.inv(torch.linalg.inv(sigma0) + c * eye))     # inverse of the denoised covariance
    if method == "gauss":
        var = torch.diagonal(sigma0)
        lam, lam_diag = (scale / var).expand(N, D), True
    else:
        lam, lam_diag = prec.to(device=dev, dtype=dt), prec.dim() == 2
    P = c * (torch.ones(D, dtype=dt, device=dev) if lam_diag else eye) + lam            # (N, D) or (N, D, D)

    def total(P):
        return _add((1 - N) * P0, prior_diag, P.sum(0), lam_diag)

    if psd:
        Lam, diag = total(P)
        if D > 1 and not diag:
            ev, V = torch.linalg.eigh(Lam)
            fix = torch.where(ev <= 0, -ev, torch.zeros_like(ev)) / (N - 1)
            corr = torch.einsum("ij,j,kj->ik", V, fix, V) + nugget * eye
            P, lam_diag = (_dense(P) if lam_diag else P) + corr, False
        else:
            corr = torch.where(Lam > 0, torch.zeros_like(Lam), -Lam) / (N - 1) + nugget
            P = P + corr
    Lam, diag = total(P)
    rhs = (1 - N) * _mv(P0, prior_diag, prior_score) + _mv(P, lam_diag, s).sum(1)
    return rhs / Lam if diag else torch.linalg.solve(Lam, rhs.unsqueeze(-1)).squeeze(-1)


def compose(tb, k: int, s: Tensor, theta: Tensor) -> Tensor:
    """The tabulated form in the tables' own precision: Linv (C sum s_i + sum Lam_i s_i) + A theta + b."""
    Linv, C, A = tb.mats[k]
    w = s.sum(1) @ C.T
    if tb.lam is not None:
        w = w + torch.einsum("ide,nie->nd", tb.lam, s)
    return w @ Linv.T + theta @ A.T + tb.vecs[k]


@torch.no_grad()
def sample_iid(o, method: str, kind: str, spec: dict, xs: Tensor, ts: Tensor, noise: Tensor, eta: float = 1.0, **kw):
    """Euler-Maruyama replay with the composed score: noise (len(ts), n, D)."""
    dt = noise.dtype
    mean_b, std_b = o.base()
    if method == "fnpe":
        std_b = std_b / xs.shape[0] ** 0.5
    theta = mean_b + std_b * noise[0]
    n = theta.shape[0]
    for k in range(1, ts.numel()):
        t1, t0 = ts[k - 1], ts[k]
        d = t1 - t0
        tt = t1.expand(n)
        g = o.diffusion(tt)[:, None]
        sc = iid_score(o, method, kind, spec, theta, xs, float(t1), **kw)
        theta = theta - (o.drift(theta, tt) - (1 + eta**2) / 2 * g**2 * sc) * d + eta * g * noise[k] * torch.sqrt(d)
    return theta.to(dt)
