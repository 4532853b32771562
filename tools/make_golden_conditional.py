#!/usr/bin/env python
"""Generate tests/golden/conditional_reference.pt from the REAL reference code (run in the build container only).

Reuses the import stubs of tools/make_golden.py.  `sbi.utils.conditional_density_utils` imports that way;
`sbi/analysis/conditional_density.py` is loaded by file path because the package `__init__` pulls in the plotting
stack.  Stored: the inputs, the reference's outputs, and an independent fp64 evaluation (numpy, the textbook weighted
Pearson formula on the stored fp32 grid) of every grid's correlation coefficient.  tests/test_conditional_cpu.py
replays them; the reference tree is NOT needed at test time.
"""

import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402,F401  (installs the stubs and puts the reference tree on sys.path)

OUT = os.path.join(make_golden.OUT, "conditional_reference.pt")


def load_reference():
    from sbi.utils import conditional_density_utils as U

    path = os.path.join(make_golden.REF, "sbi", "analysis", "conditional_density.py")
    spec = importlib.util.spec_from_file_location("_ref_conditional_density", path)
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    return U, A


class Gaussian:
    """log N(theta; mean, cov) in fp32 from the precision matrix, element-wise in a fixed order (no BLAS call), so
    that tests/test_conditional_cpu.py -- which carries the same few lines -- evaluates bit-identical log-probs on any
    machine and the comparison with these recorded outputs is about the code under test alone."""

    def __init__(self, mean, cov):
        self.mean = mean
        self.prec = torch.linalg.inv(cov.double()).float()
        self.const = float(-0.5 * (len(mean) * np.log(2 * np.pi) + torch.logdet(cov.double())))

    def log_prob(self, theta):
        d = theta - self.mean
        q = torch.zeros_like(d[:, 0])
        for a in range(d.shape[1]):
            for b in range(d.shape[1]):
                q = q + self.prec[a, b] * d[:, a] * d[:, b]
        return self.const - 0.5 * q


def rho_fp64(probs, lim_x, lim_y):
    """Weighted Pearson coefficient of probs[i, j] at (x_j, y_i) in numpy fp64 (x along columns, as the reference)."""
    w = probs.double().numpy()
    Ry, Rx = w.shape
    x = torch.linspace(float(lim_x[0]), float(lim_x[1]), Rx).double().numpy()
    y = torch.linspace(float(lim_y[0]), float(lim_y[1]), Ry).double().numpy()
    S = w.sum()
    ex, ey = (w.sum(0) * x).sum() / S, (w.sum(1) * y).sum() / S
    vx = (w.sum(0) * (x - ex) ** 2).sum() / S
    vy = (w.sum(1) * (y - ey) ** 2).sum() / S
    cov = (w * np.outer(y - ey, x - ex)).sum() / S
    return float(cov / np.sqrt(vx * vy))


def main():
    U, A = load_reference()
    g = {}
    torch.manual_seed(20261019)

    # ---- an analytic Gaussian density at D = 4
    D = 4
    M = torch.randn(D, D) * 0.5
    cov = M @ M.T + 0.4 * torch.eye(D)
    mean = torch.tensor([0.2, -0.3, 0.1, 0.4])
    dens = Gaussian(mean, cov)
    limits = torch.tensor([[-2.0, 2.0]] * D)
    conditions = mean + 0.5 * torch.randn(3, D)
    grids = []
    for R in (20, 50):
        for (d1, d2) in ((0, 1), (1, 3), (2, 0), (3, 3)):
            probs = A.eval_conditional_density(dens, conditions[:1], limits, d1, d2, resolution=R)
            raw = A.eval_conditional_density(dens, conditions[:1], limits, d1, d2, resolution=R,
                                             return_raw_log_prob=True)
            e = dict(R=R, dim1=d1, dim2=d2, probs=probs.clone(), raw=raw.clone())
            if d1 != d2:
                e["rho_ref"] = U.compute_corrcoeff(probs, limits[[d1, d2]]).reshape(()).clone()
                e["rho_fp64"] = rho_fp64(probs, limits[d1], limits[d2])
            grids.append(e)
    g["gaussian4"] = dict(mean=mean, cov=cov, prec=dens.prec, const=dens.const, limits=limits, conditions=conditions,
                          grids=grids)
    g["corrcoeff"] = dict(
        full=A.conditional_corrcoeff(dens, limits, conditions, resolution=50).clone(),
        subset=[0, 2, 3],
        sub=A.conditional_corrcoeff(dens, limits, conditions, subset=[0, 2, 3], resolution=50).clone())

    # ---- the rho family: bivariate Gaussians, sigma in [0.3, 1], limits [-2, 2] / [-1, 3]
    lim2 = torch.tensor([[-2.0, 2.0], [-1.0, 3.0]])
    fam = []
    for R in (20, 50):
        for _ in range(6):
            s = 0.3 + 0.7 * torch.rand(2)
            r = 1.6 * torch.rand(()) - 0.8
            c2 = torch.tensor([[s[0] ** 2, r * s[0] * s[1]], [r * s[0] * s[1], s[1] ** 2]])
            m2 = torch.tensor([0.0, 1.0]) + 0.6 * (torch.rand(2) - 0.5)
            d2 = Gaussian(m2, c2)
            probs = A.eval_conditional_density(d2, torch.zeros(1, 2), lim2, 0, 1, resolution=R)
            fam.append(dict(R=R, mean=m2, cov=c2, prec=d2.prec, const=d2.const, probs=probs.clone(),
                            rho_ref=U.compute_corrcoeff(probs, lim2).reshape(()).clone(),
                            rho_fp64=rho_fp64(probs, lim2[0], lim2[1])))
    g["family"] = dict(limits=lim2, cases=fam)

    # ---- condition_mog: K = 3, D = 4, dims [0, 2]
    K = 3
    logits = torch.log_softmax(torch.randn(1, K), dim=-1)
    means = torch.randn(1, K, D)
    precfs = torch.triu(0.4 * torch.randn(1, K, D, D), diagonal=1) + torch.diag_embed(0.8 + torch.rand(1, K, D))
    cond = torch.randn(1, D)
    dims = [0, 2]
    cl, cm, cp, cs = U.condition_mog(cond, dims, logits, means, precfs)
    g["condition_mog"] = dict(condition=cond, dims=dims, logits=logits, means=means, precfs=precfs,
                              out_logits=cl.clone(), out_means=cm.clone(), out_precfs=cp.clone(),
                              out_sumlogdiag=cs.clone())
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(g, OUT)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
