#!/usr/bin/env python
"""Generate tests/golden/diagnostics_reference.pt from the REAL sbi diagnostics (build container only):
`sbi.diagnostics.sbc._run_sbc` / `check_uniformity_frequentist` and `sbi.diagnostics.tarp._run_tarp` /
`get_tarp_references` / `check_tarp`.

The task is the analytic linear-Gaussian one (theta ~ N(0, 1), x = theta + 0.5 eps, D = 3): the exact posterior is
N(x / 1.25, 0.2).  Three sample sets are recorded per observation -- the exact posterior and the same draws pulled
towards / pushed away from the posterior mean by 0.5 and 2 (a too-narrow and a too-wide posterior) -- with the inputs
(`thetas`, `xs`, `posterior_samples`, `references`) and the outputs: ranks for "marginals" and for a callable reduce
(the squared norm of theta plus the first coordinate of x), their KS p-values, ecp / alpha with `z_score_theta` on and
off, and the area to the curve.  Data only; N = 200, L = 100 keeps the file under 1 MiB."""

import os
import sys

import torch

N, L, D = 200, 100, 3
SCALES = {"calibrated": 1.0, "narrow": 0.5, "wide": 2.0}


def reduce_sqnorm(theta, x):
    return (theta**2).sum(-1) + x.reshape(-1)[0]


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # third-party stubs + the reference tree on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib", "tqdm", "tqdm.auto",
                "skorch", "skorch.callbacks", "skorch.dataset", "skorch.utils"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.diagnostics.sbc import _run_sbc, check_uniformity_frequentist
    from sbi.diagnostics.tarp import _run_tarp, check_tarp, get_tarp_references

    torch.manual_seed(0)
    thetas = torch.randn(N, D)
    xs = thetas + 0.5 * torch.randn(N, D)
    mean, std = xs / 1.25, 0.2**0.5
    eps = torch.randn(L, N, D)
    references = get_tarp_references(thetas)
    g = {"thetas": thetas, "xs": xs, "references": references, "num_posterior_samples": L, "cases": {}}
    for name, scale in SCALES.items():
        samples = mean + scale * std * eps
        case = {"posterior_samples": samples}
        for key, fns in (("marginals", "marginals"), ("callable", reduce_sqnorm)):
            ranks = _run_sbc(thetas, xs, samples, fns, show_progress_bar=False)
            case[f"ranks_{key}"] = ranks
            case[f"ks_pvals_{key}"] = check_uniformity_frequentist(ranks, L)
        for z in (True, False):
            ecp, alpha = _run_tarp(samples, thetas, references, num_bins=None, z_score_theta=z)
            atc, ks = check_tarp(ecp, alpha)
            tag = "z" if z else "raw"
            case.update({f"ecp_{tag}": ecp, f"alpha_{tag}": alpha, f"atc_{tag}": float(atc), f"tarp_ks_{tag}": float(ks)})
        g["cases"][name] = case
        print(name, case["ks_pvals_marginals"].tolist(), case["atc_z"], case["atc_raw"])
    out = os.path.join(make_golden.OUT, "diagnostics_reference.pt")
    torch.save(g, out)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
