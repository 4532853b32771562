#!/usr/bin/env python
"""Generate tests/golden/mdn_reference.pt: outputs of the REAL sbi classes `MultivariateGaussianMDN`,
`MixtureDensityEstimator`, `MoG` and `build_mdn` (sbi/neural_nets/estimators/mixture_density_estimator.py, mog.py,
net_builders/mdn.py) on small fixed inputs -- mixture components, log_prob with and without a sample dimension, loss,
the parameter gradient of the mean loss, `sample` with the `torch.multinomial` choices and `torch.randn` draws it made
recorded, and the constants a fresh `_initialize` leaves.  Build container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_case(build_mdn, D, C, H, K, B, seed):
    torch.manual_seed(seed)
    theta = torch.randn(B, D) * 1.7 + 0.4
    x = torch.randn(B, C) * 0.8 - 0.3
    est = build_mdn(theta, x, hidden_features=H, num_components=K)
    init = {k: v.clone() for k, v in est.state_dict().items()
            if k in ("net._unconstrained_diagonal_layer.bias", "net._upper_layer.bias")}
    init_std = {k: float(v.std()) for k, v in est.state_dict().items()
                if k in ("net._logits_layer.weight", "net._unconstrained_diagonal_layer.weight", "net._upper_layer.weight")}
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():     # away from the near-constant initial heads: every term of the density matters
        for p in est.net.parameters():
            p.add_(0.25 * torch.randn(p.shape, generator=g))
    out = {"D": D, "C": C, "H": H, "K": K, "theta": theta, "x": x, "init_constants": init, "init_std": init_std,
           "state_dict": {k: v.clone() for k, v in est.state_dict().items()}}
    with torch.no_grad():
        mog = est.get_uncorrected_mog(x)
        out["logits"], out["means"] = mog.logits.clone(), mog.means.clone()
        out["precision_factors"], out["precisions"] = mog.precision_factors.clone(), mog.precisions.clone()
        out["log_prob"] = est.log_prob(theta, x).clone()
        theta_s = torch.randn(5, B, D, generator=g) * 1.7
        out["theta_s"], out["log_prob_s"] = theta_s, est.log_prob(theta_s, x).clone()
        out["loss"] = est.loss(theta, x).clone()
    est.zero_grad()
    est.loss(theta, x).mean().backward()
    out["grad"] = {k: p.grad.clone() for k, p in est.named_parameters()}
    rec = {}
    real_multinomial, real_randn = torch.multinomial, torch.randn

    def multinomial(*a, **k):
        rec["choices"] = real_multinomial(*a, **k)
        return rec["choices"]

    def randn(*a, **k):
        rec["z"] = real_randn(*a, **k)
        return rec["z"]

    torch.multinomial, torch.randn = multinomial, randn
    try:
        with torch.no_grad():
            out["samples"] = est.sample(torch.Size([7]), x).clone()     # (7, B, D)
    finally:
        torch.multinomial, torch.randn = real_multinomial, real_randn
    out["choices"], out["z"] = rec["choices"].clone(), rec["z"].clone()   # (B, 7), (B, 7, D, 1)
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # installs the third-party stubs and puts the reference on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.neural_nets.estimators.mixture_density_estimator import MixtureDensityEstimator, MultivariateGaussianMDN
    from sbi.neural_nets.estimators.mog import MoG
    from sbi.neural_nets.net_builders.mdn import build_mdn

    def checked_build(*a, **k):
        est = build_mdn(*a, **k)
        assert isinstance(est, MixtureDensityEstimator) and isinstance(est.net, MultivariateGaussianMDN)
        assert isinstance(est.get_uncorrected_mog(a[1][:2]), MoG)
        return est

    out = {"d3": one_case(checked_build, 3, 4, 16, 4, 24, 5), "d1": one_case(checked_build, 1, 4, 16, 3, 24, 9)}
    path = os.path.join(ROOT, "tests", "golden", "mdn_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), {k: float(v["loss"].mean()) for k, v in out.items()})


if __name__ == "__main__":
    main()
