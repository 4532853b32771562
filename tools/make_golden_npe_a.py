#!/usr/bin/env python
"""Generate tests/golden/npe_a_reference.pt: outputs of the REAL sbi functions `_correct_for_proposal`
(sbi/inference/trainers/npe/npe_a.py) and `MoG.log_prob` / `MoG.sample` / `MoG.from_gaussian`
(sbi/neural_nets/estimators/mog.py) on small fixed mixtures -- (D, K, L) in {(1, 3, 1), (3, 4, 2)}, each with a
Gaussian prior and with none.  Inputs are float32-representable values stored as float64 and the reference runs in
float64, so the recorded outputs serve as the fp64 truth of the float32 routes.  `MoG.sample` is recorded with the
`torch.multinomial` choices and `torch.randn` draws it made.  Tensors only.  Build container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mixture(g, B, K, D, lo, hi, mean_scale):
    """Precision factors with diagonal U(lo, hi) and strict upper (0.5 lo / D) N(0, 1); float32 values as float64."""
    A = torch.triu(torch.randn(B, K, D, D, generator=g), 1) * (0.5 * lo / D)
    i = torch.arange(D)
    A[..., i, i] = torch.rand(B, K, D, generator=g) * (hi - lo) + lo
    prec = A.transpose(-1, -2) @ A
    logits = torch.randn(B, K, generator=g)
    means = mean_scale * torch.randn(B, K, D, generator=g)
    return logits.double(), means.double(), prec.double(), A.double()


def one_case(MoG, correct, D, K, L, with_prior, seed):
    g = torch.Generator().manual_seed(seed)
    B = 3
    d = mixture(g, B, K, D, 2.0, 4.0, 0.5)
    p = mixture(g, 1, L, D, 0.5, 1.0, 0.5)
    out = {"D": D, "K": K, "L": L, "density": d, "proposal": p}
    density, proposal = MoG(*d), MoG(*p)
    prior = None
    if with_prior:
        _, m0, P0, _ = mixture(g, 1, 1, D, 0.2, 0.3, 0.1)
        cov0 = torch.linalg.inv(P0[0, 0]).float().double()
        cov0 = 0.5 * (cov0 + cov0.T)
        prior = MoG.from_gaussian(m0[0, 0], cov0)
        out["prior_mean"], out["prior_cov"] = m0[0, 0], cov0
        out["from_gaussian"] = (prior.logits, prior.means, prior.precisions, prior.precision_factors)
    post = correct(density, proposal, prior)
    out["corrected"] = (post.logits, post.means, post.precisions, post.precision_factors)
    theta = (0.6 * torch.randn(5, B, D, generator=g)).double()
    out["theta"], out["log_prob"] = theta, post.log_prob(theta)
    out["log_prob_2d"] = post.log_prob(theta[0])
    rec = {}
    real_multinomial, real_randn = torch.multinomial, torch.randn

    def multinomial(*a, **k):
        rec["choices"] = real_multinomial(*a, **k)
        return rec["choices"]

    def randn(*a, **k):
        rec["z"] = real_randn(*a, **k)
        return rec["z"]

    torch.manual_seed(seed + 1)
    torch.multinomial, torch.randn = multinomial, randn
    try:
        out["samples"] = post.sample(torch.Size([7]))          # (7, B, D)
    finally:
        torch.multinomial, torch.randn = real_multinomial, real_randn
    out["choices"], out["z"] = rec["choices"], rec["z"]          # (B, 7), (B, 7, D, 1)
    return {k: (tuple(t.clone() for t in v) if isinstance(v, tuple) else (v.clone() if torch.is_tensor(v) else v))
            for k, v in out.items()}


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # installs the third-party stubs and puts the reference on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.inference.trainers.npe.npe_a import _correct_for_proposal
    from sbi.neural_nets.estimators.mog import MoG

    out = {}
    for D, K, L, seed in ((1, 3, 1, 11), (3, 4, 2, 17)):
        for with_prior in (True, False):
            out[f"d{D}k{K}l{L}_{'prior' if with_prior else 'uniform'}"] = one_case(
                MoG, _correct_for_proposal, D, K, L, with_prior, seed)
    path = os.path.join(ROOT, "tests", "golden", "npe_a_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), {k: float(v["log_prob"].mean()) for k, v in out.items()})


if __name__ == "__main__":
    main()
