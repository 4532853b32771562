#!/usr/bin/env python
"""Generate tests/golden/nre_reference.pt: the REAL `_loss` methods of sbi's NRE_A, NRE_B, NRE_C and BNRE
(sbi/inference/trainers/nre/nre_{a,b,c}.py, bnre.py, through `_classifier_logits`, nre_base.py:396-415) and the real
`_log_ratios_over_trials` (sbi/inference/potentials/ratio_based_potential.py:122-160), evaluated with a ResNet classifier
(the oracle's ResidualNet behind z-scoring), with the contrasting-atom choices they drew (torch.multinomial) recorded.
Build container only."""

import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Classifier(torch.nn.Module):
    """net(theta, x) -> logit: Standardize theta and x, concatenate, ResidualNet (build_resnet_classifier's network)."""

    def __init__(self, D, C, H, NB, zstats):
        super().__init__()
        sys.path.insert(0, ROOT)
        from oracle.nsf_oracle import ResidualNet

        self.D, self.C = D, C
        self.net = ResidualNet(D + C, 1, H, None, NB)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for p in self.net.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
        self.register_buffer("zstats", zstats)

    def forward(self, theta, x):
        D, C, z = self.D, self.C, self.zstats
        zt = (theta - z[:D]) / z[D : 2 * D]
        zx = (x - z[2 * D : 2 * D + C]) / z[2 * D + C :]
        return self.net(torch.cat([zt, zx], dim=-1)).squeeze(-1)


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # installs the third-party stubs and puts the reference on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.inference.potentials.ratio_based_potential import _log_ratios_over_trials
    from sbi.inference.trainers.nre.bnre import BNRE
    from sbi.inference.trainers.nre.nre_a import NRE_A
    from sbi.inference.trainers.nre.nre_b import NRE_B
    from sbi.inference.trainers.nre.nre_c import NRE_C

    D, C, H, NB, B = 3, 4, 20, 2, 24
    torch.manual_seed(11)
    theta, x = torch.randn(B, D) * 1.3, torch.randn(B, C)
    zstats = torch.cat([theta.mean(0), theta.std(0), x.mean(0), x.std(0)])
    net = Classifier(D, C, H, NB, zstats)
    out = {"D": D, "C": C, "H": H, "NB": NB, "theta": theta, "x": x, "zstats": zstats,
           "state_dict": {k: v.clone() for k, v in net.net.state_dict().items()}, "losses": {}}
    cases = {"NRE_A": (NRE_A, dict(num_atoms=2)), "NRE_B": (NRE_B, dict(num_atoms=7)),
             "NRE_C": (NRE_C, dict(num_atoms=5, gamma=1.7)), "BNRE": (BNRE, dict(num_atoms=2, regularization_strength=30.0))}
    for name, (cls, kw) in cases.items():
        self = types.SimpleNamespace(_device="cpu", _neural_net=net)
        self._classifier_logits = lambda th, xx, a, _s=self, _c=cls: _c._classifier_logits(_s, th, xx, a)
        if cls is NRE_C:
            self._get_prior_probs_marginal_and_joint = NRE_C._get_prior_probs_marginal_and_joint
        recorded = []
        real_multinomial = torch.multinomial

        def rec(*a, **k):
            r = real_multinomial(*a, **k)
            recorded.append(r.clone())
            return r

        torch.multinomial = rec
        try:
            with torch.no_grad():
                loss = cls._loss(self, theta, x, **kw)
        finally:
            torch.multinomial = real_multinomial
        out["losses"][name] = {"kwargs": kw, "choices": recorded, "loss": loss.detach().clone()}
    x_o, th_t = torch.randn(5, C), torch.randn(9, D)
    with torch.no_grad():
        out["trials"] = {"x_o": x_o, "theta": th_t, "sum": _log_ratios_over_trials(x_o, th_t, net).clone()}
    path = os.path.join(ROOT, "tests", "golden", "nre_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), {k: float(v["loss"]) for k, v in out["losses"].items()})


if __name__ == "__main__":
    main()
