"""The NRE loss restatements and the iid-trials sum against the reference's own code (tests/golden/nre_reference.pt,
written by tools/make_golden_nre.py: sbi's real NRE_A / NRE_B / NRE_C / BNRE `_loss` and `_log_ratios_over_trials`
with the contrasting-atom choices they drew)."""

import os

import pytest
import torch

from oracle.nsf_oracle import ResidualNet
from sbi_amd.inference.trainers.nre.nre import MODE_A, MODE_B, MODE_BNRE, MODE_C, row_losses_torch

G = torch.load(os.path.join(os.path.dirname(__file__), "golden", "nre_reference.pt"), weights_only=False)


def _logit_fn():
    D, C = G["D"], G["C"]
    net = ResidualNet(D + C, 1, G["H"], None, G["NB"])
    net.load_state_dict(G["state_dict"])
    z = G["zstats"]

    def logit(theta, x):
        zt = (theta - z[:D]) / z[D : 2 * D]
        zx = (x - z[2 * D : 2 * D + C]) / z[2 * D + C :]
        return net(torch.cat([zt, zx], dim=-1)).squeeze(-1)

    return logit


def _atoms(theta, choices):
    """Atoms-major (A, B, D): atom 0 the row itself, then the recorded contrasting rows (the reference's row-major
    atomic_theta, nre_base.py:407-413, transposed)."""
    return torch.cat([theta[None], theta[choices].permute(1, 0, 2)], dim=0)


@pytest.mark.parametrize("name,mode", [("NRE_A", MODE_A), ("NRE_B", MODE_B), ("NRE_C", MODE_C), ("BNRE", MODE_BNRE)])
def test_row_losses_match_the_reference_loss_given_its_choices(name, mode):
    rec = G["losses"][name]
    theta, x = G["theta"], G["x"]
    B, D = theta.shape
    A = rec["kwargs"]["num_atoms"]
    logit = _logit_fn()
    if mode == MODE_C:
        # the reference draws the marginal set (K + 1 atoms) first, then the joint set (K atoms)
        c_m, c_j = rec["choices"]
        atoms = torch.cat([_atoms(theta, c_m), _atoms(theta, c_j)])
    else:
        (ch,) = rec["choices"]
        atoms = _atoms(theta, ch)
    for c in rec["choices"]:       # contrasting atoms are other rows
        assert (c != torch.arange(B)[:, None]).all()
    with torch.no_grad():
        logits = logit(atoms.reshape(-1, D), x.repeat(atoms.shape[0], 1))
        rows = row_losses_torch(mode, logits, B, A, rec["kwargs"].get("gamma", 1.0),
                                rec["kwargs"].get("regularization_strength", 100.0))
    assert rows.shape == (B,)
    assert torch.allclose(rows.mean(), rec["loss"], rtol=2e-6, atol=2e-6), (float(rows.mean()), float(rec["loss"]))


def test_trials_sum_matches_the_reference():
    tr = G["trials"]
    x_o, theta = tr["x_o"], tr["theta"]
    T, N = x_o.shape[0], theta.shape[0]
    logit = _logit_fn()
    with torch.no_grad():       # theta-major pairs, the trials kernel's layout: theta c against trials 0 .. T - 1
        s = logit(theta.repeat_interleave(T, 0), x_o.repeat(N, 1)).reshape(N, T).double().sum(1).float()
    assert torch.allclose(s, tr["sum"], rtol=1e-5, atol=1e-5)
