"""The eager restatement (tests/mdn_oracle.py) reproduces every quantity recorded from the real sbi classes
(tests/golden/mdn_reference.pt, tools/make_golden_mdn.py) to 1e-6 relative: mixture components, log_prob with and
without a sample dimension, loss, the parameter gradient of the mean loss, sample for the recorded choices and draws,
and the constants a fresh initialisation leaves."""
import math
import os

import pytest
import torch

from tests.mdn_oracle import MDNOracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mdn_reference.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN)


def _close(got, ref, what):
    err = (got - ref).abs().max().item()
    assert err <= 1e-6 * max(1.0, ref.abs().max().item()), f"{what}: {err:.3e}"


@pytest.mark.parametrize("case", ["d3", "d1"])
def test_restatement_reproduces_the_reference(golden, case):
    c = golden[case]
    D, B = c["D"], c["theta"].shape[0]
    o = MDNOracle(D, c["C"], c["H"], c["K"])
    assert list(o.state_dict()) == list(c["state_dict"])        # the reference's keys, in its order
    o.load_state_dict(c["state_dict"], strict=True)
    with torch.no_grad():
        logits, means, A = o.components(c["x"])
        _close(logits, c["logits"], "logits")
        _close(means, c["means"], "means")
        _close(A, c["precision_factors"], "precision_factors")
        _close(o.precisions(A), c["precisions"], "precisions")
        lp = o.log_prob(c["theta"], c["x"])
        assert lp.shape == (B,)
        _close(lp, c["log_prob"], "log_prob")
        _close(o.log_prob(c["theta_s"], c["x"]), c["log_prob_s"], "log_prob with a sample dimension")
        _close(o.loss(c["theta"], c["x"]), c["loss"], "loss")
        comp = c["choices"].t().reshape(-1)
        zeta = c["z"][..., 0].transpose(0, 1).reshape(-1, D)
        _close(o.sample_given(comp, zeta, c["x"]).reshape(7, B, D), c["samples"], "sample")
    o.zero_grad()
    o.loss(c["theta"], c["x"]).mean().backward()
    named = dict(o.named_parameters())
    assert set(named) == set(c["grad"])
    scale = max(v.abs().max().item() for v in c["grad"].values())
    for k, v in c["grad"].items():
        assert (named[k].grad - v).abs().max().item() <= 1e-6 * max(1.0, scale), k


@pytest.mark.parametrize("case", ["d3", "d1"])
def test_initialisation_constants(golden, case):
    c = golden[case]
    eps = 1e-4
    o = MDNOracle(c["D"], c["C"], c["H"], c["K"])
    sd = o.state_dict()
    assert set(c["init_constants"]) == {"net._unconstrained_diagonal_layer.bias"} | (
        {"net._upper_layer.bias"} if c["D"] > 1 else set())
    for k, v in c["init_constants"].items():
        assert (sd[k] - v).abs().max() <= 1e-6, k
    assert abs(float(sd["net._unconstrained_diagonal_layer.bias"][0]) - math.log(math.exp(1 - eps) - 1)) <= 1e-6
    for k, std in c["init_std"].items():        # ~N(0, eps) weights: the same scale as the reference's draw
        assert 0.5 * std <= float(sd[k].std()) <= 2.0 * std, k
