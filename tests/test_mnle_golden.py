"""The eager restatement (tests/mnle_oracle.py) against recorded outputs of the real in-tree sbi classes
`CategoricalMADE`, `CategoricalMassEstimator` and `MixedDensityEstimator` (tests/golden/mnle_reference.pt,
tools/make_golden_mnle.py --reference).  The two nflows-dependent pieces (the MADE trunk and the flow) were stand-ins
built from the restatement when the file was recorded, so this pins the in-tree arithmetic only: the value <-> index
mapping, the -inf masking of the logits, the log-softmax gather and sum, the combination of the two terms with the
log-transform's Jacobian, the shapes, and the composition of `sample` from the recorded draws."""
import os

import pytest
import torch

from tests.mnle_oracle import MixedOracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnle_reference.pt")


def load(case):
    c = torch.load(GOLDEN)[case]
    o = MixedOracle(c["cats"].tolist(), c["values"], c["C"], 16, 2, 12, 16, 4, 2, 1, 10.0, True)
    o.load_state_dict(c["state_dict"], strict=True)
    return c, o


@pytest.mark.parametrize("case", ["v1", "v3"])
def test_restatement_matches_the_recorded_in_tree_arithmetic(case):
    c, o = load(case)
    x, theta = c["x"], c["theta"]
    made = o.discrete_net.net
    with torch.no_grad():
        idx = made.map_values_to_indices(x[:, 1:])
        assert torch.equal(idx, c["indices"]) and torch.equal(made.map_indices_to_values(idx), c["values_back"])
        lg = o.logits(x, theta).reshape(x.shape[0], -1)
        assert torch.equal(torch.isneginf(lg), torch.isneginf(c["logits"]))
        fin = torch.isfinite(lg)
        assert (lg[fin] - c["logits"][fin]).abs().max() <= 1e-6
        lp_d, lp_c = o.parts(x, theta)
        assert c["discrete_log_prob"].shape == (1, x.shape[0])
        assert (lp_d - c["discrete_log_prob"][0]).abs().max() <= 1e-5
        assert c["log_prob"].shape == (1, x.shape[0])
        assert (lp_d + lp_c - c["log_prob"][0]).abs().max() <= 1e-5
        assert (o.loss(x, theta) - c["loss"]).abs().max() <= 1e-5 and c["loss"].shape == (x.shape[0],)
        for s in range(2):
            assert (o.log_prob(c["x_s"][s], theta) - c["log_prob_s"][s]).abs().max() <= 1e-5
        # sample = recorded categorical draws -> raw values -> inverse flow of the recorded noise -> exp
        vals = made.map_indices_to_values(c["choices"])
        cz = o.condition_embedding(theta[:1]).expand(5, -1)
        z, _ = o.continuous_net.net.inverse_from_noise(c["noise"][:, None], torch.cat((vals, cz), -1))
        got = torch.cat((z.exp(), vals), -1)
        assert c["samples"].shape == (5, 1, x.shape[1])
        assert (got - c["samples"][:, 0]).abs().max() <= 1e-5 * c["samples"].abs().max()
    with pytest.raises(ValueError, match="not seen during training"):
        made.map_values_to_indices(torch.full((1, len(c["values"])), 123.0))
