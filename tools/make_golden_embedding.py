#!/usr/bin/env python
"""Generate tests/golden/embedding_reference.pt: state_dict, inputs, outputs and parameter gradients of the REAL sbi
classes `FCEmbedding` and `PermutationInvariantEmbedding` (sbi/neural_nets/embedding_nets) on small fixed inputs.  The
permutation-invariant cases are drawn from the inputs on which sbi's trial count and ours agree: input_dim == 1 with
varying counts, input_dim == 3 with equal counts, B == 1 with padding -- each under "sum" and "mean".  Data only; build
container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(net, x, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():      # away from the small default init: every layer matters
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
    out = net(x)
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    # the gradient as ONE flat vector in named_parameters() order (= state_dict order): fewer tensors, a smaller file
    return {"state_dict": {k: v.clone() for k, v in net.state_dict().items()}, "x": x.clone(), "out": out.detach().clone(),
            "wts": wts, "grad_flat": torch.cat([p.grad.reshape(-1) for p in net.parameters()])}


def padded(B, T, D, counts, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, D, generator=g) * 1.3 + 0.2
    for b, n in enumerate(counts):
        x[b, n:] = float("nan")
    return x


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # installs the third-party stubs and puts the reference on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.neural_nets.embedding_nets.fully_connected import FCEmbedding
    from sbi.neural_nets.embedding_nets.permutation_invariant import PermutationInvariantEmbedding

    out = {"fc": {}, "perminv": {}}
    torch.manual_seed(11)
    out["fc"]["in3_h50_l2"] = dict(kwargs=dict(input_dim=3, num_hiddens=50, num_layers=2),
                                   **record(FCEmbedding(3, num_hiddens=50, num_layers=2), torch.randn(9, 3) * 1.5, 1))
    out["fc"]["in17_h32_l3"] = dict(kwargs=dict(input_dim=17, output_dim=7, num_hiddens=32, num_layers=3),
                                    **record(FCEmbedding(17, output_dim=7, num_hiddens=32, num_layers=3),
                                             torch.randn(5, 17), 2))
    shapes = {"d1_varying": (6, 5, 1, [5, 1, 3, 2, 4, 1]), "d3_equal": (4, 6, 3, [4, 4, 4, 4]),
              "b1_padded": (1, 7, 3, [3])}
    for name, (B, T, D, counts) in shapes.items():
        trial_kwargs = dict(input_dim=D, output_dim=8, num_hiddens=16, num_layers=2)
        kwargs = dict(trial_net_output_dim=8, num_hiddens=24, num_layers=2, output_dim=5)
        case = dict(trial_kwargs=trial_kwargs, kwargs=kwargs, counts=counts)
        for agg in ("sum", "mean"):     # the same weights and inputs under both aggregations, stored once
            torch.manual_seed(17)
            net = PermutationInvariantEmbedding(FCEmbedding(**trial_kwargs), aggregation_fn=agg, **kwargs)
            rec = record(net, padded(B, T, D, counts, 3), 4)
            case["state_dict"], case["x"] = rec["state_dict"], rec["x"]
            case[agg] = {k: rec[k] for k in ("out", "wts", "grad_flat")}
        out["perminv"][name] = case
    path = os.path.join(ROOT, "tests", "golden", "embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
