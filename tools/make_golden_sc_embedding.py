#!/usr/bin/env python
"""Generate tests/golden/sc_embedding_reference.pt: state_dict, inputs, outputs and flat parameter gradients of the REAL
sbi class `SpectralConvEmbedding` (sbi/neural_nets/embedding_nets/SC_embedding.py) on eight cases, plus the messages of
its shape error and its modes assertion.  Every parameter is moved by 0.2 randn (both parts of a complex one) so that
every term matters.  The gradient is flat in state_dict order, a complex entry as (re, im) pairs of its complex .grad.
Data only; runs on the CPU, where the reference works; build container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DOC = dict(modes=15, in_channels=3, out_channels=1, conv_channels=5, num_layers=4)

# name: (kwargs, batch, n_points, grid: None (equispaced) / "sorted" (one sorted random grid for all samples) /
# "per_sample" (unsorted, one per sample, in [-1, 2))
CASES = {
    "default": (dict(in_channels=1), 3, 64, None),
    "docstring_equispaced": (DOC, 4, 40, None),
    "docstring_positions": (DOC, 4, 40, "sorted"),
    "modes_at_the_limit_even": (dict(in_channels=2, modes=9, conv_channels=4, num_layers=2), 3, 16, None),
    "modes_at_the_limit_odd": (dict(in_channels=2, modes=9, conv_channels=4, num_layers=2), 3, 17, "sorted"),
    "out_channels": (dict(in_channels=1, modes=6, out_channels=3, conv_channels=7, num_layers=2), 5, 33, None),
    "one_layer": (dict(in_channels=2, modes=4, out_channels=2, conv_channels=3, num_layers=1), 3, 21, "per_sample"),
    "wide": (dict(in_channels=3, modes=5, out_channels=2, conv_channels=17, num_layers=2), 2, 50, "per_sample"),
}


def record(cls, kwargs, batch, n, grid, seed):
    torch.manual_seed(100 + seed)
    net = cls(**kwargs)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g, dtype=p.dtype) * (2 ** 0.5 if p.is_complex() else 1.0))
    cin = kwargs["in_channels"]
    values = torch.randn(batch, cin, n, generator=g) * 1.3 + 0.2
    if grid is None:
        x = values
    else:
        if grid == "sorted":
            pos = torch.sort(torch.rand(n, generator=g))[0].repeat(batch, cin, 1)
        else:
            pos = (3 * torch.rand(batch, 1, n, generator=g) - 1).repeat(1, cin, 1)
        x = torch.stack([values, pos], dim=1)
    out = net(x)
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    assert all(p.grad.dtype == p.dtype for p in net.parameters())
    flat = torch.cat([(torch.view_as_real(p.grad) if p.is_complex() else p.grad).reshape(-1)
                      for p in net.parameters()])
    return {"kwargs": kwargs, "seed": seed, "grid": grid, "state_dict": {k: v.clone() for k, v in
                                                                         net.state_dict().items()},
            "x": x.clone(), "out": out.detach().clone(), "wts": wts, "grad_flat": flat}


def message(fn, kind):
    try:
        fn()
    except kind as e:
        return str(e)
    raise RuntimeError("no error raised")


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # installs the third-party stubs and puts the reference on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.neural_nets.embedding_nets.SC_embedding import SpectralConvEmbedding

    out = {"cases": {name: record(SpectralConvEmbedding, *case, i) for i, (name, case) in enumerate(CASES.items())}}
    out["messages"] = {
        "rank": message(lambda: SpectralConvEmbedding(1)(torch.zeros(2, 64)), ValueError),
        "modes": message(lambda: SpectralConvEmbedding(1)(torch.zeros(2, 1, 17)), AssertionError),
    }
    path = os.path.join(ROOT, "tests", "golden", "sc_embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path))
    print(out["messages"])


if __name__ == "__main__":
    main()
