#!/usr/bin/env python
"""Generate tests/golden/lru_embedding_reference.pt: state_dict, inputs, outputs, aggregated hidden states and flat
real-view parameter gradients of the REAL sbi class `LRUEmbedding` (sbi/neural_nets/embedding_nets/lru.py) on five
small cases, plus the messages of its errors.  Every parameter is moved by 0.2 randn (complex noise for B and C) so
that every term matters.  Data only; build container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(state_dim=5, hidden_dim=12)
# name: (kwargs, (batch, T))
CASES = {
    "default": (dict(input_dim=2, output_dim=6), (3, 9)),
    "unidirectional": (dict(input_dim=1, output_dim=4, bidirectional=False, **SMALL), (2, 17)),
    "last_step": (dict(input_dim=3, output_dim=5, aggregate_fcn="last_step", **SMALL), (4, 6)),
    "one_block": (dict(input_dim=2, output_dim=3, num_blocks=1, state_dim=7, hidden_dim=8), (3, 20)),
    "layer_norm": (dict(input_dim=2, output_dim=4, apply_input_normalization=True, **SMALL), (3, 11)),
}


def record(cls, kwargs, shape, seed):
    torch.manual_seed(100 + seed)
    net = cls(**kwargs)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            noise = torch.randn(p.shape, generator=g)
            if p.is_complex():
                noise = torch.complex(noise, torch.randn(p.shape, generator=g))
            p.add_(0.2 * noise)
    x = torch.randn(*shape, kwargs["input_dim"], generator=g) * 1.3 + 0.2
    out = net(x)
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    with torch.no_grad():
        features = net.aggregation(net.lru_blocks(net.input_layer(x)))
    real = lambda t: torch.view_as_real(t) if t.is_complex() else t     # noqa: E731
    return {"kwargs": kwargs, "seed": seed, "state_dict": {k: v.clone() for k, v in net.state_dict().items()},
            "x": x.clone(), "out": out.detach().clone(), "features": features.clone(), "wts": wts,
            "grad_flat": torch.cat([real(p.grad).reshape(-1) for p in net.parameters()])}


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
    from sbi.neural_nets.embedding_nets.lru import LRU, LRUEmbedding

    out = {"cases": {name: record(LRUEmbedding, kwargs, shape, i)
                     for i, (name, (kwargs, shape)) in enumerate(CASES.items())}}
    unit = dict(input_dim=4, state_dim=3, r_min=0.0, r_max=1.0, phase_max=1.0, bidirectional=True, mode="loop")
    out["messages"] = {
        "num_blocks": message(lambda: LRUEmbedding(1, 2, num_blocks=0), ValueError),
        "radii": message(lambda: LRUEmbedding(1, 2, r_min=0.5, r_max=0.25), ValueError),
        "phase_max": message(lambda: LRUEmbedding(1, 2, phase_max=7.0), ValueError),
        "mode": message(lambda: LRUEmbedding(1, 2, mode="fft"), ValueError),
        "aggregate_fcn": message(lambda: LRUEmbedding(1, 2, aggregate_fcn="max"), ValueError),
        "input_dim": message(lambda: LRU(**{**unit, "input_dim": 0}), ValueError),
        "state_dim": message(lambda: LRU(**{**unit, "state_dim": 0}), ValueError),
        "forward_mode": message(lambda: LRU(**unit)(torch.zeros(2, 5, 4), mode="fft"), ValueError),
        "state_shape": message(lambda: LRU(**unit)(torch.zeros(2, 5, 4), state=torch.zeros(2, 3, dtype=torch.cfloat)),
                               AssertionError),
    }
    path = os.path.join(ROOT, "tests", "golden", "lru_embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path))
    print(out["messages"])


if __name__ == "__main__":
    main()
