#!/usr/bin/env python
"""Generate tests/golden/cnn_embedding_reference.pt: state_dict, inputs, outputs and flat parameter gradients of the
REAL sbi class `CNNEmbedding` (sbi/neural_nets/embedding_nets/cnn.py) on four small cases in 1-D and 2-D, plus the
messages of its assertions and of its input-shape ValueError.  The seed of every case is the first one on which the
fp64 oracle (tests/cnn_embedding_oracle.py) finds the case well separated, so that a gradient comparison is defined.
Data only; build container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "1d_default": (dict(input_shape=(20,)), 5),
    "1d_c3_k3_p3": (dict(input_shape=(33,), in_channels=3, out_channels_per_layer=[5, 7], kernel_size=3,
                         pool_kernel_size=3, num_linear_units=16, output_dim=6), 4),
    "2d_default": (dict(input_shape=(12, 12)), 4),
    "2d_c2_l1": (dict(input_shape=(9, 11), in_channels=2, out_channels_per_layer=[8], num_conv_layers=1, kernel_size=3,
                      num_linear_layers=3, num_linear_units=24, output_dim=9), 3),
}


def record(cls, kwargs, B, oracle):
    for seed in range(1000):
        torch.manual_seed(100 + seed)
        net = cls(**kwargs)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():      # away from the small default init: every layer matters
            for p in net.parameters():
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        x = torch.randn(B, *net.input_shape, generator=g) * 1.3 + 0.2
        conv = [p for n, p in net.named_parameters() if n.startswith("cnn_subnet")]
        report = []
        oracle.cnn_forward([p.detach().double() for p in conv], x.double(), kwargs.get("pool_kernel_size", 2), report)
        if report[0] >= 1.0:
            break
    else:
        raise RuntimeError("no well separated seed")
    out = net(x)
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    with torch.no_grad():
        features = net.cnn_subnet(x).reshape(B, -1)
    return {"kwargs": kwargs, "seed": seed, "separation": report[0],
            "state_dict": {k: v.clone() for k, v in net.state_dict().items()}, "x": x.clone(),
            "out": out.detach().clone(), "features": features.clone(), "wts": wts,
            "grad_flat": torch.cat([p.grad.reshape(-1) for p in net.parameters()])}


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
    from sbi.neural_nets.embedding_nets.cnn import CNNEmbedding

    sys.path.insert(0, os.path.join(ROOT, "tests"))     # the reference tree has a `tests` package of its own
    import cnn_embedding_oracle as oracle

    out = {"cases": {name: record(CNNEmbedding, kwargs, B, oracle) for name, (kwargs, B) in CASES.items()}}
    net = CNNEmbedding((12,))
    out["messages"] = {
        "shape_not_tuple": message(lambda: CNNEmbedding([8]), AssertionError),
        "shape_3d": message(lambda: CNNEmbedding((4, 4, 4)), AssertionError),
        "channels_mismatch": message(lambda: CNNEmbedding((8,), out_channels_per_layer=[4]), AssertionError),
        "zero_size": message(lambda: CNNEmbedding((6,), num_conv_layers=3, out_channels_per_layer=[2, 2, 2]),
                             AssertionError),
        "wrong_input": message(lambda: net(torch.zeros(2, 7)), ValueError),
        "wrong_input_2d": message(lambda: CNNEmbedding((12, 13), in_channels=2)(torch.zeros(2, 12, 13)), ValueError),
    }
    path = os.path.join(ROOT, "tests", "golden", "cnn_embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), {k: (v["seed"], v["separation"]) for k, v in out["cases"].items()})
    print(out["messages"])


if __name__ == "__main__":
    main()
