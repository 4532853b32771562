#!/usr/bin/env python
"""Generate tests/golden/causal_cnn_embedding_reference.pt: state_dict, inputs, outputs, pooled causal-stack outputs
and flat parameter gradients of the REAL sbi class `CausalCNNEmbedding`
(sbi/neural_nets/embedding_nets/causal_cnn.py) on seven cases, plus the messages of its assertions and errors.  Every
parameter is moved by 0.2 randn so that every term matters.  Data only; build container only."""

import contextlib
import io
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(in_channels=3, out_channels_per_layer=[5, 7, 4], num_conv_layers=3, kernel_size=3, dilation=[1, 3, 2],
             pool_kernel_size=4)


def small_aggregator(channels, steps, out):
    """a custom aggregator: one convolution over the pooled steps and a linear read-out"""
    return ("small", channels, steps, out)


def build_aggregator(spec):
    _, channels, steps, out = spec
    return nn.Sequential(nn.Conv1d(channels, 6, kernel_size=3, padding=1), nn.Tanh(), nn.Flatten(),
                         nn.Linear(6 * steps, out))


# name: (kwargs without activation / aggregator, activation (class name, kwargs), aggregator spec or None, batch,
# layout of x)
CASES = {
    "default": (dict(input_shape=(400,)), None, None, 3, "bare"),
    "small_flat": (dict(input_shape=(37,), **SMALL), None, small_aggregator(4, 9, 5), 4, "flat"),
    "small_channel_first": (dict(input_shape=(37,), **SMALL), None, small_aggregator(4, 9, 5), 4, "channel_first"),
    "no_dilation": (dict(input_shape=(50,), in_channels=2, out_channels_per_layer=[6, 6], num_conv_layers=2,
                         dilation="none", kernel_size=2, pool_kernel_size=7), None, small_aggregator(6, 7, 4), 3,
                    "channel_first"),
    "exponential": (dict(input_shape=(64,), out_channels_per_layer=[4, 17, 8, 3], num_conv_layers=4,
                         dilation="exponential", kernel_size=4, pool_kernel_size=5), ("LeakyReLU", dict(
                             negative_slope=0.3)), small_aggregator(3, 12, 4), 2, "bare"),
    "relu": (dict(input_shape=(41,), in_channels=2, out_channels_per_layer=[8, 5], num_conv_layers=2,
                  dilation=[2, 2], kernel_size=3, pool_kernel_size=3), ("ReLU", {}), small_aggregator(5, 13, 3), 3,
             "flat"),
    "tanh": (dict(input_shape=(30,), in_channels=2, out_channels_per_layer=[4, 4], num_conv_layers=2,
                  dilation="exponential", kernel_size=2, pool_kernel_size=5), ("Tanh", {}), small_aggregator(4, 6, 3),
             3, "channel_first"),
}


def make(cls, kwargs, activation, aggregator):
    kw = dict(kwargs)
    if activation is not None:
        kw["activation"] = getattr(nn, activation[0])(**activation[1])
    if aggregator is not None:
        kw["aggregator"] = build_aggregator(aggregator)
    with contextlib.redirect_stdout(io.StringIO()):        # the real aggregator builder prints shapes
        return cls(**kw)


def record(cls, kwargs, activation, aggregator, batch, layout, seed):
    torch.manual_seed(100 + seed)
    net = make(cls, kwargs, activation, aggregator)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
    C, T = kwargs.get("in_channels", 1), kwargs["input_shape"][0]
    x = torch.randn(batch, C, T, generator=g) * 1.3 + 0.2
    x = x.reshape(batch, C * T) if layout == "flat" else x.reshape(batch, T) if layout == "bare" else x
    out = net(x)
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    with torch.no_grad():
        features = net.pooling_layer(net.causal_cnns(x.reshape(batch, C, T)))
    return {"kwargs": kwargs, "activation": activation, "aggregator": aggregator, "seed": seed, "layout": layout,
            "state_dict": {k: v.clone() for k, v in net.state_dict().items()}, "x": x.clone(),
            "out": out.detach().clone(), "features": features.clone(), "wts": wts,
            "grad_flat": torch.cat([p.grad.reshape(-1) for p in net.parameters()])}


def message(fn, kind):
    try:
        with contextlib.redirect_stdout(io.StringIO()):
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
    from sbi.neural_nets.embedding_nets.causal_cnn import CausalCNNEmbedding, WaveNetSRLikeAggregator, causalConv1d

    out = {"cases": {name: record(CausalCNNEmbedding, *case, i) for i, (name, case) in enumerate(CASES.items())}}
    out["messages"] = {
        "input_shape_type": message(lambda: CausalCNNEmbedding([400]), AssertionError),
        "input_shape_2d": message(lambda: CausalCNNEmbedding((20, 20)), AssertionError),
        "pool_too_large": message(lambda: CausalCNNEmbedding((100,)), AssertionError),
        "dilation_name": message(lambda: CausalCNNEmbedding((400,), dilation="linear"), ValueError),
        "dilation_type": message(lambda: CausalCNNEmbedding((400,), dilation=(1, 2, 4, 8, 16)), AssertionError),
        "dilation_too_large": message(lambda: CausalCNNEmbedding((400,), dilation=[1, 2, 4, 8, 400]), AssertionError),
        "already_small": message(lambda: CausalCNNEmbedding((200,)), AssertionError),
        "stride_and_dilation": message(lambda: causalConv1d(2, 3, 2, dilation=2, stride=2), AssertionError),
        "channel_sizes": message(lambda: WaveNetSRLikeAggregator(4, 10, 5, kernel_sizes=[3, 3, 3]), AssertionError),
        "stride_sizes": message(lambda: WaveNetSRLikeAggregator(4, 10, 5, stride_sizes=[1]), AssertionError),
        "trailing_shape": message(lambda: CausalCNNEmbedding((400,))(torch.zeros(2, 399)), ValueError),
    }
    path = os.path.join(ROOT, "tests", "golden", "causal_cnn_embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path))
    print(out["messages"])


if __name__ == "__main__":
    main()
