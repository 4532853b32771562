#!/usr/bin/env python
"""Generate tests/golden/resnet_embedding_reference.pt: kwargs, state_dict, inputs, outputs and flat parameter gradients
of the REAL sbi classes `ResNetEmbedding1D` / `ResNetEmbedding2D` (sbi/neural_nets/embedding_nets/resnet.py), plus their
error messages and a few recorded facts (entry order and shapes at the defaults, the 2D entry list before and after the
first forward, what the constructors write into the caller's kwargs dict).  Every parameter is moved by a seeded
0.05 randn (activations then stay O(1 - 10) through 20 blocks).  The gradient is flat in `parameters()` order.  An
activation is recorded by its class name in torch.nn.  Sizes are kept small (the file must stay under 1 MB).  Data
only; runs on the CPU, where the reference works; build container only."""

import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (class, kwargs (activation by name), input shape)
CASES = {
    "1d_initial_3": ("1D", dict(c_in=7, c_out=5, n_blocks=3, c_internal=17, c_hidden_final=16,
                                construct_mapping_kwargs={"c_hidden": 20}), (9, 7)),
    "1d_identity_1": ("1D", dict(c_in=24, c_out=4, n_blocks=1, c_internal=24, c_hidden_final=12,
                                 construct_mapping_kwargs={"c_hidden": 16}), (6, 24)),
    "1d_identity_3": ("1D", dict(c_in=16, c_out=3, n_blocks=3, c_internal=16, c_hidden_final=16,
                                 construct_mapping_kwargs={"c_hidden": 24}), (18, 16)),
    "1d_initial_1_c_in_1": ("1D", dict(c_in=1, c_out=2, n_blocks=1, c_internal=5, c_hidden_final=8,
                                       construct_mapping_kwargs={"c_hidden": 4}), (33, 1)),
    "1d_tanh": ("1D", dict(c_in=5, c_out=3, n_blocks=3, c_internal=12, c_hidden_final=16, activation="Tanh",
                           construct_mapping_kwargs={"c_hidden": 10}), (8, 5)),
    "2d_conv_4d": ("2D", dict(c_in=1, c_out=5, c_hidden_fc=16, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8],
                              construct_mapping_kwargs={"c_hidden": 6}), (2, 1, 16, 16)),
    "2d_conv_3d": ("2D", dict(c_in=1, c_out=5, c_hidden_fc=16, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8],
                              construct_mapping_kwargs={"c_hidden": 6}), (2, 16, 16)),
    "2d_zeros_4d": ("2D", dict(c_in=1, c_out=5, c_hidden_fc=16, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8],
                               change_c_mode="zeros", construct_mapping_kwargs={"c_hidden": 6}), (2, 1, 16, 16)),
    "2d_zeros_3d": ("2D", dict(c_in=1, c_out=5, c_hidden_fc=16, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8],
                               change_c_mode="zeros", construct_mapping_kwargs={"c_hidden": 6}), (2, 16, 16)),
}


def build(cls, kwargs):
    kw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in kwargs.items()}
    if "activation" in kw:
        kw["activation"] = getattr(nn, kw["activation"])
    return cls(**kw)


def record(classes, kind, kwargs, shape, seed):
    torch.manual_seed(100 + seed)
    net = build(classes[kind], kwargs)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 1.3 + 0.2
    if kind == "2D":
        net(x.clone())              # the head exists only after the first forward
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    out = net(x.clone())
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in net.parameters()])
    return {"class": kind, "kwargs": kwargs, "seed": seed,
            "state_dict": {k: v.clone() for k, v in net.state_dict().items()},
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
    from sbi.neural_nets.embedding_nets.resnet import (ResidualBLock, ResNetEmbedding1D, ResNetEmbedding2D,
                                                       construct_simple_fc_net, zero_pad)

    classes = {"1D": ResNetEmbedding1D, "2D": ResNetEmbedding2D}
    out = {"cases": {name: record(classes, *case, i) for i, (name, case) in enumerate(CASES.items())}}
    small2d = dict(c_in=1, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8], c_hidden_fc=16,
                   construct_mapping_kwargs={"c_hidden": 6})
    block = dict(is_conv_block=True, construct_mapping=lambda a, b, **kw: nn.Identity(), construct_mapping_kwargs=None,
                 activation=nn.ReLU)
    out["messages"] = {
        "zero_pad_rank": message(lambda: zero_pad(torch.zeros(2, 3, 4), 5), ValueError),
        "zero_pad_c_out": message(lambda: zero_pad(torch.zeros(2, 3, 4, 4), 3), ValueError),
        "stages_blocks": message(lambda: ResNetEmbedding2D(1, n_stages=3, c_stages=[4, 8, 8]), ValueError),
        "stages_channels": message(lambda: ResNetEmbedding2D(1, n_stages=2, blocks_per_stage=[1, 1]), ValueError),
        "rank_2d": message(lambda: build(ResNetEmbedding2D, small2d)(torch.zeros(2, 16)), ValueError),
        "rank_1d": message(lambda: ResNetEmbedding1D(3, 2, n_blocks=1, c_internal=4, c_hidden_final=4)(
            torch.zeros(2, 3, 1)), ValueError),
        "zeros_shrinks": message(lambda: ResidualBLock(c_in=8, c_out=4, change_c_mode="zeros", **block), ValueError),
        "change_c_mode": message(lambda: ResidualBLock(c_in=4, c_out=8, change_c_mode="ones", **block), ValueError),
        "rank_block": message(lambda: ResidualBLock(
            c_in=4, c_out=4, is_conv_block=False, construct_mapping=construct_simple_fc_net,
            construct_mapping_kwargs={"c_hidden": 4, "activation": nn.ReLU}, activation=nn.ReLU)(torch.zeros(2, 3, 4)),
            ValueError),
    }
    default1d = ResNetEmbedding1D(c_in=10, c_out=8)
    net2d = build(ResNetEmbedding2D, small2d)
    before = list(net2d.state_dict().keys())
    final_before = net2d.final
    net2d(torch.zeros(2, 1, 16, 16))
    kw1, kw2 = {"c_hidden": 6}, {"c_hidden": 6}
    ResNetEmbedding1D(3, 2, n_blocks=1, c_internal=4, c_hidden_final=4, construct_mapping_kwargs=kw1)
    ResNetEmbedding2D(**dict(small2d, construct_mapping_kwargs=kw2))
    zeros2d = build(ResNetEmbedding2D, dict(small2d, change_c_mode="zeros"))
    out["facts"] = {
        "keys_1d_default": list(default1d.state_dict().keys()),
        "shapes_1d_default": [tuple(v.shape) for v in default1d.state_dict().values()],
        "param_count_1d_default": sum(p.numel() for p in default1d.parameters()),
        "initial_identity": type(ResNetEmbedding1D(4, 2, n_blocks=1, c_internal=4, c_hidden_final=4).initial).__name__,
        "initial_linear": type(ResNetEmbedding1D(3, 2, n_blocks=1, c_internal=4, c_hidden_final=4).initial).__name__,
        "keys_2d_before": before,
        "final_2d_before_is_none": final_before is None,
        "keys_2d_after": list(net2d.state_dict().keys()),
        "shapes_2d_after": [tuple(v.shape) for v in net2d.state_dict().values()],
        "kwargs_1d_after": {k: (v.__name__ if isinstance(v, type) else v) for k, v in kw1.items()},
        "kwargs_2d_after": {k: (v.__name__ if isinstance(v, type) else v) for k, v in kw2.items()},
        "zeros_residual_type": type(zeros2d.blocks[0].residual).__name__,
        "keys_2d_zeros_before": list(zeros2d.state_dict().keys()),
    }
    path = os.path.join(ROOT, "tests", "golden", "resnet_embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path))
    print(out["messages"])
    print({k: v for k, v in out["facts"].items() if not k.startswith(("keys", "shapes"))})


if __name__ == "__main__":
    main()
