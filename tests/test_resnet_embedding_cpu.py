"""ResNetEmbedding1D / ResNetEmbedding2D on the host: the eager route against recordings of the real sbi classes
(tests/golden/resnet_embedding_reference.pt, tools/make_golden_resnet_embedding.py), the fp64 oracle against the same
recordings, the routing reasons, and the host-only part of the C ABI (include/sbi_amd_resnet.h).

Tolerances.  The eager route runs the recorded formula with the same torch operators: it is held to 64 * 2^-24 * max|rec|
(a different summation order inside a GEMM at most).  The fp64 oracle is held to the recording's own fp32 error: at most
23 layers deep here, a few ulp of the running maximum each, 1024 * 2^-24 * max|rec|.
"""

import ctypes
import os

import pytest
import torch
from torch import nn

from sbi_amd import _lib
from sbi_amd.neural_nets import (ResidualBLock, ResNetEmbedding1D, ResNetEmbedding2D, construct_simple_conv_net,
                                 construct_simple_fc_net, zero_pad)
from sbi_amd.neural_nets.embedding_nets import resnet as RN
from tests import resnet_embedding_oracle as O

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "resnet_embedding_reference.pt"),
                    weights_only=False)
CASES = sorted(GOLDEN["cases"])
CLASSES = {"1D": ResNetEmbedding1D, "2D": ResNetEmbedding2D}


def build(kind, kwargs):
    kw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in kwargs.items()}
    if "activation" in kw:
        kw["activation"] = getattr(nn, kw["activation"])
    return CLASSES[kind](**kw)


def close(got, rec, ulps):
    bound = ulps * 2.0**-24 * rec.abs().max().item()
    err = (got.double() - rec.double()).abs().max().item()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("name", CASES)
def test_the_eager_route_gives_the_recorded_numbers(name):
    c = GOLDEN["cases"][name]
    net = build(c["class"], c["kwargs"])
    if c["class"] == "2D":
        assert net.final is None
        net(c["x"].clone())                       # the head exists only after the first forward
    assert list(net.state_dict()) == list(c["state_dict"])
    net.load_state_dict(c["state_dict"], strict=True)
    assert net.kernel_route(c["x"])[0] is False
    out = net(c["x"].clone())
    close(out, c["out"], 64)
    (out * c["wts"]).sum().backward()
    close(O.flat_grad(net), c["grad_flat"], 64)


@pytest.mark.parametrize("name", CASES)
def test_the_oracle_gives_the_recorded_numbers(name):
    c = GOLDEN["cases"][name]
    trunk, out, flat = O.reference(c["state_dict"], c["x"], c["wts"], c["kwargs"])
    close(out, c["out"], 1024)
    close(flat, c["grad_flat"], 1024)
    assert (trunk is None) == (c["class"] == "2D")


def test_the_messages():
    m = GOLDEN["messages"]
    small2d = dict(c_in=1, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8], c_hidden_fc=16,
                   construct_mapping_kwargs={"c_hidden": 6})
    block = dict(is_conv_block=True, construct_mapping=lambda a, b, **kw: nn.Identity(), construct_mapping_kwargs=None,
                 activation=nn.ReLU)
    raising = {
        "zero_pad_rank": lambda: zero_pad(torch.zeros(2, 3, 4), 5),
        "zero_pad_c_out": lambda: zero_pad(torch.zeros(2, 3, 4, 4), 3),
        "stages_blocks": lambda: ResNetEmbedding2D(1, n_stages=3, c_stages=[4, 8, 8]),
        "stages_channels": lambda: ResNetEmbedding2D(1, n_stages=2, blocks_per_stage=[1, 1]),
        "rank_2d": lambda: ResNetEmbedding2D(**small2d)(torch.zeros(2, 16)),
        "rank_1d": lambda: ResNetEmbedding1D(3, 2, n_blocks=1, c_internal=4, c_hidden_final=4)(torch.zeros(2, 3, 1)),
        "zeros_shrinks": lambda: ResidualBLock(c_in=8, c_out=4, change_c_mode="zeros", **block),
        "change_c_mode": lambda: ResidualBLock(c_in=4, c_out=8, change_c_mode="ones", **block),
        "rank_block": lambda: ResidualBLock(
            c_in=4, c_out=4, is_conv_block=False, construct_mapping=construct_simple_fc_net,
            construct_mapping_kwargs={"c_hidden": 4, "activation": nn.ReLU}, activation=nn.ReLU)(torch.zeros(2, 3, 4)),
    }
    assert sorted(raising) == sorted(m)
    for key, fn in raising.items():
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == m[key], key


def test_the_recorded_facts():
    f = GOLDEN["facts"]
    net = ResNetEmbedding1D(c_in=10, c_out=8)
    assert list(net.state_dict()) == f["keys_1d_default"]
    assert [tuple(v.shape) for v in net.state_dict().values()] == f["shapes_1d_default"]
    assert sum(p.numel() for p in net.parameters()) == f["param_count_1d_default"]
    assert type(ResNetEmbedding1D(4, 2, n_blocks=1, c_internal=4, c_hidden_final=4).initial).__name__ == \
        f["initial_identity"] == "Identity"
    assert type(ResNetEmbedding1D(3, 2, n_blocks=1, c_internal=4, c_hidden_final=4).initial).__name__ == \
        f["initial_linear"] == "Linear"
    small2d = dict(c_in=1, n_stages=2, blocks_per_stage=[1, 2], c_stages=[4, 8], c_hidden_fc=16)
    net2d = ResNetEmbedding2D(**small2d, construct_mapping_kwargs={"c_hidden": 6})
    assert list(net2d.state_dict()) == f["keys_2d_before"]
    assert (net2d.final is None) == f["final_2d_before_is_none"] is True
    net2d(torch.zeros(2, 1, 16, 16))
    assert list(net2d.state_dict()) == f["keys_2d_after"]
    assert [tuple(v.shape) for v in net2d.state_dict().values()] == f["shapes_2d_after"]
    # the caller's kwargs dict is written to
    kw1, kw2 = {"c_hidden": 6}, {"c_hidden": 6}
    ResNetEmbedding1D(3, 2, n_blocks=1, c_internal=4, c_hidden_final=4, construct_mapping_kwargs=kw1)
    ResNetEmbedding2D(**small2d, construct_mapping_kwargs=kw2)
    named = lambda kw: {k: (v.__name__ if isinstance(v, type) else v) for k, v in kw.items()}  # noqa: E731
    assert named(kw1) == f["kwargs_1d_after"]
    assert named(kw2) == f["kwargs_2d_after"]
    zeros = ResNetEmbedding2D(**small2d, change_c_mode="zeros", construct_mapping_kwargs={"c_hidden": 6})
    assert type(zeros.blocks[0].residual).__name__ == f["zeros_residual_type"]
    assert list(zeros.state_dict()) == f["keys_2d_zeros_before"]


def test_the_constructors_of_a_mapping():
    fc = construct_simple_fc_net(3, 5, 4, nn.Tanh)
    assert [type(m).__name__ for m in fc] == ["Linear", "Tanh", "Linear", "Tanh", "Linear"]
    assert fc(torch.zeros(2, 3)).shape == (2, 5)
    conv = construct_simple_conv_net(2, 6, 4, nn.ReLU, True)
    assert [m.stride for m in conv if isinstance(m, nn.Conv2d)] == [(2, 2), (1, 1), (1, 1)]
    assert conv(torch.zeros(1, 2, 8, 8)).shape == (1, 6, 4, 4)
    assert zero_pad(torch.ones(1, 2, 3, 3), 5)[:, 2:].abs().sum() == 0


def test_the_routing_reasons_on_the_host():
    x = torch.zeros(4, 10)
    net = ResNetEmbedding1D(10, 4, n_blocks=2, c_internal=16, c_hidden_final=8)
    assert net.kernel_route(x) == (False, "input is not on a ROCm device")
    assert net.kernel_route(x.double()) == (False, "input is not float32")
    net.force_eager = True
    assert net.kernel_route(x) == (False, "force_eager is set")
    tanh = ResNetEmbedding1D(10, 4, n_blocks=2, c_internal=16, c_hidden_final=8, activation=nn.Tanh)
    assert tanh.kernel_route(x) == (False, "activation is not nn.ReLU")
    custom = ResNetEmbedding1D(10, 4, n_blocks=1, c_internal=16, c_hidden_final=8,
                               construct_mapping=lambda a, b, activation: nn.Linear(a, b), construct_mapping_kwargs={})
    assert custom.kernel_route(x)[1].startswith("a custom construct_mapping")
    assert custom(x).shape == (4, 4)
    assert ResNetEmbedding2D(1).kernel_route(x)[0] is False


def config(c_in, c_internal, c_hidden, n_blocks):
    return RN.resnet_config(c_in, c_internal, c_hidden, n_blocks)


def test_param_count_and_offsets_follow_the_state_dict():
    for c_in, ci, ch, nb in [(10, 128, 128, 20), (1, 1, 1, 1), (128, 128, 128, 64), (7, 17, 20, 3), (16, 16, 5, 2)]:
        net = ResNetEmbedding1D(c_in, 3, n_blocks=nb, c_internal=ci, c_hidden_final=4,
                                construct_mapping_kwargs={"c_hidden": ch})
        params = net.kernel_parameters()
        n, offsets = RN.param_count(net.kernel_config())
        assert n == sum(p.numel() for p in params)
        sizes = [p.numel() for p in params]
        assert offsets == [sum(sizes[:i]) for i in range(len(sizes))]
        keys = [k for k in net.state_dict() if not k.startswith("final.")]
        assert len(keys) == len(params) == 6 * nb + (2 if c_in != ci else 0)
        for k, p in zip(keys, params):
            assert net.state_dict()[k].data_ptr() == p.data_ptr(), k


def test_the_envelope_and_bad_arguments():
    E, B = _lib.E_UNSUPPORTED, _lib.E_BADARG
    assert RN.plan(config(1, 1, 1, 1), 1)[0] == 0
    assert RN.plan(config(128, 128, 128, 64), 1)[0] == 0
    assert RN.plan(config(128, 128, 128, 65), 1)[0] == E
    for bad in [(129, 16, 16, 1), (16, 129, 16, 1), (16, 16, 129, 1)]:
        assert RN.plan(config(*bad), 4)[0] == E
        assert RN.param_count(config(*bad))[0] == E
        assert RN.workspace_bytes(config(*bad), 4, True) == E
    for bad in [(0, 16, 16, 1), (16, 0, 16, 1), (16, 16, 0, 1), (16, 16, 16, 0), (-1, 16, 16, 1)]:
        assert RN.plan(config(*bad), 4)[0] == B
        assert RN.param_count(config(*bad))[0] == B
    ok = config(10, 128, 128, 20)
    assert RN.plan(ok, 0)[0] == B
    assert RN.plan(ok, 2**31 - 65)[0] == 0
    assert RN.plan(ok, 2**31 - 64)[0] == E
    lib = _lib.load()
    assert lib.sbi_amd_resnet_plan(None, 4, None, None, None) == B
    assert lib.sbi_amd_resnet_plan(ctypes.byref(ok), 4, None, None, None) == 0
    # null device pointers launch nothing
    assert lib.sbi_amd_resnet_forward(ctypes.byref(ok), None, None, 4, None, None, 0, None) == B
    assert lib.sbi_amd_resnet_backward(ctypes.byref(ok), None, None, 4, None, None, None, None) == B


def test_the_plan_and_the_workspace_formula():
    pad = lambda v: -(-v // 16) * 16  # noqa: E731
    for (c_in, ci, ch, nb), rows in [((10, 128, 128, 20), 200), ((3, 17, 20, 2), 3000), ((16, 16, 4, 64), 5000),
                                     ((10, 128, 128, 20), 65536), ((7, 50, 17, 2), 16385)]:
        cfg = config(c_in, ci, ch, nb)
        rc, tile, lds, splits = RN.plan(cfg, rows)
        assert rc == 0
        assert tile == (16 if rows <= 4096 else 32 if rows <= 16384 else 64)
        panel = 32 if tile == 64 else 64
        assert lds == [(3 * tile * 132 + 2 * panel * 144) * 4] * 2 and lds[0] <= 160 * 1024
        CI, CH, CN, Rp = pad(ci), pad(ch), pad(c_in), -(-rows // 64) * 64
        assert splits == -(-Rp // (64 * -(-(Rp // 64) // min(-(-Rp // 1024), 64))))
        BI = 4 * CI * CH + 2 * CH * CH + 2 * CH + CI
        II = CN * CI + CI if c_in != ci else 0
        PB = 2 * ch * ci + ch * ch + 2 * ch + ci
        PI = ci * c_in + ci if c_in != ci else 0
        image = II + nb * BI
        assert RN.workspace_bytes(cfg, rows, False) == 4 * image
        train = image + (nb + 1) * Rp * CI + 2 * Rp * CI + 4 * Rp * CH + (splits * max(PB, PI) if splits > 1 else 0)
        assert RN.workspace_bytes(cfg, rows, True) == 4 * train
    # sbi's training batch at the defaults is far below the cap, 65 536 rows still under it, 2^17 rows above
    default = config(10, 128, 128, 20)
    assert RN.workspace_bytes(default, 65536, True) < RN.MAX_WORKSPACE_BYTES < RN.workspace_bytes(default, 2**17, True)
