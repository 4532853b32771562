"""CNNEmbedding without a GPU: the eager route and the fp64 oracle (tests/cnn_embedding_oracle.py) against the recorded
outputs of the real sbi class (tests/golden/cnn_embedding_reference.pt, tools/make_golden_cnn_embedding.py), the
module's surface, the host-side plan and the routing reasons.

Bounds: forward within 1e-6 (1 + |ref|), flat gradient within 1e-5 (1 + |ref|): fp32 against fp32 on one host (the
project's row bound); the fp64 oracle against the fp32 recording to the same bounds."""
import ctypes
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import CNNEmbedding, calculate_filter_output_size, get_new_cnn_output_size
from sbi_amd.neural_nets.embedding_nets import cnn as C
from tests import cnn_embedding_oracle as O

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "cnn_embedding_reference.pt"), weights_only=False)
CASES = sorted(GOLDEN["cases"])


def within(got, ref, tol):
    return bool(((got.double() - ref.double()).abs() <= tol * (1 + ref.double().abs())).all())


def loaded(case):
    net = CNNEmbedding(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    return net


def flat_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


@pytest.mark.parametrize("name", CASES)
def test_the_eager_route_reproduces_the_real_class(name):
    case = GOLDEN["cases"][name]
    net = loaded(case)
    assert list(net.state_dict()) == list(case["state_dict"])
    assert net.kernel_route(case["x"]) == (False, "input is not on a ROCm device")
    out = net(case["x"])
    (out * case["wts"]).sum().backward()
    assert within(out, case["out"], 1e-6)
    assert within(flat_grad(net), case["grad_flat"], 1e-5)
    with torch.no_grad():
        assert within(net.cnn_subnet(case["x"]).reshape(len(case["x"]), -1), case["features"], 1e-6)


@pytest.mark.parametrize("name", CASES)
def test_the_oracle_agrees_with_the_real_class(name):
    case = GOLDEN["cases"][name]
    net = loaded(case)
    conv = net.conv_parameters()
    pk = net.dims[5]
    # the recorded gradient of the whole module gives d loss / d features through the head; the head is eager fp32
    features = O.cnn_forward([p.detach().double() for p in conv], case["x"].double(), pk)
    assert within(features, case["features"], 1e-6)
    f32 = features.float().requires_grad_(True)
    (net.linear_subnet(f32) * case["wts"]).sum().backward()
    _, grad, separation, _ = O.cnn_reference(conv, case["x"], f32.grad, pk)
    n = sum(p.numel() for p in conv)
    assert separation >= 1.0, separation
    assert within(grad, case["grad_flat"][:n], 1e-5)


def test_messages_match_the_real_class():
    want = GOLDEN["messages"]
    with pytest.raises(AssertionError) as e:
        CNNEmbedding([8])
    assert str(e.value) == want["shape_not_tuple"]
    with pytest.raises(AssertionError) as e:
        CNNEmbedding((4, 4, 4))
    assert str(e.value) == want["shape_3d"]
    with pytest.raises(AssertionError) as e:
        CNNEmbedding((8,), out_channels_per_layer=[4])
    assert str(e.value) == want["channels_mismatch"]
    with pytest.raises(AssertionError) as e:
        CNNEmbedding((6,), num_conv_layers=3, out_channels_per_layer=[2, 2, 2])
    assert str(e.value) == want["zero_size"]
    with pytest.raises(ValueError) as e:
        CNNEmbedding((12,))(torch.zeros(2, 7))
    assert str(e.value) == want["wrong_input"]
    with pytest.raises(ValueError) as e:
        CNNEmbedding((12, 13), in_channels=2)(torch.zeros(2, 12, 13))
    assert str(e.value) == want["wrong_input_2d"]
    conv, pool = torch.nn.Conv1d(1, 2, 5, padding=1), torch.nn.MaxPool1d(2)
    with pytest.raises(AssertionError, match="input shape must be Tuple."):
        get_new_cnn_output_size([12], conv, pool)
    with pytest.raises(AssertionError, match="input shape must be 1 or 2d."):
        get_new_cnn_output_size((1, 2, 3), conv, pool)
    assert get_new_cnn_output_size((12,), conv, pool) == (5,)
    assert calculate_filter_output_size(28, 1, 1, 5, 1) == 26 and calculate_filter_output_size(26, 0, 1, 2, 2) == 13


def test_defaults_and_the_three_input_layouts():
    net = CNNEmbedding((12, 12))
    assert net.input_shape == (1, 12, 12) and net.dims == (2, 1, (12, 12), (6, 12), 5, 2)
    assert [type(m).__name__ for m in net.cnn_subnet] == ["Conv2d", "ReLU", "MaxPool2d"] * 2
    assert net.linear_subnet.dims == (12, 50, 20, 2)
    x = torch.randn(3, 12, 12)
    with torch.no_grad():
        a, b, c = net(x), net(x.reshape(3, 1, 12, 12)), net(x.reshape(3, 144))
    assert a.shape == (3, 20) and torch.equal(a, b) and torch.equal(a, c)
    rgb = CNNEmbedding((12,), in_channels=3)
    with torch.no_grad():
        assert rgb(torch.randn(2, 3, 12)).shape == (2, 20) and rgb(torch.randn(2, 36)).shape == (2, 20)
    with pytest.raises(ValueError, match="Expected flat or channel-first input"):
        rgb(torch.randn(2, 12))          # the bare spatial layout needs in_channels == 1


PLAN_NETS = [dict(input_shape=(20,)), dict(input_shape=(28, 28)), dict(input_shape=(9, 17), in_channels=3,
             out_channels_per_layer=[4, 4, 4], num_conv_layers=3, kernel_size=3),
             dict(input_shape=(33,), in_channels=3, out_channels_per_layer=[5, 17], kernel_size=3, pool_kernel_size=3)]


@pytest.mark.parametrize("kwargs", PLAN_NETS, ids=lambda k: "x".join(map(str, k["input_shape"])))
def test_counts_on_the_host_match_the_module(kwargs):
    net = CNNEmbedding(**kwargs)
    conv = net.conv_parameters()
    assert C.param_count(net.dims) == sum(p.numel() for p in conv)
    assert C.feature_count(net.dims) == net.linear_subnet.dims[0]
    offsets = (ctypes.c_int64 * (2 * len(net.dims[3])))()
    _lib.load().sbi_amd_cnn_param_count(ctypes.byref(C.cnn_config(net.dims)), offsets)
    starts, at = [], 0
    for p in conv:
        starts.append(at)
        at += p.numel()
    assert list(offsets) == starts
    assert C.plan(net.dims, 200) == 0
    lds = ctypes.c_int32()
    assert _lib.load().sbi_amd_cnn_plan(ctypes.byref(C.cnn_config(net.dims)), 200, ctypes.byref(lds), None) == 0
    assert lds.value == O.lds_bytes(net.dims[2], net.dims[1], net.dims[3], net.dims[4], net.dims[5])


def test_the_plan_answers_on_the_host():
    base = (1, 1, (100,), (6, 12), 5, 2)
    assert C.plan(base, 200) == 0
    assert C.plan((1, 1, (100,), (6, 12), 9, 2), 200) == _lib.E_UNSUPPORTED          # kernel_size 9
    assert C.plan((1, 1, (100,), (6, 33), 5, 2), 200) == _lib.E_UNSUPPORTED          # out_channels 33
    assert C.plan((1, 9, (100,), (6, 12), 5, 2), 200) == _lib.E_UNSUPPORTED
    assert C.plan((1, 1, (100,), (6, 12), 5, 5), 200) == _lib.E_UNSUPPORTED
    assert C.plan((1, 1, (100,), (6, 12, 6, 6, 6), 3, 2), 200) == _lib.E_UNSUPPORTED
    assert C.plan(base, 2**31) == _lib.E_UNSUPPORTED
    assert C.plan((1, 1, (6,), (6, 12), 5, 2), 200) == _lib.E_BADARG                 # shrinks to 0 at layer 2
    assert C.plan((2, 1, (12, 3), (6, 12), 5, 2), 200) == _lib.E_BADARG
    assert C.plan(base, 0) == _lib.E_BADARG
    assert C.plan((1, 0, (100,), (6, 12), 5, 2), 1) == _lib.E_BADARG
    assert C.plan((3, 1, (100,), (6, 12), 5, 2), 1) == _lib.E_BADARG
    lib = _lib.load()
    assert lib.sbi_amd_cnn_plan(None, 1, None, None) == _lib.E_BADARG
    cfg = C.cnn_config(base)
    assert lib.sbi_amd_cnn_forward(ctypes.byref(cfg), None, None, 1, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_cnn_backward(ctypes.byref(cfg), None, None, 1, None, None, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_cnn_workspace_bytes(ctypes.byref(cfg), 0) == _lib.E_BADARG
    assert lib.sbi_amd_cnn_workspace_bytes(ctypes.byref(cfg), 200) == 200 * C.param_count(base) * 4
    assert lib.sbi_amd_cnn_workspace_bytes(ctypes.byref(cfg), 1024) == 512 * C.param_count(base) * 4
    # batches above 1024 are left to eager torch, which measured faster there: plan and launchers agree
    assert C.plan(base, 1024) == 0 and C.plan(base, 1025) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_cnn_workspace_bytes(ctypes.byref(cfg), 1025) == _lib.E_UNSUPPORTED
    assert C.plan_reason(_lib.E_UNSUPPORTED, 1025) == "batch above 1024: eager torch measured faster there"
    assert C.plan_reason(_lib.E_UNSUPPORTED, 200).startswith("shape outside the kernel envelope")


def test_a_1d_input_too_long_to_be_resident_is_e_lds():
    # the documented image of the default 1-D stack grows by about 17.5 floats per input element: find the edge
    fits = lambda n: O.lds_bytes((n,), 1, (6, 12), 5, 2) <= 160 * 1024      # noqa: E731
    n = 100
    while fits(n + 1):
        n += 1
    assert 1000 < n < 4000
    assert C.plan((1, 1, (n,), (6, 12), 5, 2), 200) == 0
    assert C.plan((1, 1, (n + 1,), (6, 12), 5, 2), 200) == _lib.E_LDS
    assert C.plan((1, 1, (2**20,), (6, 12), 5, 2), 200) == _lib.E_LDS
    assert C.plan((2, 8, (2**20, 2**20), (32, 32), 1, 2), 200) == _lib.E_LDS
    assert C.feature_count((1, 1, (2**20,), (6, 12), 5, 2)) == 12 * (((2**20 - 2) // 2 - 2) // 2)
    net = CNNEmbedding((n + 1,))
    assert C.plan_reason(C.plan(net.dims, 5)) == "weights plus one sample's maps exceed 160 KiB of LDS"


def test_routing_reasons_on_the_host():
    net = CNNEmbedding((12,))
    assert net.static_route() == (True, "kernel")
    assert net.kernel_route(torch.zeros(2, 12)) == (False, "input is not on a ROCm device")
    assert net.kernel_route(torch.zeros(2, 12, dtype=torch.float64)) == (False, "input is not float32")
    net.force_eager = True
    assert net.static_route() == (False, "force_eager is set")
    assert net.kernel_route(torch.zeros(2, 12)) == (False, "force_eager is set")
    assert not CNNEmbedding.force_eager
