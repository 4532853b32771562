"""CausalCNNEmbedding without a GPU: the public surface against the recording of the real sbi class
(tests/golden/causal_cnn_embedding_reference.pt), the eager route's numbers, the host-side answers of the C ABI
(include/sbi_amd_causal_cnn.h) and the fp64 oracle against autograd."""
import ctypes
import inspect
import os

import pytest
import torch
from torch import nn

from sbi_amd import _lib
from sbi_amd.neural_nets import CausalCNNEmbedding, WaveNetSRLikeAggregator, causalConv1d
from sbi_amd.neural_nets.embedding_nets import causal_cnn as C
from tests import causal_cnn_embedding_oracle as O

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "causal_cnn_embedding_reference.pt"),
                    weights_only=False)
MESSAGES = GOLDEN["messages"]
DEFAULTS = (1, 400, (16,) * 5, (1, 2, 4, 8, 16), 2, 160, 0.01)


def raised(fn, kind):
    with pytest.raises(kind) as info:
        fn()
    return str(info.value)


# ---- surface ----------------------------------------------------------------------------------------------------------
def test_signatures_and_defaults():
    p = inspect.signature(CausalCNNEmbedding.__init__).parameters
    assert list(p) == ["self", "input_shape", "in_channels", "out_channels_per_layer", "dilation", "num_conv_layers",
                       "activation", "pool_kernel_size", "kernel_size", "aggregator", "output_dim"]
    assert [p[n].default for n in list(p)[2:] if n != "activation"] == [1, None, "exponential_cyclic", 5, 160, 2, None,
                                                                        20]
    act = p["activation"].default
    assert isinstance(act, nn.LeakyReLU) and act.inplace and act.negative_slope == 0.01
    p = inspect.signature(causalConv1d).parameters
    assert [(n, v.default) for n, v in p.items()][3:] == [("dilation", 1), ("stride", 1)]
    assert list(p)[:3] == ["in_channels", "out_channels", "kernel_size"]
    p = inspect.signature(WaveNetSRLikeAggregator).parameters
    assert list(p) == ["in_channels", "num_timepoints", "output_dim", "activation", "kernel_sizes",
                       "intermediate_channel_sizes", "stride_sizes"]
    assert (p["kernel_sizes"].default, p["intermediate_channel_sizes"].default, p["stride_sizes"].default) == (
        None, None, 1)
    net = CausalCNNEmbedding((400,))
    assert net.dims == DEFAULTS and net.input_shape == (1, 400) and not net.force_eager
    assert [type(m).__name__ for m in net.aggregation] == ["Conv1d", "LeakyReLU", "MaxPool1d", "Conv1d", "LeakyReLU",
                                                           "MaxPool1d", "AdaptiveAvgPool1d"]
    assert (net.aggregation[0].kernel_size, net.aggregation[3].kernel_size) == ((2,), (1,))     # min(9, 2), min(5, 1)
    assert (net.aggregation[0].out_channels, net.aggregation[3].out_channels) == (64, 20)
    cyclic = CausalCNNEmbedding((2000,), num_conv_layers=12, aggregator=nn.Flatten())
    assert cyclic.dims[3] == (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1, 2)
    assert CausalCNNEmbedding((400,), dilation="Exponential", num_conv_layers=3).dims[3] == (1, 2, 4)
    pad, conv = causalConv1d(2, 3, 3, dilation=4)
    assert isinstance(pad, nn.ZeroPad1d) and tuple(pad.padding) == (8, 0)
    assert (conv.dilation, conv.stride, conv.padding, conv.kernel_size) == ((4,), (1,), (0,), (3,))
    assert causalConv1d(2, 3, 3, stride=2)[1].stride == (2,)


def test_messages_equal_the_recording():
    got = {
        "input_shape_type": raised(lambda: CausalCNNEmbedding([400]), AssertionError),
        "input_shape_2d": raised(lambda: CausalCNNEmbedding((20, 20)), AssertionError),
        "pool_too_large": raised(lambda: CausalCNNEmbedding((100,)), AssertionError),
        "dilation_name": raised(lambda: CausalCNNEmbedding((400,), dilation="linear"), ValueError),
        "dilation_type": raised(lambda: CausalCNNEmbedding((400,), dilation=(1, 2, 4, 8, 16)), AssertionError),
        "dilation_too_large": raised(lambda: CausalCNNEmbedding((400,), dilation=[1, 2, 4, 8, 400]), AssertionError),
        "already_small": raised(lambda: CausalCNNEmbedding((200,)), AssertionError),
        "stride_and_dilation": raised(lambda: causalConv1d(2, 3, 2, dilation=2, stride=2), AssertionError),
        "channel_sizes": raised(lambda: WaveNetSRLikeAggregator(4, 10, 5, kernel_sizes=[3, 3, 3]), AssertionError),
        "stride_sizes": raised(lambda: WaveNetSRLikeAggregator(4, 10, 5, stride_sizes=[1]), AssertionError),
        "trailing_shape": raised(lambda: CausalCNNEmbedding((400,))(torch.zeros(2, 399)), ValueError),
    }
    assert got == MESSAGES


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_state_dict_keys_and_strict_loading_both_ways(name):
    case = GOLDEN["cases"][name]
    net = O.golden_net(CausalCNNEmbedding, case)          # the real class's checkpoint loads with strict=True
    ours = net.state_dict()
    # ... and ours into the real class: the same keys in the same order, shapes and dtypes
    assert list(ours) == list(case["state_dict"])
    assert all(ours[k].shape == v.shape and ours[k].dtype == v.dtype for k, v in case["state_dict"].items())
    layers = len(case["kwargs"].get("out_channels_per_layer", [16] * 5))
    assert [k for k in ours if k.startswith("causal_cnns")] == [
        f"causal_cnns.{2 * l}.1.{w}" for l in range(layers) for w in ("weight", "bias")]
    if name == "default":
        assert [k for k in ours if k.startswith("aggregation")] == [
            f"aggregation.{i}.{w}" for i in (0, 3) for w in ("weight", "bias")]


# ---- the eager route --------------------------------------------------------------------------------------------------
def close(got, ref):
    """fp32 rounding of sums of a few hundred terms: 1e-5 of the largest entry"""
    return (got.detach() - ref).abs().max() <= 1e-5 * ref.abs().max()


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_the_eager_route_reproduces_the_recording(name):
    case = GOLDEN["cases"][name]
    net = O.golden_net(CausalCNNEmbedding, case)
    assert net.kernel_route(case["x"])[0] is False
    out = net(case["x"])
    (out * case["wts"]).sum().backward()
    grad = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert out.shape == case["out"].shape and close(out, case["out"])
    assert close(net.features(case["x"]), case["features"])
    assert grad.shape == case["grad_flat"].shape and close(grad, case["grad_flat"])
    # the formula the kernels implement is the same function (where the activation has a slope)
    if net.dims[6] is not None and case["activation"] != ("Tanh", {}):
        C_, T = net.input_shape
        with torch.no_grad():
            assert close(C.causal_functional(case["x"].reshape(-1, C_, T), net.conv_parameters(), net.dims),
                         case["features"])


def test_routing_reasons_on_the_host():
    x = torch.zeros(2, 400)
    net = CausalCNNEmbedding((400,))
    assert net.kernel_route(x) == (False, "input is not on a ROCm device")
    assert net.kernel_route(x.double()) == (False, "input is not float32")
    net.force_eager = True
    assert net.kernel_route(x) == (False, "force_eager is set")
    tanh = CausalCNNEmbedding((400,), activation=nn.Tanh())
    assert tanh.kernel_route(x) == (False, "activation is neither nn.LeakyReLU nor nn.ReLU")
    assert CausalCNNEmbedding((400,), activation=nn.ReLU()).dims[6] == 0.0
    assert CausalCNNEmbedding((400,), activation=nn.LeakyReLU(0.3)).dims[6] == pytest.approx(0.3)


def test_the_three_input_layouts_agree():
    torch.manual_seed(3)
    one = CausalCNNEmbedding((48,), num_conv_layers=2, pool_kernel_size=6)
    x = torch.randn(3, 1, 48)
    with torch.no_grad():
        ref = one(x)
        assert ref.shape == (3, 20)
        assert torch.equal(one(x.reshape(3, 48)), ref)                 # bare and flat coincide for one channel
        assert torch.equal(one.features(x[:, 0]), one.features(x)) and one.features(x).shape == (3, 16, 8)
    two = CausalCNNEmbedding((48,), in_channels=2, num_conv_layers=2, pool_kernel_size=6)
    x = torch.randn(3, 2, 48)
    with torch.no_grad():
        assert torch.equal(two(x.reshape(3, 96)), two(x))
    assert raised(lambda: two(x[:, 0]), ValueError).startswith("Expected flat or channel-first input")


def test_nothing_is_printed_and_a_passed_list_is_not_changed(capsys):
    CausalCNNEmbedding((400,))
    sizes = [12, 9]
    agg = WaveNetSRLikeAggregator(4, 20, 5, kernel_sizes=[3, 3, 3], intermediate_channel_sizes=sizes,
                                  stride_sizes=[1, 1, 1])
    assert capsys.readouterr().out == ""
    assert sizes == [12, 9]
    assert [m.out_channels for m in agg if isinstance(m, nn.Conv1d)] == [12, 9, 5]
    assert [m.kernel_size for m in agg if isinstance(m, nn.MaxPool1d)] == [2, 2, 2]       # 20 -> 10 -> 5 -> 2 steps
    assert agg(torch.zeros(2, 4, 20)).shape == (2, 5, 1)
    assert [m.kernel_size for m in WaveNetSRLikeAggregator(4, 4, 5) if isinstance(m, nn.MaxPool1d)] == [2, 1]


# ---- host-side answers of the C ABI -----------------------------------------------------------------------------------
def full_plan(dims, batch=1):
    tile, bwd, fwd = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = _lib.load().sbi_amd_ccnn_plan(ctypes.byref(C.ccnn_config(dims)), batch, ctypes.byref(tile), ctypes.byref(bwd),
                                       ctypes.byref(fwd))
    return rc, tile.value, bwd.value, fwd.value


def with_(dims, **kw):
    names = ("cin", "T", "couts", "dils", "k", "pool", "slope")
    return tuple(kw.get(n, v) for n, v in zip(names, dims))


def test_the_symbols_are_exported():
    lib = _lib.load()
    assert len(_lib.exported_symbols_causal_cnn()) == 5
    assert all(hasattr(lib, name) for name in _lib.exported_symbols_causal_cnn())


def test_param_count_and_offsets():
    net = CausalCNNEmbedding((37,), in_channels=3, out_channels_per_layer=[5, 7, 4], num_conv_layers=3, kernel_size=3,
                             dilation=[1, 3, 2], pool_kernel_size=4, aggregator=nn.Flatten())
    assert C.param_count(net.dims) == sum(p.numel() for p in net.conv_parameters()) == 5 * 9 + 5 + 7 * 15 + 7 + 4 * 21 + 4
    offsets = (ctypes.c_int64 * 6)()
    assert _lib.load().sbi_amd_ccnn_param_count(ctypes.byref(C.ccnn_config(net.dims)), offsets) == 250
    assert list(offsets) == [0, 45, 50, 155, 162, 246]
    assert C.param_count(DEFAULTS) == 16 * 2 + 16 + 4 * (16 * 32 + 16)
    assert C.receptive_field(DEFAULTS) == 31 and C.receptive_field(net.dims) == 12


def test_the_plan_at_the_defaults_is_the_same_at_every_T():
    answers = {full_plan(with_(DEFAULTS, T=T), B) for T in (320, 400, 10_000, 1 << 20) for B in (1, 200)}
    assert len(answers) == 1
    rc, tile, bwd, fwd = answers.pop()
    assert rc == 0 and tile % 16 == 0 and tile >= 31 and fwd <= bwd <= 160 * 1024
    assert tile == 288                                                 # the figure of the header and the README


@pytest.mark.parametrize("dims", [
    DEFAULTS,
    (3, 37, (5, 7, 4), (1, 3, 2), 3, 4, 0.0),
    (3, 4000, (32,) * 5, (1,) * 5, 3, 160, 0.01),
    (1, 4000, (4,), (1,), 2, 2, 0.3),
    (32, 4000, (32, 32), (1, 2), 3, 7, 0.01),
])
def test_tile_steps_is_a_multiple_of_16_and_at_least_the_receptive_field(dims):
    rc, tile, bwd, fwd = full_plan(dims)
    assert rc == 0 and tile % 16 == 0 and 16 <= tile <= 2048 and tile >= C.receptive_field(dims)
    assert 0 < fwd <= bwd <= 160 * 1024
    assert C.plan(dims, 1) == (0, tile)


def test_the_lds_limit():
    wavenet = (1, 100_000, (16,) * 10, tuple(2 ** i for i in range(10)), 2, 160, 0.01)
    assert C.receptive_field(wavenet) == 1023
    assert full_plan(wavenet)[0] == _lib.E_LDS and C.plan(wavenet, 1)[0] == _lib.E_LDS
    # a tile fits, but none as long as the receptive field
    rc, tile, _, _ = full_plan((1, 4000, (16,) * 8, tuple(2 ** i for i in range(8)), 2, 160, 0.01))
    assert (rc, tile < 255) == (_lib.E_LDS, True)
    assert C.plan_reason(_lib.E_LDS) == "no time tile as long as the receptive field fits 160 KiB of LDS"


def test_the_envelope_edges():
    ok = lambda dims, B=1: full_plan(dims, B)[0]      # noqa: E731
    assert ok(with_(DEFAULTS, cin=32)) == 0 and ok(with_(DEFAULTS, cin=33)) == _lib.E_UNSUPPORTED
    assert ok(with_(DEFAULTS, couts=(16, 16, 16, 16, 32))) == 0
    assert ok(with_(DEFAULTS, couts=(16, 16, 16, 16, 33))) == _lib.E_UNSUPPORTED
    assert [ok(with_(DEFAULTS, k=k)) for k in (1, 2, 4, 5)] == [_lib.E_UNSUPPORTED, 0, 0, _lib.E_UNSUPPORTED]
    assert ok(with_(DEFAULTS, T=1 << 20)) == 0 and ok(with_(DEFAULTS, T=(1 << 20) + 1)) == _lib.E_UNSUPPORTED
    assert ok(with_(DEFAULTS, T=160)) == 0 and ok(with_(DEFAULTS, T=159)) == _lib.E_UNSUPPORTED      # pool <= T
    assert ok(with_(DEFAULTS, T=400, dils=(1, 2, 4, 8, 399))) in (0, _lib.E_LDS)
    assert ok(with_(DEFAULTS, T=400, dils=(1, 2, 4, 8, 400))) == _lib.E_UNSUPPORTED
    assert ok(with_(DEFAULTS, slope=-0.1)) == _lib.E_UNSUPPORTED and ok(with_(DEFAULTS, slope=0.0)) == 0
    sixteen = (1, 400, (4,) * 16, (1,) * 16, 2, 160, 0.01)
    assert ok(sixteen) == 0 and C.plan((1, 400, (4,) * 17, (1,) * 17, 2, 160, 0.01), 1)[0] == _lib.E_UNSUPPORTED
    cfg = C.ccnn_config(sixteen)
    cfg.num_conv_layers = 17
    assert _lib.load().sbi_amd_ccnn_plan(ctypes.byref(cfg), 1, None, None, None) == _lib.E_UNSUPPORTED
    # B C T < 2^31
    long = with_(DEFAULTS, T=1 << 20)
    assert ok(long, 2047) == 0 and ok(long, 2048) == _lib.E_UNSUPPORTED
    # bad arguments
    assert ok(DEFAULTS, 0) == _lib.E_BADARG and C.plan(DEFAULTS, 0)[0] == _lib.E_BADARG
    assert ok(with_(DEFAULTS, cin=0)) == _lib.E_BADARG and ok(with_(DEFAULTS, T=0)) == _lib.E_BADARG
    assert ok(with_(DEFAULTS, couts=(16, 0, 16, 16, 16))) == _lib.E_BADARG
    assert ok(with_(DEFAULTS, dils=(1, 2, 0, 8, 16))) == _lib.E_BADARG and ok(with_(DEFAULTS, pool=0)) == _lib.E_BADARG
    assert _lib.load().sbi_amd_ccnn_plan(None, 1, None, None, None) == _lib.E_BADARG
    # nothing is launched outside: the launchers answer before they touch a pointer
    lib = _lib.load()
    for dims, rc in ((with_(DEFAULTS, cin=33), _lib.E_UNSUPPORTED), (with_(DEFAULTS, cin=0), _lib.E_BADARG)):
        cfg = C.ccnn_config(dims)
        assert lib.sbi_amd_ccnn_forward(ctypes.byref(cfg), None, None, 1, None, None) == rc
        assert lib.sbi_amd_ccnn_backward(ctypes.byref(cfg), None, None, 1, None, None, None, None) == rc
    assert lib.sbi_amd_ccnn_forward(ctypes.byref(C.ccnn_config(DEFAULTS)), None, None, 1, None, None) == _lib.E_BADARG


def test_the_backward_workspace_does_not_grow_with_T():
    lib = _lib.load()
    size = lambda dims, B: lib.sbi_amd_ccnn_workspace_bytes(ctypes.byref(C.ccnn_config(dims)), B)     # noqa: E731
    assert size(with_(DEFAULTS, T=4000), 200) == size(with_(DEFAULTS, T=32_000), 200) == 512 * 2160 * 4
    assert size(with_(DEFAULTS, T=4000), 1) == size(with_(DEFAULTS, T=4000), 4096)
    assert size(with_(DEFAULTS, cin=33), 1) == _lib.E_UNSUPPORTED and size(DEFAULTS, 0) == _lib.E_BADARG


# ---- the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in GOLDEN["cases"].items() if c["activation"] != ("Tanh", {})))
def test_the_oracle_agrees_with_autograd_of_the_fp64_formula(name):
    case = GOLDEN["cases"][name]
    net = O.golden_net(CausalCNNEmbedding, case).double()
    d = net.dims
    x = case["x"].double().reshape(-1, d[0], d[1])
    wts = torch.randn(x.shape[0], d[2][-1], d[1] // d[5], generator=torch.Generator().manual_seed(5)).double()
    pooled, grad = O.reference(O.conv_params(net.state_dict(), len(d[2])), x, wts, d[3], d[5], d[6])
    params = net.conv_parameters()
    out = C.causal_functional(x, params, d)
    auto = torch.cat([g.reshape(-1) for g in torch.autograd.grad((out * wts).sum(), params)])
    assert (pooled - out).abs().max() <= 1e-12 * out.abs().max()
    assert (grad - auto).abs().max() <= 1e-12 * auto.abs().max()
    # and with the module itself, which the recording pins to the real class
    assert (pooled.float() - case["features"]).abs().max() <= 1e-5 * case["features"].abs().max()
