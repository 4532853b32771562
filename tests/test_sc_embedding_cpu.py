"""SpectralConvEmbedding without a GPU: the public surface against the recording of the real sbi class
(tests/golden/sc_embedding_reference.pt), the eager route's and the fp64 oracle's numbers against it, the gradient
convention of the complex weights, and the host-side answers of the C ABI (include/sbi_amd_sc.h)."""
import ctypes
import inspect
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import VFT, SpectralConv1d_SMM, SpectralConvEmbedding
from sbi_amd.neural_nets.embedding_nets import sc_embedding as S
from tests import sc_embedding_oracle as O

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "sc_embedding_reference.pt"), weights_only=False)
MESSAGES = GOLDEN["messages"]
DEFAULTS = (1, 10, 1, 5, 3)         # (in_channels, modes, out_channels, conv_channels, num_layers)


def raised(fn, kind):
    with pytest.raises(kind) as info:
        fn()
    return str(info.value)


# ---- surface ----------------------------------------------------------------------------------------------------------
def test_signatures_and_defaults():
    p = inspect.signature(SpectralConvEmbedding.__init__).parameters
    assert [(n, v.default) for n, v in p.items()][1:] == [
        ("in_channels", inspect.Parameter.empty), ("modes", 10), ("out_channels", 1), ("conv_channels", 5),
        ("num_layers", 3)]
    p = inspect.signature(VFT.__init__).parameters
    assert list(p)[:5] == ["self", "batch_size", "n_points", "modes", "point_positions"]
    assert p["point_positions"].default is None and p["device"].default is None
    assert list(inspect.signature(SpectralConv1d_SMM.__init__).parameters) == ["self", "in_channels", "out_channels",
                                                                               "modes"]
    for name in ("forward", "last_layer", "compl_mul1d"):
        assert callable(getattr(SpectralConv1d_SMM, name))
    for name in ("forward", "inverse", "make_matrix"):
        assert callable(getattr(VFT, name))
    net = SpectralConvEmbedding(1)
    assert net.dims == DEFAULTS and not net.force_eager
    assert (net.modes, net.in_channels, net.out_channels, net.conv_channels, net.num_layers) == (10, 1, 1, 5, 3)


def test_state_dict_keys_shapes_and_dtypes():
    sd = SpectralConvEmbedding(3, modes=7, out_channels=2, conv_channels=4, num_layers=2).state_dict()
    assert list(sd) == ["fc0.weight", "fc0.bias", "conv_layers.0.weights1", "conv_layers.1.weights1",
                        "w_layers.0.weight", "w_layers.0.bias", "w_layers.1.weight", "w_layers.1.bias",
                        "conv_last.weights1", "fc_last.weight", "fc_last.bias"]
    assert sd["fc0.weight"].shape == (4, 3) and sd["fc_last.weight"].shape == (2, 4)
    assert sd["w_layers.1.weight"].shape == (4, 4, 1) and sd["w_layers.1.bias"].shape == (4,)
    for key in ("conv_layers.0.weights1", "conv_layers.1.weights1", "conv_last.weights1"):
        assert sd[key].shape == (4, 4, 7) and sd[key].dtype == torch.complex64
    assert all(v.dtype == torch.float32 for k, v in sd.items() if "weights1" not in k)


def test_the_initialisation_is_uniform_below_the_scale():
    torch.manual_seed(0)
    conv = SpectralConv1d_SMM(4, 8, 50)
    w = torch.view_as_real(conv.weights1.detach())
    assert conv.scale == 1 / 32 and w.min() >= 0 and w.max() < 1 / 32
    assert abs(w.mean().item() - 1 / 64) < 2e-3 and (conv.in_channels, conv.out_channels, conv.modes) == (4, 8, 50)


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_strict_loading_and_a_state_dict_the_real_class_would_take(name):
    case = GOLDEN["cases"][name]
    net = O.golden_net(SpectralConvEmbedding, case)       # the real class's checkpoint loads with strict=True
    ours = net.state_dict()
    # ... and the reverse as far as it can be checked without the real class: ours has the recorded state_dict's keys
    # in the same order with the same shapes and dtypes
    assert list(ours) == list(case["state_dict"])
    assert all(ours[k].shape == v.shape and ours[k].dtype == v.dtype for k, v in case["state_dict"].items())


def test_messages_equal_the_recording():
    got = {"rank": raised(lambda: SpectralConvEmbedding(1)(torch.zeros(2, 64)), ValueError),
           "modes": raised(lambda: SpectralConvEmbedding(1)(torch.zeros(2, 1, 17)), AssertionError)}
    assert got == MESSAGES
    assert raised(lambda: SpectralConvEmbedding(1)(torch.zeros(2, 2, 1, 3, 17)), ValueError).endswith(
        "torch.Size([2, 2, 1, 3, 17]).")


# ---- the eager route and the oracle against the real class ------------------------------------------------------------
def close(got, ref):
    """the project's row parity: |d| <= 1e-5 (1 + |ref|) element by element"""
    return bool(((got.detach().double() - ref.double()).abs() <= 1e-5 * (1 + ref.double().abs())).all())


def test_the_recording_has_the_cases_the_module_is_used_in():
    cases = GOLDEN["cases"]
    assert len(cases) >= 6
    assert cases["default"]["kwargs"] == dict(in_channels=1) and cases["default"]["x"].shape == (3, 1, 64)
    limits = [(c["kwargs"].get("modes", 10), c["x"].shape[-1]) for c in cases.values()]
    assert any(m == n // 2 + 1 and n % 2 == 0 for m, n in limits) and any(m == n // 2 + 1 and n % 2 for m, n in limits)
    assert any(c["x"].ndim == 4 for c in cases.values()) and any(c["x"].ndim == 3 for c in cases.values())
    assert any(c["kwargs"].get("out_channels", 1) > 1 for c in cases.values())
    assert any(c["kwargs"].get("num_layers", 3) == 1 for c in cases.values())


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_the_eager_route_reproduces_the_recording(name):
    case = GOLDEN["cases"][name]
    net = O.golden_net(SpectralConvEmbedding, case)
    assert net.kernel_route(case["x"]) == (False, "input is not on a ROCm device")
    out = net(case["x"])
    (out * case["wts"]).sum().backward()
    assert all(p.grad.dtype == p.dtype for p in net.parameters())       # complex64 .grad on the spectral weights
    assert out.shape == case["out"].shape and close(out, case["out"])
    grad = O.flat_grad(net)
    assert grad.shape == case["grad_flat"].shape and close(grad, case["grad_flat"])
    # the formula behind the kernel route's double backward is the same function
    with torch.no_grad():
        assert close(S.sc_functional(case["x"], list(net.parameters()), net.dims), case["out"])


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_the_oracle_reproduces_the_recording(name):
    case = GOLDEN["cases"][name]
    out, grad = O.reference(case["state_dict"], case["x"], case["wts"])
    assert out.dtype == torch.float64 and out.shape == case["out"].shape and close(out, case["out"])
    assert grad.shape == case["grad_flat"].shape and close(grad, case["grad_flat"])


def test_the_gradient_convention_of_the_complex_weights():
    """a real-pair gradient (dL/dRe, dL/dIm) handed back through view_as_real arrives as dL/dRe + i dL/dIm, the
    convention of the recorded .grad of the real class"""
    w = torch.nn.Parameter(torch.randn(3, 2, dtype=torch.cfloat))
    pair = torch.view_as_real(w)
    coeff = torch.randn(3, 2, 2)
    (pair * coeff).sum().backward()                       # L = sum cr Re w + ci Im w
    assert w.grad.dtype == torch.complex64
    assert torch.equal(w.grad.real, coeff[..., 0]) and torch.equal(w.grad.imag, coeff[..., 1])
    # and the module's complex .grad is what autograd gives for a complex leaf: L = |w z|^2 has dL/dw* form 2 w |z|^2
    case = GOLDEN["cases"]["one_layer"]
    net = O.golden_net(SpectralConvEmbedding, case)
    (net(case["x"]) * case["wts"]).sum().backward()
    off = sum(p.numel() for p in (net.fc0.weight, net.fc0.bias))
    n = net.conv_layers[0].weights1.numel()
    pairs = case["grad_flat"][off:off + 2 * n].reshape(*net.conv_layers[0].weights1.shape, 2)
    assert close(net.conv_layers[0].weights1.grad.real, pairs[..., 0])
    assert close(net.conv_layers[0].weights1.grad.imag, pairs[..., 1])


def test_vft_and_the_spectral_layer_on_their_own():
    torch.manual_seed(1)
    vft = VFT(2, 16, 5)
    assert vft.V_fwd.shape == (2, 5, 16) and vft.V_inv.shape == (2, 16, 5) and vft.V_fwd.dtype == torch.complex64
    assert (vft.number_points, vft.batch_size, vft.modes) == (16, 2, 5)
    data = torch.randn(2, 16, 3)
    ref = torch.fft.fft(data, dim=1)[:, :5]
    for norm, scale in (("forward", 1 / 16), ("ortho", 1 / 4), ("backward", 1.0)):
        assert (vft.forward(data.to(torch.complex64), norm=norm) - ref * scale).abs().max() < 1e-5
    spectrum = torch.randn(2, 5, 3, dtype=torch.cfloat)
    assert (vft.inverse(spectrum, norm="backward") * 16 - vft.inverse(spectrum)).abs().max() < 1e-5
    assert (vft.inverse(spectrum, norm="ortho") * 4 - vft.inverse(spectrum)).abs().max() < 1e-5
    pos = torch.rand(2, 16)
    moved = VFT(2, 16, 5, pos)
    assert (moved.V_fwd[1, 3] - torch.exp(-2j * torch.pi * 3 * pos[1])).abs().max() < 1e-5
    conv = SpectralConv1d_SMM(3, 3, 5)
    assert conv(data, vft).shape == (2, 16, 3) and conv(data, vft).dtype == torch.float32
    last = conv.last_layer(data, vft)
    coeff = conv.compl_mul1d(vft.forward(data.to(torch.complex64)).permute(0, 2, 1), conv.weights1)    # (2, 3, 5)
    assert last.shape == (2, 10, 3) and torch.allclose(last[:, 0::2], coeff.real.permute(0, 2, 1))
    assert torch.allclose(last[:, 1::2], coeff.imag.permute(0, 2, 1))


def test_routing_reasons_on_the_host():
    net = SpectralConvEmbedding(1)
    x = torch.zeros(2, 1, 64)
    assert net.kernel_route(x) == (False, "input is not on a ROCm device")
    assert net.kernel_route(x.double()) == (False, "input is not float32")
    net.force_eager = True
    assert net.kernel_route(x) == (False, "force_eager is set")


# ---- host-side answers of the C ABI -----------------------------------------------------------------------------------
def full_plan(dims, n_points, batch=1, positions=False, cfg=None):
    bwd, fwd, parts = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    cfg = cfg or S.sc_config(dims, n_points, positions)
    rc = _lib.load().sbi_amd_sc_plan(ctypes.byref(cfg), batch, ctypes.byref(bwd), ctypes.byref(fwd),
                                     ctypes.byref(parts))
    return rc, bwd.value, fwd.value, parts.value


def header_formula(dims, n, positions):
    """the LDS images of include/sbi_amd_sc.h in bytes and `parts`"""
    cin, M, cout, C, L = dims
    r4 = lambda v: (v + 3) // 4 * 4       # noqa: E731
    ceil16 = lambda v: (v + 15) // 16     # noqa: E731
    Mp, Cs = r4(M), C | 1
    P = C * cin + C + (L + 1) * 2 * C * C * M + L * (C * C + C) + cout * C + cout
    tw = r4(2 * M * (n | 1) if positions else 2 * n)
    T1, T2 = ceil16(2 * Mp) * ceil16(C), ceil16(C) * ceil16(max(C, cin) + 1)
    parts = max(1, 8 // T1)
    fwd = tw + 2 * r4(n * Cs) + 2 * 2 * Mp * C + 256 * parts * T1 + r4(C * Cs) + r4(C)
    bwd = tw + (L + 3) * r4(n * Cs) + 3 * 2 * Mp * C + 256 * parts * (2 * T1 + T2) + r4(C * Cs) + r4(C) + P
    return 4 * bwd, 4 * fwd, parts, P


def test_the_symbols_are_exported():
    lib = _lib.load()
    assert len(_lib.exported_symbols_sc()) == 5
    assert all(hasattr(lib, name) for name in _lib.exported_symbols_sc())


def test_param_count_and_offsets_at_the_defaults():
    net = SpectralConvEmbedding(1)
    sizes = [p.numel() * (2 if p.is_complex() else 1) for p in net.parameters()]
    assert S.param_count(DEFAULTS) == sum(sizes) == 2106
    offsets = (ctypes.c_int64 * 14)()
    assert _lib.load().sbi_amd_sc_param_count(ctypes.byref(S.sc_config(DEFAULTS, 64, False)), offsets) == 2106
    assert list(offsets) == [sum(sizes[:i]) for i in range(14)] == [0, 5, 10, 510, 1010, 1510, 1535, 1540, 1565, 1570,
                                                                    1595, 1600, 2100, 2105]


@pytest.mark.parametrize("dims,n", [(DEFAULTS, 64), (DEFAULTS, 500), ((3, 15, 1, 5, 4), 500), ((3, 17, 3, 17, 1), 65),
                                    ((1, 1, 1, 32, 3), 15), ((32, 64, 32, 1, 8), 126), ((2, 16, 3, 16, 3), 31)])
@pytest.mark.parametrize("positions", [False, True])
def test_the_lds_bytes_equal_the_headers_formula(dims, n, positions):
    bwd, fwd, parts, P = header_formula(dims, n, positions)
    assert S.param_count(dims) == P
    assert full_plan(dims, n, 7, positions) == (0 if bwd <= 160 * 1024 else _lib.E_LDS, bwd, fwd, parts)
    assert fwd < bwd


def test_the_defaults_fit_and_the_first_n_points_that_do_not():
    assert full_plan(DEFAULTS, 64)[0] == 0 and full_plan(DEFAULTS, 500, 200, True)[0] == 0
    # the figures of the header and the README
    for positions, longest in ((False, 1041), (True, 666)):
        assert full_plan(DEFAULTS, longest, 1, positions)[0] == 0
        assert full_plan(DEFAULTS, longest + 1, 1, positions)[0] == _lib.E_LDS
        assert header_formula(DEFAULTS, longest, positions)[0] <= 160 * 1024 < header_formula(
            DEFAULTS, longest + 1, positions)[0]
        assert S.plan(DEFAULTS, longest + 1, 1, positions)[0] == _lib.E_LDS
    assert S.plan_reason(_lib.E_LDS) == ("the sample's maps, twiddles and gradient accumulators do not fit 160 KiB of "
                                         "LDS")


def test_the_envelope_edges():
    ok = lambda dims, n=200, B=1, pos=False: full_plan(dims, n, B, pos)[0]      # noqa: E731
    with_ = lambda **kw: tuple(kw.get(k, v) for k, v in zip(("cin", "M", "cout", "C", "L"), DEFAULTS))  # noqa: E731
    assert ok(with_(M=64)) == 0 and ok(with_(M=65)) == _lib.E_UNSUPPORTED
    assert ok(with_(cin=32)) == 0 and ok(with_(cin=33)) == _lib.E_UNSUPPORTED
    assert ok(with_(cout=32)) == 0 and ok(with_(cout=33)) == _lib.E_UNSUPPORTED
    assert ok(with_(C=32, M=1), 50) == 0 and ok(with_(C=33, M=1), 50) == _lib.E_UNSUPPORTED
    assert ok(with_(L=8, M=4)) == 0 and ok(with_(L=9, M=4)) == _lib.E_UNSUPPORTED
    assert ok(with_(M=1, L=1, C=1), 65535) in (0, _lib.E_LDS) and ok(with_(M=1, L=1, C=1), 65536) == _lib.E_UNSUPPORTED
    assert ok(DEFAULTS, 18) == 0 and ok(DEFAULTS, 17) == _lib.E_UNSUPPORTED          # modes <= n_points // 2 + 1
    assert ok(with_(M=1), 1) == 0
    assert ok(with_(cin=32), 500, 134217) == 0 and ok(with_(cin=32), 500, 134218) == _lib.E_UNSUPPORTED   # B C n < 2^31
    # bad arguments
    assert ok(DEFAULTS, 200, 0) == _lib.E_BADARG and S.plan(DEFAULTS, 200, 0, False)[0] == _lib.E_BADARG
    assert _lib.load().sbi_amd_sc_plan(None, 1, None, None, None) == _lib.E_BADARG
    assert ok(with_(cin=0)) == _lib.E_BADARG and ok(with_(M=0)) == _lib.E_BADARG and ok(DEFAULTS, 0) == _lib.E_BADARG
    cfg = S.sc_config(DEFAULTS, 200, False)
    cfg.has_positions = 2
    assert full_plan(None, 0, cfg=cfg)[0] == _lib.E_BADARG
    # nothing is launched outside: the launchers answer before they touch a pointer
    lib = _lib.load()
    for dims, n, rc in ((with_(M=65), 200, _lib.E_UNSUPPORTED), (with_(C=0), 200, _lib.E_BADARG),
                        (DEFAULTS, 5000, _lib.E_LDS), (DEFAULTS, 200, _lib.E_BADARG)):
        cfg = S.sc_config(dims, n, False)
        assert lib.sbi_amd_sc_forward(ctypes.byref(cfg), None, None, 0, 0, None, 0, 1, None, None) == rc
        assert lib.sbi_amd_sc_backward(ctypes.byref(cfg), None, None, 0, 0, None, 0, 1, None, None, None, None) == rc


def test_the_backward_workspace():
    lib = _lib.load()
    size = lambda dims, n, B: lib.sbi_amd_sc_workspace_bytes(ctypes.byref(S.sc_config(dims, n, False)), B)    # noqa: E731
    assert size(DEFAULTS, 64, 3) == 3 * 2106 * 4 and size(DEFAULTS, 500, 200) == 200 * 2106 * 4
    assert size(DEFAULTS, 500, 512) == size(DEFAULTS, 64, 100_000) == 512 * 2106 * 4
    assert size(DEFAULTS, 5000, 1) == _lib.E_LDS and size(DEFAULTS, 64, 0) == _lib.E_BADARG
