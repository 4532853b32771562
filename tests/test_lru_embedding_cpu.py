"""LRUEmbedding without a device: the reference's surface (defaults, state_dict, messages) from the recording of the
real sbi class, the fp64 oracle (tests/lru_embedding_oracle.py) against that recording, the eager route against the
oracle, and the host-side answers of include/sbi_amd_lru.h.

Parity bound (the bound of tests/test_embedding_nets_gpu.py): the eager route's worst error against the fp64 oracle is
at most 4 x the real class's recorded error against the same oracle, with the floor 16 * 2^-24 * max|ref|.

Oracle against the recording: an LRU output at step t is a sum over at most T recurrence steps of S2 products, then H-
wide sums in the gate, num_blocks times.  With T <= 20, S2, H <= 40 and 2 blocks that is a few hundred fp32 roundings
per entry, growing like their square root (about 16 ulp); the bound is 32 * 2^-24 * max(1, max|ref|)."""
import copy
import ctypes
import inspect
import math
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import LRU, LRUBlock, LRUEmbedding
from sbi_amd.neural_nets.embedding_nets import lru as L
from tests import lru_embedding_oracle as O

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "lru_embedding_reference.pt"), weights_only=False)
CASES = sorted(GOLDEN["cases"])
ULP = 2.0**-24


def oracle_of(case, through="out"):
    kw = case["kwargs"]
    return O.reference(case["state_dict"], case["x"], case["wts"], kw.get("state_dim", 20),
                       kw.get("bidirectional", True), kw.get("aggregate_fcn", "mean"), through)


def loaded(case):
    net = LRUEmbedding(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    return net


def worst(got, ref):
    return (got.detach().double() - ref).abs().max().item()


def test_defaults_are_the_reference_s():
    sig = inspect.signature(LRUEmbedding.__init__).parameters
    want = dict(state_dim=20, hidden_dim=40, num_blocks=2, r_min=0.0, r_max=1.0, phase_max=2 * math.pi,
                bidirectional=True, mode="loop", dropout=0.0, apply_input_normalization=False, aggregate_fcn="mean")
    assert list(sig)[1:3] == ["input_dim", "output_dim"]
    assert {k: sig[k].default for k in want} == want
    assert list(inspect.signature(LRU.__init__).parameters)[1:] == ["input_dim", "state_dim", "r_min", "r_max",
                                                                    "phase_max", "bidirectional", "mode"]
    assert list(inspect.signature(LRUBlock.__init__).parameters)[1:] == [
        "hidden_dim", "state_dim", "r_min", "r_max", "phase_max", "bidirectional", "mode", "dropout",
        "apply_input_normalization"]


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_shapes_and_dtypes_are_the_recorded_ones(name):
    case = GOLDEN["cases"][name]
    got, want = LRUEmbedding(**case["kwargs"]).state_dict(), case["state_dict"]
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert want["lru_blocks.0.lru.B"].dtype == torch.complex64 and want["lru_blocks.0.lru.C"].dtype == torch.complex64


@pytest.mark.parametrize("name", CASES)
def test_the_recorded_state_dict_loads_strictly(name):
    case = GOLDEN["cases"][name]
    net = loaded(case)
    for k, v in net.state_dict().items():
        assert torch.equal(v, case["state_dict"][k]), k
    assert all(isinstance(p, torch.nn.Parameter) for p in net.parameters())


def test_the_initialisation_follows_the_paper():
    torch.manual_seed(0)
    unit = LRU(input_dim=6, state_dim=500, r_min=0.4, r_max=0.9, phase_max=0.5, bidirectional=True, mode="loop")
    lam = unit.lambda_complex.detach()
    assert lam.shape == (1000,) and lam.abs().min() >= 0.4 - 1e-6 and lam.abs().max() <= 0.9 + 1e-6
    assert lam.angle().min() >= 0 and lam.angle().max() <= 0.5 + 1e-6
    # |lambda|^2 is uniform on [r_min^2, r_max^2]
    assert abs((lam.abs() ** 2).mean().item() - (0.4**2 + 0.9**2) / 2) < 0.02
    assert torch.allclose(unit.gamma.detach(), torch.sqrt(1 - lam.abs() ** 2), atol=1e-6)
    # Glorot: the real and imaginary parts have variance 1 / (2 input_dim)
    for m in (unit.B.detach(), unit.C.detach()):
        assert abs(torch.view_as_real(m).var().item() * 12 - 1) < 0.1


def test_error_messages_are_the_recorded_ones():
    msg = GOLDEN["messages"]
    unit = dict(input_dim=4, state_dim=3, r_min=0.0, r_max=1.0, phase_max=1.0, bidirectional=True, mode="loop")
    raising = {
        "num_blocks": (ValueError, lambda: LRUEmbedding(1, 2, num_blocks=0)),
        "radii": (ValueError, lambda: LRUEmbedding(1, 2, r_min=0.5, r_max=0.25)),
        "phase_max": (ValueError, lambda: LRUEmbedding(1, 2, phase_max=7.0)),
        "mode": (ValueError, lambda: LRUEmbedding(1, 2, mode="fft")),
        "aggregate_fcn": (ValueError, lambda: LRUEmbedding(1, 2, aggregate_fcn="max")),
        "input_dim": (ValueError, lambda: LRU(**{**unit, "input_dim": 0})),
        "state_dim": (ValueError, lambda: LRU(**{**unit, "state_dim": 0})),
        "forward_mode": (ValueError, lambda: LRU(**unit)(torch.zeros(2, 5, 4), mode="fft")),
        "state_shape": (AssertionError,
                        lambda: LRU(**unit)(torch.zeros(2, 5, 4), state=torch.zeros(2, 3, dtype=torch.cfloat))),
    }
    assert sorted(raising) == sorted(msg)
    for key, (kind, fn) in raising.items():
        with pytest.raises(kind) as e:
            fn()
        assert str(e.value) == msg[key], key


@pytest.mark.parametrize("name", CASES)
def test_the_oracle_reproduces_the_recording(name):
    case = GOLDEN["cases"][name]
    out, features, grad = oracle_of(case)
    for what, rec, ref in (("out", case["out"], out), ("features", case["features"], features),
                           ("grad", case["grad_flat"], grad)):
        err, bound = worst(rec, ref), 32 * ULP * max(1.0, ref.abs().max().item())
        print(f"{name} {what}: recorded vs oracle {err:.3e} bound {bound:.3e}")
        assert rec.shape == ref.shape and err <= bound, (what, err, bound)


@pytest.mark.parametrize("name", CASES)
def test_the_eager_route_against_the_oracle(name):
    case = GOLDEN["cases"][name]
    net = loaded(case)
    assert not net.kernel_route(case["x"])[0]
    out = net(case["x"])
    (out * case["wts"]).sum().backward()
    grad = L.flat_image([p.grad for p in net.parameters()])
    with torch.no_grad():
        features = net.features(case["x"])
    ref_out, ref_features, ref_grad = oracle_of(case)
    for what, got, rec, ref in (("out", out, case["out"], ref_out), ("features", features, case["features"], ref_features),
                                ("grad", grad, case["grad_flat"], ref_grad)):
        e_m, e_r, scale = worst(got, ref), worst(rec, ref), ref.abs().max().item()
        bound = max(4 * e_r, 16 * ULP * scale)
        print(f"{name} {what}: eager {e_m:.3e} real class {e_r:.3e} max|ref| {scale:.3e} bound {bound:.3e}")
        assert e_m <= bound, (what, e_m, bound)


def test_modes_initial_state_and_bare_units_are_the_same_function():
    torch.manual_seed(1)
    unit = LRU(input_dim=4, state_dim=3, r_min=0.0, r_max=1.0, phase_max=1.0, bidirectional=True, mode="scan")
    u = torch.randn(2, 7, 4)
    assert torch.equal(unit(u), unit(u, mode="loop"))
    state = torch.complex(torch.randn(2, 6), torch.randn(2, 6))
    # x_0 = lambda state + v_0 for the forward half, x_{T-1} = lambda state + v_{T-1} for the reversed one: the state
    # adds C (lambda^(t+1) state) resp. C (lambda^(T-t) state) to the output
    lam, S = unit.lambda_complex, 3
    t = torch.arange(7.0)
    pw = torch.cat([lam[None, :S] ** (t[:, None] + 1), lam[None, S:] ** (7 - t[:, None])], dim=1)      # (T, 2 S)
    want = unit(u) + ((pw[None] * state[:, None]) @ unit.C.mT).real
    assert torch.allclose(unit(u, state=state), want, atol=1e-5)
    blk = LRUBlock(4, 3, 0.0, 1.0, 1.0, True, "loop", 0.0, False)
    y = torch.nn.functional.gelu(blk.lru(u))
    assert torch.allclose(blk(u), y * torch.sigmoid(blk.state_mixing_gate(y)) + u, atol=1e-6)


def test_the_functional_is_the_module_without_its_output_layer():
    for name in ("default", "unidirectional", "last_step", "one_block"):
        case = GOLDEN["cases"][name]
        net = loaded(case)
        with torch.no_grad():
            assert torch.equal(L.lru_functional(case["x"], net.kernel_parameters(), net.dims), net.features(case["x"]))


# ---- host-side answers of the C ABI ------------------------------------------------------------------------------------
def cfg(input_dim=2, hidden_dim=40, state_dim=20, num_blocks=2, bidirectional=1, aggregation=0):
    return L.lru_config((input_dim, hidden_dim, state_dim, num_blocks, bidirectional, aggregation))


def plan_of(c, B=4, T=10):
    lds, fwd = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = _lib.load().sbi_amd_lru_plan(ctypes.byref(c), B, T, ctypes.byref(lds), ctypes.byref(fwd))
    return rc, lds.value, fwd.value


def lds_floats(I, H, S2):
    """the image of include/sbi_amd_lru.h: (backward, forward)"""
    fwd = 2 * S2 + 4 * S2 * H + H * H + 2 * H + 18 * 2 * S2 + 4 * 16 * H
    return fwd + 16 * 2 * S2 + 3 * 16 * H + 16 * I, fwd


def test_param_count_is_the_real_view_numel_of_the_kernel_parameters():
    for kw in (dict(input_dim=2, output_dim=6), dict(input_dim=1, output_dim=4, bidirectional=False, state_dim=5,
                                                      hidden_dim=12), dict(input_dim=3, output_dim=2, num_blocks=3,
                                                                           state_dim=7, hidden_dim=8)):
        net = LRUEmbedding(**kw)
        flat = L.flat_image(net.kernel_parameters())
        assert L.param_count(net.dims) == flat.numel()
        # with output_layer it is every parameter of the module
        everything = L.flat_image(list(net.parameters()))
        assert everything.numel() == flat.numel() + sum(p.numel() for p in net.output_layer.parameters())
        offsets = (ctypes.c_int64 * (1 + net.dims[3]))()
        _lib.load().sbi_amd_lru_param_count(ctypes.byref(L.lru_config(net.dims)), offsets)
        per_block = (flat.numel() - net.dims[1] * (net.dims[0] + 1)) // net.dims[3]
        assert list(offsets) == [0] + [net.dims[1] * (net.dims[0] + 1) + i * per_block for i in range(net.dims[3])]


def test_the_plan_answers_on_the_host():
    lib = _lib.load()
    rc, lds, fwd = plan_of(cfg())
    assert rc == 0 and (lds, fwd) == tuple(4 * n for n in lds_floats(2, 40, 40))
    # the edges of the envelope, inside
    for c, B, T in ((cfg(input_dim=64), 4, 10), (cfg(num_blocks=8), 4, 10), (cfg(), 1, 65535), (cfg(), 32768, 65535),
                    (cfg(state_dim=64, hidden_dim=40), 1, 1), (cfg(state_dim=128, hidden_dim=16, bidirectional=0), 1, 1),
                    (cfg(hidden_dim=128, state_dim=4), 1, 1), (cfg(input_dim=1, hidden_dim=1, state_dim=1, num_blocks=1), 1, 1),
                    (cfg(aggregation=1), 4, 10)):
        assert plan_of(c, B, T)[0] == 0, (list(bytes(c)), B, T)
    # outside
    for c, B, T in ((cfg(input_dim=65), 4, 10), (cfg(hidden_dim=129), 4, 10), (cfg(state_dim=65), 4, 10),
                    (cfg(state_dim=129, bidirectional=0), 4, 10), (cfg(num_blocks=9), 4, 10), (cfg(), 1, 65536),
                    (cfg(), 32769, 65535), (cfg(aggregation=2), 4, 10)):
        assert plan_of(c, B, T)[0] == _lib.E_UNSUPPORTED, (B, T)
    for c, B, T in ((cfg(input_dim=0), 4, 10), (cfg(hidden_dim=0), 4, 10), (cfg(state_dim=0), 4, 10),
                    (cfg(num_blocks=0), 4, 10), (cfg(), 0, 10), (cfg(), 4, 0), (cfg(bidirectional=2), 4, 10)):
        assert plan_of(c, B, T)[0] == _lib.E_BADARG
    assert lib.sbi_amd_lru_plan(None, 4, 10, None, None) == _lib.E_BADARG
    # 160 KiB: the widest block that is resident, and one state more
    H = 72
    S2 = max(s for s in range(1, 129) if 4 * lds_floats(2, H, s)[0] <= 160 * 1024)
    assert 66 <= S2 < 128
    assert plan_of(cfg(hidden_dim=H, state_dim=S2, bidirectional=0))[0] == 0
    rc, lds, _ = plan_of(cfg(hidden_dim=H, state_dim=S2 + 1, bidirectional=0))
    assert rc == _lib.E_LDS and lds == 4 * lds_floats(2, H, S2 + 1)[0] > 160 * 1024
    assert plan_of(cfg(hidden_dim=128, state_dim=64))[0] == _lib.E_LDS


def test_workspace_and_null_pointers_on_the_host():
    lib = _lib.load()
    c = cfg()
    P = L.param_count((2, 40, 20, 2, 1, 0))
    rows, H, W2 = 4 * 10, 40, 80
    assert lib.sbi_amd_lru_workspace_bytes(ctypes.byref(c), 4, 10, 0) == 4 * (2 * rows * H + rows * W2)
    assert lib.sbi_amd_lru_workspace_bytes(ctypes.byref(c), 4, 10, 1) == 4 * (3 * rows * H + 2 * rows * W2 + 4 * P + P)
    # the partial gradients: one row per workgroup, at most 512
    big = lib.sbi_amd_lru_workspace_bytes(ctypes.byref(c), 600, 1, 1)
    assert big == 4 * (3 * 600 * H + 2 * 600 * W2 + 512 * P + P)
    assert lib.sbi_amd_lru_workspace_bytes(ctypes.byref(c), 0, 10, 1) == _lib.E_BADARG
    assert lib.sbi_amd_lru_workspace_bytes(ctypes.byref(c), 4, 65536, 1) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_lru_workspace_bytes(ctypes.byref(cfg(hidden_dim=128, state_dim=64)), 4, 10, 1) == _lib.E_LDS
    # null pointers and bad sizes: nothing is launched (no device is needed to be told so)
    assert lib.sbi_amd_lru_forward(ctypes.byref(c), None, None, 4, 10, None, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_lru_backward(ctypes.byref(c), None, None, 4, 10, None, None, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_lru_forward(ctypes.byref(cfg(hidden_dim=129)), None, None, 4, 10, None, None,
                                   None) == _lib.E_UNSUPPORTED
    assert set(_lib.exported_symbols_lru()) == {"sbi_amd_lru_param_count", "sbi_amd_lru_plan",
                                                "sbi_amd_lru_workspace_bytes", "sbi_amd_lru_forward",
                                                "sbi_amd_lru_backward"}


def test_routing_reasons_on_the_host():
    x = torch.zeros(3, 7, 2)
    net = LRUEmbedding(2, 4)
    assert net.kernel_route(x) == (False, "input is not on a ROCm device")
    assert net.kernel_route(x.double()) == (False, "input is not float32")
    forced = copy.deepcopy(net)
    forced.force_eager = True
    assert forced.kernel_route(x) == (False, "force_eager is set")
    assert LRUEmbedding(2, 4, apply_input_normalization=True).kernel_route(x) == (
        False, "apply_input_normalization (no layer norm in the kernels)")
    drop = LRUEmbedding(2, 4, dropout=0.1)
    assert drop.kernel_route(x) == (False, "dropout in training mode (no dropout in the kernels)")
    assert drop.eval().kernel_route(x) == (False, "input is not on a ROCm device")
    assert LRUEmbedding(2, 4, aggregate_fcn=lambda h: h.amax(dim=1)).kernel_route(x) == (
        False, "aggregate_fcn is a callable")
    # every one of them computes: a fallback, never a refusal
    for m in (net, forced, drop, LRUEmbedding(2, 4, aggregate_fcn=lambda h: h.amax(dim=1))):
        assert m(x).shape == (3, 4)
    assert L.plan_reason(_lib.E_LDS) == "one block's weights plus the time tiles exceed 160 KiB of LDS"
    assert L.plan((2, 40, 20, 2, 1, 0), 0, 5) == _lib.E_BADARG and L.plan((2, 40, 20, 2, 1, 0), 4, 70000) == _lib.E_UNSUPPORTED
