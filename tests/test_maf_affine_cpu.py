"""The affine MAF (sbi's default "maf") without a GPU: the CPU oracle's own consistency in fp64, its nflows
state-dict keys, MAFConfig / build_maf / trainer plumbing, every refusal, the host-side mask and de-interleave
tables, and the exported C symbols."""
import ctypes
import dataclasses
import os
import re
import warnings

import pytest
import torch
from torch import nn

from sbi_amd import _build, _lib
from sbi_amd.inference import NLE, NPE
from sbi_amd.neural_nets import MAFConfig, build_maf
from sbi_amd.neural_nets.estimators.maf_affine_flow import MAFAffineHyper, MAFAffineNet, MAFFlow
from sbi_amd.utils.torchutils import BoxUniform
from tests.helpers import linear_gaussian_data
from tests.maf_affine_oracle import MAFOracle, MaskedAffineAutoregressiveTransform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle64(D, C, n=64, **kw):
    theta, x = linear_gaussian_data(n, D, C)
    torch.manual_seed(3)
    o = MAFOracle(theta, x, **kw)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in o.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g))
    return o.double(), theta.double(), x.double()


# ------------------------------------------------------------------ the oracle, fp64, D = 3, C = 2
def test_oracle_log_prob_is_the_change_of_variables():
    o, theta, x = _oracle64(3, 2, hidden_features=16, num_transforms=3)
    lp = o.log_prob(theta[:8], x[:8])[0]
    for i in range(8):
        ctx = o.net._embedding_net(x[i : i + 1])
        f = lambda t: o.net._transform(t[None], context=ctx)[0][0]   # noqa: E731
        J = torch.autograd.functional.jacobian(f, theta[i])
        z = f(theta[i])
        # (the base density's constant is the oracle's own: sbi keeps 0.5 D log(2 pi) rounded to fp32)
        ref = -0.5 * (z * z).sum() - o.net._distribution._log_z + torch.linalg.slogdet(J)[1]
        assert abs(lp[i].item() - ref.item()) <= 1e-10


def test_oracle_transform_jacobian_is_lower_triangular_and_inverse_inverts():
    torch.manual_seed(0)
    tr = MaskedAffineAutoregressiveTransform(3, 16, 2).double()
    with torch.no_grad():
        for p in tr.parameters():
            p.add_(0.5 * torch.randn_like(p))
    z, c = torch.randn(5, 3, dtype=torch.float64), torch.randn(5, 2, dtype=torch.float64)
    for i in range(5):
        J = torch.autograd.functional.jacobian(lambda t: tr(t[None], c[i : i + 1])[0][0], z[i])
        assert torch.equal(torch.triu(J, diagonal=1), torch.zeros(3, 3, dtype=torch.float64))
        assert (torch.diagonal(J) > 0).all()
    y, ld = tr(z, c)
    back, ld_inv = tr.inverse(y, c)
    assert (back - z).abs().max() <= 1e-12
    assert (ld + ld_inv).abs().max() <= 1e-12


def test_oracle_d1_depends_on_the_context_only():
    tr = MaskedAffineAutoregressiveTransform(1, 8, 3).double()
    assert tr.autoregressive_net.initial_layer.mask.sum() == 0          # empty initial mask
    c = torch.randn(4, 3, dtype=torch.float64)
    s1, b1 = tr.scale_and_shift(torch.randn(4, 1, dtype=torch.float64), c)
    s2, b2 = tr.scale_and_shift(torch.randn(4, 1, dtype=torch.float64) * 7, c)
    assert torch.equal(s1, s2) and torch.equal(b1, b2)
    s3, _ = tr.scale_and_shift(torch.zeros(4, 1, dtype=torch.float64), c + 1)
    assert not torch.equal(s1, s3)


def _expected_keys(zt: bool, zx: bool):
    keys = []
    first = 1 if zt else 0
    if zt:
        keys += ["net._transform._transforms.0._shift", "net._transform._transforms.0._scale"]
    for t in range(2):
        a = f"net._transform._transforms.{first + 2 * t}.autoregressive_net."
        keys += [a + "initial_layer.weight", a + "initial_layer.bias", a + "initial_layer.mask",
                 a + "initial_layer.degrees", a + "context_layer.weight", a + "context_layer.bias"]
        for b in range(2):
            keys += [a + f"blocks.{b}.linear.weight", a + f"blocks.{b}.linear.bias", a + f"blocks.{b}.linear.mask",
                     a + f"blocks.{b}.linear.degrees"]
        keys += [a + "final_layer.weight", a + "final_layer.bias", a + "final_layer.mask", a + "final_layer.degrees"]
        keys += [f"net._transform._transforms.{first + 2 * t + 1}._permutation"]
    if zx:
        keys += ["net._embedding_net.0._mean", "net._embedding_net.0._std"]
    return keys


@pytest.mark.parametrize("z", ["independent", "none"])
def test_state_dict_keys_are_nflows(z):
    theta, x = linear_gaussian_data(50, 3, 2)
    o = MAFOracle(theta, x, z_score_theta=z, z_score_x=z, hidden_features=8, num_transforms=2, num_blocks=2)
    want = _expected_keys(z != "none", z != "none")
    assert list(o.state_dict().keys()) == want
    est = build_maf(theta, x, z_score_x=z, z_score_y=z, hidden_features=8, num_transforms=2, num_blocks=2)
    assert sorted(est.state_dict().keys()) == sorted(want)
    # and the exchange is exact both ways, the (2D, H) final layer in nflows' interleaved row order
    est.net.load_nflows_state_dict(o.state_dict())
    sd = est.state_dict()
    for k, v in o.state_dict().items():
        assert torch.equal(sd[k].to(v.dtype), v), k
    assert tuple(sd["net._transform._transforms.%d.autoregressive_net.final_layer.weight" % (z != "none")].shape) == (6, 8)
    o2 = MAFOracle(theta, x, z_score_theta=z, z_score_x=z, hidden_features=8, num_transforms=2, num_blocks=2)
    o2.load_state_dict(sd)
    bad = dict(o.state_dict())
    key = [k for k in bad if k.endswith("final_layer.mask")][0]
    bad[key] = 1 - bad[key]
    with pytest.raises(ValueError, match="mask"):
        est.net.load_nflows_state_dict(bad)


# ------------------------------------------------------------------ MAFConfig / build_maf / trainers
def test_mafconfig_fields_and_defaults_are_the_reference_ones():
    # sbi MAFConfig: _ConditionalDensityConfigBase + _NFlowsFlowConfigBase fields, extra_kwargs; no spline fields
    want = [("z_score_input", "independent"), ("z_score_condition", "independent"), ("embedding_net", nn.Identity),
            ("hidden_features", 50), ("num_transforms", 5), ("num_blocks", 2), ("dropout_probability", 0.0),
            ("use_batch_norm", False), ("dtype", torch.float32), ("extra_kwargs", {})]
    cfg = MAFConfig()
    # (names and defaults, not order: the reference's keyword-only `extra_kwargs` comes first in its fields())
    assert sorted(f.name for f in dataclasses.fields(cfg)) == sorted(n for n, _ in want)
    for name, default in want:
        v = getattr(cfg, name)
        assert type(v) is nn.Identity if name == "embedding_net" else v == default, name
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.hidden_features = 3
    with pytest.raises(ValueError):
        MAFConfig(z_score_input="nope")
    with pytest.raises(ValueError):
        MAFConfig(num_transforms=0)
    assert MAFConfig(z_score_input=None).z_score_input == "none"


def test_mafconfig_repr_shows_non_defaults_only():
    assert repr(MAFConfig()) == "MAFConfig()"
    assert repr(MAFConfig(hidden_features=32, z_score_condition="none")) == \
        "MAFConfig(z_score_condition='none', hidden_features=32)"
    assert repr(MAFConfig(extra_kwargs={"a": 1})) == "MAFConfig(extra_kwargs={'a': 1})"


def test_build_maf_and_config_build():
    theta, x = linear_gaussian_data(100, 4, 6)
    est = MAFConfig(hidden_features=20, num_transforms=3, num_blocks=1).build(theta, x)
    assert isinstance(est, MAFFlow) and isinstance(est.net, MAFAffineNet)
    h = est.net.hyper
    assert (h.D, h.C, h.hidden_features, h.num_transforms, h.num_blocks) == (4, 6, 20, 3, 1)
    assert h.epsilon == 1e-3
    assert est.net.flat_params.numel() == 3 * (20 * 4 + 20 + 20 * 6 + 20 + 20 * 20 + 20 + 8 * 20 + 8)
    assert est.net.supports_atomic is False
    # unrelated kwargs are ignored, like the reference
    build_maf(theta, x, num_bins=7, tail_bound=4.0, num_components=3)
    with pytest.warns(UserWarning, match="one-dimensional"):
        build_maf(theta[:, :1], x)
    # nflows' construction order: the same seed gives the oracle's weights and permutations
    torch.manual_seed(11)
    est = build_maf(theta, x, hidden_features=8, num_transforms=2)
    torch.manual_seed(11)
    o = MAFOracle(theta, x, hidden_features=8, num_transforms=2)
    ref = est.state_dict()
    for k, v in o.state_dict().items():
        assert torch.equal(ref[k].to(v.dtype), v), k


def test_trainers_accept_an_instance_and_reject_the_class():
    prior = BoxUniform(-torch.ones(2), torch.ones(2))
    inf = NPE(prior, density_estimator=MAFConfig(hidden_features=8, num_transforms=1))
    est = inf._build_neural_net(torch.randn(50, 2), torch.randn(50, 4))
    assert isinstance(est, MAFFlow) and tuple(est.input_shape) == (2,) and tuple(est.condition_shape) == (4,)
    inf = NLE(prior, density_estimator=MAFConfig(hidden_features=8, num_transforms=1))
    est = inf._build_neural_net(torch.randn(50, 2), torch.randn(50, 4))      # roles swapped: q(x | theta)
    assert isinstance(est, MAFFlow) and tuple(est.input_shape) == (4,) and tuple(est.condition_shape) == (2,)
    for cls in (NPE, NLE):
        with pytest.raises(TypeError, match="instance"):
            cls(prior, density_estimator=MAFConfig)


def test_the_string_and_default_routes_still_refuse():
    from sbi_amd.neural_nets import likelihood_nn, posterior_nn

    prior = BoxUniform(-torch.ones(2), torch.ones(2))
    theta, x = linear_gaussian_data(64, 2, 3)
    with pytest.raises(NotImplementedError):
        posterior_nn("maf")(theta, x)
    with pytest.raises(NotImplementedError):
        likelihood_nn("maf")
    with pytest.raises(NotImplementedError):
        NLE(prior)
    with pytest.raises(NotImplementedError):
        NLE(prior, density_estimator="maf")


def test_refusals():
    theta, x = linear_gaussian_data(100, 3, 4)
    with pytest.raises(NotImplementedError, match="dropout_probability=0.0"):
        build_maf(theta, x, dropout_probability=0.1)
    with pytest.raises(NotImplementedError, match="use_batch_norm=False"):
        MAFConfig(use_batch_norm=True).build(theta, x)
    with pytest.raises(NotImplementedError, match="NSFConfig"):
        build_maf(theta, x, embedding_net=nn.Linear(4, 3))
    build_maf(theta, x, embedding_net=nn.Flatten())                     # parameter-free: applied in front
    with pytest.raises(ValueError, match="not supported by `build_maf`"):     # as build_maf_rqs refuses it
        build_maf(theta, x, z_score_x="transform_to_unconstrained")
    # a round with a proposal: no split forward / backward, the fused step refuses the atomic loss (as maf_rqs)
    from sbi_amd.inference.trainers.fused import FusedTrainStep

    est = build_maf(theta, x, hidden_features=8, num_transforms=1)
    stepper = object.__new__(FusedTrainStep)
    stepper.est, stepper.net = est, est.net
    with pytest.raises(NotImplementedError, match="autograd path"):
        stepper.atomic_loss_and_grad(theta, x, None, None, 10)
    # multi-GPU training
    inf = NPE(density_estimator=MAFConfig(hidden_features=8, num_transforms=1), show_progress_bars=False)
    inf.append_simulations(theta, x)

    class TwoRanks:                      # an initialised process group, as far as train() looks before the refusal
        def broadcast(self, buf, src=0):
            pass

    inf._dist = lambda: TwoRanks()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match="one device"):
            inf.train()


# ------------------------------------------------------------------ host tables against the oracle's masks
@pytest.mark.parametrize("D,H", [(1, 8), (2, 8), (5, 17), (16, 64)])
def test_host_masks_and_deinterleave_table_agree_with_the_oracle(D, H):
    tr = MaskedAffineAutoregressiveTransform(D, H, 3, num_blocks=1)
    made = tr.autoregressive_net
    h = MAFAffineHyper(D=D, C=3, hidden_features=H, num_blocks=1)
    assert torch.equal(h.mask(0), made.initial_layer.mask)
    assert torch.equal(h.mask(2), made.blocks[0].linear.mask)
    assert torch.equal(h.mask(3), made.final_layer.mask)
    assert torch.equal(h.hidden_degrees(), made.initial_layer.degrees)
    assert torch.equal(h.output_degrees(), made.final_layer.degrees)
    assert h.mask(1) is None
    # image row 16 tile + d holds nflows row 2 d + tile; view(-1, D, 2)[..., tile] picks exactly those rows
    rows = h.final_tile_rows()
    params = torch.arange(2 * D, dtype=torch.float32)[None]
    u, s = tr._unconstrained_scale_and_shift(params)
    assert torch.equal(rows[:D].float(), u[0]) and torch.equal(rows[16 : 16 + D].float(), s[0])
    assert (rows[D:16] == -1).all() and (rows[16 + D :] == -1).all()
    assert [k for k, _, _ in h.layer_entries()][-2:] == ["autoregressive_net.final_layer.weight",
                                                         "autoregressive_net.final_layer.bias"]
    assert h.layer_entries()[-2][1] == (2 * D, H)


# ------------------------------------------------------------------ C ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "sbi_amd_maf_affine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sbi_amd_\w+)\s*\(", text)))


def test_library_exports_the_ten_symbols():
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    syms = _declared()
    assert syms == sorted([
        "sbi_amd_maf_affine_param_count", "sbi_amd_maf_affine_packed_floats", "sbi_amd_maf_affine_param_offset",
        "sbi_amd_maf_affine_plan_waves", "sbi_amd_maf_affine_pack", "sbi_amd_maf_affine_log_prob", "sbi_amd_maf_affine_sample",
        "sbi_amd_maf_affine_train_workspace_floats", "sbi_amd_maf_affine_loss_fwd_bwd",
        "sbi_amd_maf_affine_log_prob_trials"])
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/sbi_amd_maf_affine.h but not exported"
    assert set(syms) == set(_lib.exported_symbols_maf_affine()), "ctypes binding and header disagree"


def test_host_side_layout_answers_and_envelope():
    lib = _lib.load()
    for kw in (dict(D=10, C=10), dict(D=1, C=3, num_transforms=2), dict(D=16, C=32, hidden_features=64, num_blocks=4),
               dict(D=4, C=7, hidden_features=17)):
        h = MAFAffineHyper(**kw)
        cfg = h.c_config()
        assert lib.sbi_amd_maf_affine_param_count(cfg) == h.param_count()
        assert lib.sbi_amd_maf_affine_packed_floats(cfg) > 0
        assert lib.sbi_amd_maf_affine_train_workspace_floats(cfg, 333) > 0
        off, per = 0, h.layer_params()
        names = [k for k, _, _ in h.layer_entries()]
        for (key, shape, _), i in zip(h.layer_entries(), range(len(names))):
            which, bias = i // 2, i % 2
            for t in range(h.num_transforms):
                assert lib.sbi_amd_maf_affine_param_offset(cfg, t, which, bias) == t * per + off, (key, t)
            n = 1
            for s in shape:
                n *= s
            off += n
    for kw in (dict(D=17, C=3), dict(D=3, C=33), dict(D=3, C=3, hidden_features=65), dict(D=3, C=3, num_transforms=17),
               dict(D=3, C=3, num_blocks=5)):
        cfg = MAFAffineHyper(**kw).c_config()
        assert lib.sbi_amd_maf_affine_param_count(cfg) == _lib.E_UNSUPPORTED, kw
        assert lib.sbi_amd_maf_affine_packed_floats(cfg) == _lib.E_UNSUPPORTED, kw
        assert lib.sbi_amd_maf_affine_train_workspace_floats(cfg, 100) == _lib.E_UNSUPPORTED, kw
    cfg = MAFAffineHyper(D=3, C=3).c_config()
    assert lib.sbi_amd_maf_affine_log_prob(cfg, None, None, None, None, 4, 4, None, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_maf_affine_param_count(MAFAffineHyper(D=0, C=3).c_config()) == _lib.E_BADARG
