"""NRE host side without a GPU: factory and config behaviour and refusals, the trainer aliases, the flat parameter
layout against the C ABI and the oracle, the sbi-keyed state-dict round trip, and the per-row loss restatements
against the reference's scalar losses (sbi/inference/trainers/nre/*.py `_loss`, row-major pairs)."""

import pytest
import torch
from torch import nn

from oracle.nsf_oracle import ResidualNet
from sbi_amd import _lib
from sbi_amd.inference.trainers.nre.nre import MODE_A, MODE_B, MODE_BNRE, MODE_C, row_losses_torch
from sbi_amd.neural_nets import ResNetClassifierConfig, classifier_nn
from sbi_amd.neural_nets.estimators.ratio_estimator import RatioHyper


def test_factory_builds_the_resnet_classifier_and_refuses_the_rest():
    est = classifier_nn("resnet", hidden_features=32, num_blocks=3)(torch.randn(50, 3), torch.randn(50, 4))
    assert est.theta_shape == (3,) and est.x_shape == (4,)
    assert est.net.hyper.H == 32 and est.net.hyper.NB == 3
    for model in ("linear", "mlp"):
        with pytest.raises(NotImplementedError, match="resnet"):
            classifier_nn(model)
    with pytest.raises(NotImplementedError, match="resnet"):
        classifier_nn("resnet", dropout_probability=0.1)
    with pytest.raises(NotImplementedError, match="resnet"):
        classifier_nn("resnet", use_batch_norm=True)
    with pytest.raises(NotImplementedError, match="resnet"):
        classifier_nn("resnet", embedding_net_x=nn.Linear(4, 2))
    with pytest.raises(ValueError):
        ResNetClassifierConfig(z_score_input="transform_to_unconstrained")
    cfg = ResNetClassifierConfig()
    assert (cfg.hidden_features, cfg.num_blocks, cfg.dropout_probability, cfg.use_batch_norm) == (50, 2, 0.0, False)
    # z-scoring: independent statistics of the training batch, none = identity
    th = torch.randn(200, 2) * 3 + 1
    e = classifier_nn("resnet", z_score_x="none")(th, torch.randn(200, 5))
    zs = e.net.zstats
    assert torch.allclose(zs[:2], th.mean(0)) and torch.allclose(zs[2:4], th.std(0))
    assert torch.equal(zs[4:9], torch.zeros(5)) and torch.equal(zs[9:], torch.ones(5))
    assert "embedding_net_x.0._mean" not in e.state_dict() and "embedding_net_theta.0._mean" in e.state_dict()


def test_aliases():
    import sbi_amd.inference as inf

    assert inf.NRE is inf.NRE_B is inf.SNRE is inf.SNRE_B is inf.SRE
    assert inf.AALR is inf.NRE_A is inf.SNRE_A
    assert inf.CNRE is inf.NRE_C is inf.SNRE_C
    assert issubclass(inf.BNRE, inf.NRE_A)


def test_sample_with_vi_is_refused():
    import sbi_amd.inference as inf

    with pytest.raises(NotImplementedError, match="mcmc"):
        inf.NRE_B(show_progress_bars=False).build_posterior(sample_with="importance",
                                                            density_estimator=classifier_nn("resnet")(
                                                                torch.randn(20, 2), torch.randn(20, 2)),
                                                            prior=torch.distributions.MultivariateNormal(
                                                                torch.zeros(2), torch.eye(2)))


@pytest.mark.parametrize("D,C,H,NB", [(1, 3, 50, 2), (10, 10, 50, 2), (32, 64, 64, 4), (3, 1, 7, 1)])
def test_parameter_layout_matches_the_abi_and_the_oracle(D, C, H, NB):
    lib = _lib.load()
    h = RatioHyper(D, C, H, NB)
    cfg = h.c_config()
    assert lib.sbi_amd_nre_param_count(cfg) == h.param_count()
    off = h.offsets()
    assert lib.sbi_amd_nre_param_offset(cfg, 0, 0) == off["initial_layer.weight"]
    assert lib.sbi_amd_nre_param_offset(cfg, 0, 1) == off["initial_layer.bias"]
    for b in range(NB):
        for i in range(2):
            assert lib.sbi_amd_nre_param_offset(cfg, 1 + 2 * b + i, 0) == off[f"blocks.{b}.linear_layers.{i}.weight"]
            assert lib.sbi_amd_nre_param_offset(cfg, 1 + 2 * b + i, 1) == off[f"blocks.{b}.linear_layers.{i}.bias"]
    assert lib.sbi_amd_nre_param_offset(cfg, 2 * NB + 1, 0) == off["final_layer.weight"]
    assert lib.sbi_amd_nre_param_offset(cfg, 2 * NB + 1, 1) == off["final_layer.bias"]
    oracle = ResidualNet(D + C, 1, H, None, NB)
    sd = oracle.state_dict()
    assert [k for k, _ in h.entries()] == list(sd.keys())
    assert [tuple(s) for _, s in h.entries()] == [tuple(v.shape) for v in sd.values()]
    assert lib.sbi_amd_nre_packed_floats(cfg) > h.param_count() - 1


def test_envelope_is_refused_not_degraded():
    lib = _lib.load()
    for D, C, H, NB in ((65, 3, 50, 2), (3, 129, 50, 2), (3, 3, 65, 2), (3, 3, 50, 5)):
        assert lib.sbi_amd_nre_param_count(_lib.NREConfigC(D, C, H, NB)) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_nre_param_count(_lib.NREConfigC(0, 3, 50, 2)) == _lib.E_BADARG
    cfg = _lib.NREConfigC(3, 3, 50, 2)
    assert lib.sbi_amd_nre_log_ratio(cfg, None, None, None, None, 4, 4, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_nre_loss_weights(0, None, 4, 2, 1.0, 0.0, 1.0, None, None, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_nre_loss_weights(0, 1, 4, 3, 1.0, 0.0, 1.0, 1, None, None, None) == _lib.E_BADARG
    with pytest.raises(RuntimeError, match="unsupported|not supported"):
        classifier_nn("resnet", hidden_features=65)(torch.randn(10, 2), torch.randn(10, 2))


def test_state_dict_round_trip_with_the_oracle():
    est = classifier_nn("resnet", hidden_features=20, num_blocks=2)(torch.randn(100, 3), torch.randn(100, 4))
    sd = est.state_dict()
    assert "net.initial_layer.weight" in sd and "net.blocks.1.linear_layers.1.bias" in sd
    assert "embedding_net_theta.0._std" in sd and "embedding_net_x.0._mean" in sd and "net.flat_params" not in sd
    oracle = ResidualNet(7, 1, 20, None, 2)
    oracle.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("net.")})
    for k, v in oracle.state_dict().items():
        with torch.no_grad():
            v.add_(0.01)
    other = classifier_nn("resnet", hidden_features=20, num_blocks=2)(torch.randn(100, 3), torch.randn(100, 4))
    new_sd = {"net." + k: v for k, v in oracle.state_dict().items()}
    new_sd.update({k: v for k, v in sd.items() if k.startswith("embedding")})
    other.load_state_dict(new_sd)
    back = other.state_dict()
    for k, v in oracle.state_dict().items():
        assert torch.equal(back["net." + k], v)
    assert torch.equal(other.net.zstats, est.net.zstats)
    # the native two-tensor form loads as well
    est.net._native_state_dict = True
    native = est.state_dict()
    est.net._native_state_dict = False
    assert set(native) == {"net.flat_params", "net.zstats"}
    other.load_state_dict(native)
    assert torch.equal(other.net.flat_params, est.net.flat_params)


def _reference_losses(mode, logits_rowmajor, B, A, gamma, lam):
    """The reference's `_loss` bodies (nre_a.py:165-189, nre_b.py:157-182, nre_c.py:168-248, bnre.py:167-202) on
    row-major logits (pair b * A + a)."""
    if mode in (MODE_A, MODE_BNRE):
        likelihood = torch.sigmoid(logits_rowmajor).squeeze()
        labels = torch.ones(2 * B, dtype=logits_rowmajor.dtype)
        labels[1::2] = 0.0
        loss = nn.BCELoss()(likelihood, labels)
        if mode == MODE_BNRE:
            reg = (torch.sigmoid(logits_rowmajor[0::2]) + torch.sigmoid(logits_rowmajor[1::2]) - 1).mean().square()
            loss = loss + lam * reg
        return loss
    if mode == MODE_B:
        lg = logits_rowmajor.reshape(B, A)
        return -torch.mean(lg[:, 0] - torch.logsumexp(lg, dim=-1))
    K = A - 1
    lm_all, lj = logits_rowmajor
    lm = lm_all.reshape(B, K + 1)[:, 1:]
    lj = lj.reshape(B, K)
    loggamma = torch.tensor(gamma, dtype=lm.dtype).log()
    logK = torch.tensor(K, dtype=lm.dtype).log()
    dm = torch.concat([loggamma + lm, logK.expand((B, 1))], dim=-1)
    dj = torch.concat([loggamma + lj, logK.expand((B, 1))], dim=-1)
    lpm = logK - torch.logsumexp(dm, dim=-1)
    lpj = loggamma + lj[:, 0] - torch.logsumexp(dj, dim=-1)
    pj, pm = gamma / (1 + gamma), 1 / (1 + gamma)
    return -torch.mean(pm * lpm + pj * lpj)


@pytest.mark.parametrize("mode", [MODE_A, MODE_B, MODE_C, MODE_BNRE])
def test_row_losses_restate_the_reference_losses(mode):
    torch.manual_seed(mode)
    B, A, gamma, lam = 37, {MODE_A: 2, MODE_BNRE: 2, MODE_B: 10, MODE_C: 6}[mode], 1.7, 30.0
    if mode == MODE_C:
        K = A - 1
        lm = torch.randn(K + 1, B, dtype=torch.float64) * 3
        lj = torch.randn(K, B, dtype=torch.float64) * 3
        atoms_major = torch.cat([lm.reshape(-1), lj.reshape(-1)])
        ref = _reference_losses(mode, (lm.t().reshape(-1), lj.t().reshape(-1)), B, A, gamma, lam)
    else:
        lg = torch.randn(A, B, dtype=torch.float64) * 3
        lg[0, :3] = 60.0       # BCELoss's log clamp at -100 in play
        atoms_major = lg.reshape(-1)
        ref = _reference_losses(mode, lg.t().reshape(-1), B, A, gamma, lam)
    rows = row_losses_torch(mode, atoms_major, B, A, gamma, lam)
    assert rows.shape == (B,)
    assert torch.allclose(rows.mean(), ref, rtol=1e-12, atol=1e-12)
