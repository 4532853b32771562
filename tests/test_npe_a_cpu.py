"""NPE-A without a GPU: the binding of include/sbi_amd_mog.h, the eager route of the mixture algebra against the
recorded outputs of the real sbi functions (tests/golden/npe_a_reference.pt) and the fp64 restatement
(tests/npe_a_oracle.py), the ``MoG`` surface, the trainer's constructor / bookkeeping / proposal rules with sbi's
messages, and ``NPE_A_Posterior`` on a stubbed network mixture."""

import os
import re
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd import _lib
from sbi_amd.inference import NPE, NPE_A, SNPE_A, NPE_A_Posterior
from sbi_amd.inference.trainers.npe.npe import PosteriorEstimatorTrainer
from sbi_amd.neural_nets import MDNConfig
from sbi_amd.neural_nets.estimators import mog_ops
from sbi_amd.neural_nets.estimators.mdn import MixtureDensityEstimator, MoG
from sbi_amd.neural_nets.net_builders.mdn import build_mdn
from sbi_amd.utils.parity import row_parity
from sbi_amd.utils.torchutils import BoxUniform
from tests import npe_a_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "npe_a_reference.pt")
KEYS = ["d1k3l1_prior", "d1k3l1_uniform", "d3k4l2_prior", "d3k4l2_uniform"]


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "sbi_amd_mog.h")).read()
    declared = set(re.findall(r"\b(sbi_amd_mog_[a-z_]+)\s*\(", text))
    assert declared == set(_lib.exported_symbols_mog()) and len(declared) == 4
    others = [getattr(_lib, n) for n in dir(_lib) if n.startswith("exported_symbols") and n != "exported_symbols_mog"]
    assert len(others) >= 10
    for fn in others:
        assert not declared & set(fn()), fn.__name__
    lib = _lib.load()
    assert lib.sbi_amd_mog_correct_workspace_bytes(3, 4, 2, 3, 1) == 8 * 18 * (3 * 4 + 2)
    assert lib.sbi_amd_mog_correct_workspace_bytes(1, 4, 2, 17, 1) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_mog_correct_workspace_bytes(1, 65537, 1, 3, 1) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_mog_correct_workspace_bytes(2, 4, 2, 3, 3) == _lib.E_BADARG


# ------------------------------------------------------------------------------------------------ the eager route
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("key", KEYS)
def test_eager_route_matches_the_recorded_reference_outputs(key, dtype):
    """fp64: the same numbers as sbi's functions to 1e-12; fp32: the project's row parity 1e-5 (1 + |ref|)."""
    c = torch.load(GOLDEN)[key]
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    d, p = (tuple(t.to(dtype) for t in c[k]) for k in ("density", "proposal"))
    prior = None
    if "prior_mean" in c:
        prior = MoG.from_gaussian(c["prior_mean"].to(dtype), c["prior_cov"].to(dtype))
        for got, want in zip((prior.logits, prior.means, prior.precisions, prior.precision_factors), c["from_gaussian"]):
            assert row_parity(got, want, tol)["exceed_frac"] == 0.0
    post = mog_ops.correct_for_proposal(MoG(*d), MoG(*p), prior)
    assert post.num_components == c["K"] * c["L"] and post.dim == c["D"] and post.dtype == dtype
    for got, want in zip((post.logits, post.means, post.precisions, post.precision_factors), c["corrected"]):
        assert row_parity(got, want, tol)["exceed_frac"] == 0.0
    rec = MoG(*(t.to(dtype) for t in c["corrected"]))
    for theta, want in ((c["theta"], c["log_prob"]), (c["theta"][0], c["log_prob_2d"])):
        got = rec.log_prob(theta.to(dtype))
        assert got.shape == want.shape and row_parity(got, want, tol)["exceed_frac"] == 0.0
    B, S = c["choices"].shape
    comp = c["choices"].T.reshape(-1)                                       # rows sample-major: i = s B + b
    zeta = c["z"][..., 0].transpose(0, 1).reshape(S * B, -1).to(dtype)
    got = mog_ops.mog_sample(rec.logits, rec.means, rec.precision_factors, zeta, comp=comp)
    assert row_parity(got.reshape(S, B, -1), c["samples"], tol)["exceed_frac"] == 0.0


@pytest.mark.parametrize("case", [(10, 10, 10, 5, 1, True), (16, 16, 4, 3, 3, False), (2, 3, 5, 4, 4, True)])
def test_eager_route_matches_the_restatement(case):
    D, K, L, B, rows, prior = case
    d, p, m0, P0 = oracle.recipe(D, K, L, B, rows, prior)
    ref = oracle.correct(d, p, m0, P0)
    got = mog_ops.correct_eager(d[0], d[1], d[2], p[0], p[1], p[2], m0, P0)
    assert not got[4].any()
    for g, r in zip(got, ref):
        assert row_parity(g, r)["exceed_frac"] == 0.0
    mix = tuple(t.float() for t in ref)
    g = torch.Generator().manual_seed(1)
    shift, scale = 0.3 * torch.randn(D, generator=g), 0.5 + torch.rand(D, generator=g)
    for mog_rows, n in ((1, 37), (B, 3 * B), (B, 3 * B + 1)):
        m = tuple(t[:mog_rows] for t in mix)
        theta = 0.6 * torch.randn(n, D, generator=g) * scale + shift
        assert row_parity(mog_ops.log_prob_eager(*m, theta, shift, scale),
                          oracle.log_prob(*m, theta, shift, scale))["exceed_frac"] == 0.0
        zeta, u = torch.randn(n, D, generator=g), torch.rand(n, generator=g)
        u[0], u[-1] = 0.0, torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
        k, dist = oracle.select(m[0], u)
        keep = dist > 1e-6
        assert torch.equal(mog_ops.select_components(m[0], u)[keep], k[keep])
        got = mog_ops.sample_eager(m[0], m[1], m[3], zeta, u=u, shift=shift, scale=scale)
        assert row_parity(got[keep], oracle.sample(m[1], m[3], k, zeta, shift, scale)[keep])["exceed_frac"] == 0.0


def test_a_zero_weight_component_is_never_selected():
    logits = torch.tensor([[0.0, -float("inf"), 0.0, -float("inf")]])
    u = torch.cat([torch.linspace(0, 1, 101)[:-1], torch.tensor([0.5, torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))])])
    k = mog_ops.select_components(logits, u)
    assert set(k.tolist()) == {0, 2}


def test_exact_gaussians_give_the_analytic_posterior():
    """Linear-Gaussian model with exact Gaussians in fp64: prior N(m0, S0), x = theta + N(0, Sn), proposal N(mp, Sp).
    The exact proposal posterior q ~ likelihood x proposal has precision Pn + Pp; correcting it by the exact proposal
    and prior returns the analytic posterior, precision Pn + P0 and mean (Pn + P0)^-1 (Pn x + P0 m0).  The algebra is
    exact with eps = 0 (to 1e-10); sbi's eps = 1e-6 on the diagonal moves the answer by O(eps)."""
    torch.manual_seed(0)
    D = 3
    dt = torch.float64

    def spd(scale):
        A = torch.randn(D, D, dtype=dt)
        return scale * (A @ A.T / D + torch.eye(D, dtype=dt))

    S0, Sn, Sp = spd(0.5), spd(0.1), spd(0.08)
    m0, mp, x = torch.randn(D, dtype=dt) * 0.2, torch.randn(D, dtype=dt) * 0.3, torch.randn(D, dtype=dt) * 0.5
    P0, Pn, Pp = (torch.linalg.inv(S) for S in (S0, Sn, Sp))
    cov_q = torch.linalg.inv(Pn + Pp)
    q = MoG.from_gaussian(cov_q @ (Pn @ x + Pp @ mp), cov_q)
    prop, prior = MoG.from_gaussian(mp, Sp), MoG.from_gaussian(m0, S0)
    cov_true = torch.linalg.inv(Pn + P0)
    mean_true = cov_true @ (Pn @ x + P0 @ m0)
    logits, means, prec, fac, status = mog_ops.correct_eager(
        q.logits, q.means, q.precisions, prop.logits, prop.means, prop.precisions, prior.means[0, 0],
        prior.precisions[0, 0], eps=0.0)
    assert not status.any()
    assert (means[0, 0] - mean_true).abs().max() < 1e-10
    assert (torch.linalg.inv(prec[0, 0]) - cov_true).abs().max() < 1e-10
    assert (fac[0, 0].T @ fac[0, 0] - prec[0, 0]).abs().max() < 1e-10
    post = mog_ops.correct_for_proposal(q, prop, prior)                 # sbi's eps = 1e-6
    assert post.dtype == dt
    assert (post.means[0, 0] - mean_true).abs().max() < 1e-6
    assert (torch.linalg.inv(post.precisions[0, 0]) - cov_true).abs().max() < 1e-6


def test_not_positive_definite_is_sbis_value_error():
    d, p, _, _ = oracle.recipe(3, 4, 2, 5, 1, False)
    with pytest.raises(ValueError, match="Posterior precision matrix is not positive definite. This is a known issue "
                                         "with NPE-A"):
        mog_ops.correct_for_proposal(MoG(*p), MoG(d[0][:1], d[1][:1], d[2][:1]))      # (density and proposal swapped)
    out = mog_ops.correct_eager(p[0].expand(3, -1), p[1].expand(3, -1, -1), p[2].expand(3, -1, -1, -1), d[0][:1],
                                d[1][:1], d[2][:1])
    assert (out[4] == 1).all() and all(torch.isfinite(t).all() for t in out[:4])


# ------------------------------------------------------------------------------------------------ MoG
def test_mog_surface_and_validation_messages():
    eye = torch.eye(3).expand(2, 4, 3, 3)
    mog = MoG(torch.zeros(2, 4), torch.zeros(2, 4, 3), eye, eye)                    # positional, four arguments
    assert (mog.num_components, mog.dim, mog.batch_shape, mog.device.type, mog.dtype) == (
        4, 3, torch.Size([2]), "cpu", torch.float32)
    assert torch.allclose(mog.weights.sum(-1), torch.ones(2)) and torch.allclose(mog.log_weights.exp(), mog.weights)
    derived = MoG(torch.zeros(2, 4), torch.zeros(2, 4, 3), 4.0 * eye)              # factors from the Cholesky + 1e-6
    assert torch.allclose(derived.precision_factors, (4.0 + 1e-6) ** 0.5 * eye)
    assert torch.equal(derived.precision_factors, torch.triu(derived.precision_factors))
    assert derived.log_prob(torch.zeros(2, 3)).shape == (2,) and derived.log_prob(torch.zeros(5, 2, 3)).shape == (5, 2)
    assert derived.sample().shape == (2, 3) and derived.sample(torch.Size([7])).shape == (7, 2, 3)
    assert derived.sample((2, 3)).shape == (2, 3, 2, 3)
    moved = derived.to("cpu").detach()
    assert isinstance(moved, MoG) and torch.equal(moved.means, derived.means)
    g = MoG.from_gaussian(torch.tensor([1.0, -1.0]), torch.tensor([[2.0, 0.5], [0.5, 1.0]]))
    assert g.logits.shape == (1, 1) and g.means.shape == (1, 1, 2) and g.precisions.shape == (1, 1, 2, 2)
    assert torch.allclose(g.precision_factors[0, 0].T @ g.precision_factors[0, 0], g.precisions[0, 0], atol=1e-6)
    want = MultivariateNormal(torch.tensor([1.0, -1.0]), torch.tensor([[2.0, 0.5], [0.5, 1.0]]))
    pts = torch.randn(6, 1, 2)
    assert torch.allclose(g.log_prob(pts)[:, 0], want.log_prob(pts[:, 0]), atol=1e-5)
    for args, msg in (
            ((torch.zeros(4), torch.zeros(2, 4, 3), eye), "logits must be 2D"),
            ((torch.zeros(2, 4), torch.zeros(2, 4), eye), "means must be 3D"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), eye[0]), "precisions must be 4D"),
            ((torch.zeros(2, 4), torch.zeros(2, 5, 3), eye), "means shape .* incompatible with logits shape"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), torch.eye(3).expand(2, 5, 3, 3)), "precisions shape .* incompatible"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), torch.zeros(2, 4, 3, 2)), "precisions must be square matrices"),
            ((torch.full((2, 4), float("nan")), torch.zeros(2, 4, 3), eye), "logits contains NaN or Inf values"),
            ((torch.zeros(2, 4), torch.full((2, 4, 3), float("inf")), eye), "means contains NaN or Inf values"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), eye * float("nan")), "precisions contains NaN or Inf values"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), -eye), "Failed to compute Cholesky decomposition"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), eye, eye[:1]), "precision_factors shape .* must match"),
            ((torch.zeros(2, 4), torch.zeros(2, 4, 3), eye, eye * float("nan")), "precision_factors contains NaN")):
        with pytest.raises(ValueError, match=msg):
            MoG(*args)
    with pytest.raises(NotImplementedError, match="MoG.condition"):
        mog.condition(torch.zeros(2, 3), [0])


# ------------------------------------------------------------------------------------------------ the trainer
def _prior(D=2):
    return MultivariateNormal(torch.zeros(D), torch.eye(D))


def test_constructor_rules_and_messages():
    theta, x = torch.randn(50, 2), torch.randn(50, 3)
    assert SNPE_A is NPE_A
    assert NPE_A(_prior())._build_neural_net(theta, x).net.hyper.num_components == 10
    assert NPE_A(_prior(), num_components=3)._build_neural_net(theta, x).net.hyper.num_components == 3
    inf = NPE_A(_prior(), MDNConfig(hidden_features=12), num_components=4)
    net = inf._build_neural_net(theta, x)
    assert isinstance(net, MixtureDensityEstimator) and (net.net.hyper.num_components, net.net.hyper.hidden_features) == (4, 12)
    assert NPE_A(_prior(), MDNConfig(num_components=5), num_components=5)._build_neural_net(theta, x).net.hyper.num_components == 5
    with pytest.raises(ValueError, match=r"`num_components` was set both on the config \(5\) and on NPE_A \(7\). For "
                                         "NPE-A it belongs on the trainer."):
        NPE_A(_prior(), MDNConfig(num_components=5), num_components=7)
    with pytest.warns(FutureWarning, match="Passing a string for `density_estimator` is deprecated. Use MDNConfig"):
        inf = NPE_A(_prior(), "mdn_snpe_a", num_components=2)
    assert inf._build_neural_net(theta, x).net.hyper.num_components == 2
    for bad in ("mdn", "nsf", 3, 1.5):
        with pytest.raises(TypeError, match="needs to be a MDNConfig, a callable, or the string 'mdn_snpe_a'!"):
            NPE_A(_prior(), bad)
    seen = {}

    def builder(batch_theta, batch_x, num_components):
        seen["K"] = num_components
        return build_mdn(batch_theta, batch_x, num_components=num_components, hidden_features=8)

    assert isinstance(NPE_A(_prior(), builder, num_components=6)._build_neural_net(theta, x), MixtureDensityEstimator)
    assert seen["K"] == 6


def test_train_rules_and_round_bookkeeping(monkeypatch):
    inf = NPE_A(_prior(), num_components=2, show_progress_bars=False)
    with pytest.raises(RuntimeError, match="No simulations found. You must call .append_simulations"):
        inf.train()
    with pytest.raises(AssertionError, match="Retraining from scratch is not supported"):
        inf.train(retrain_from_scratch=True)
    proposal = MultivariateNormal(torch.zeros(2), 0.5 * torch.eye(2))
    sizes = (40, 50, 60)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # in particular: no "atomic loss will be used" warning
        inf.append_simulations(torch.randn(sizes[0], 2), torch.randn(sizes[0], 2))
        inf.append_simulations(torch.randn(sizes[1], 2), torch.randn(sizes[1], 2), proposal=proposal)
        inf.append_simulations(torch.full((sizes[2], 2), 7.0), torch.randn(sizes[2], 2), proposal=proposal)
    assert inf._data_round_index == [0, 1, 2]
    with pytest.warns(UserWarning, match="atomic"):        # (the NPE-C trainer still warns)
        NPE(_prior()).append_simulations(torch.randn(40, 2), torch.randn(40, 2), proposal=proposal)

    # what the shared loop is asked for
    seen = {}

    def fake_train(self, **kw):
        seen.update(kw)
        return "net"

    monkeypatch.setattr(PosteriorEstimatorTrainer, "train", fake_train)
    assert inf.train(max_num_epochs=3) == "net"
    assert seen["force_first_round_loss"] is True and seen["discard_prior_samples"] is True
    assert seen["max_num_epochs"] == 3 and inf._round == 2 and "num_atoms" not in seen
    monkeypatch.undo()

    # which rows the shared loop then takes: the latest round only
    class Stop(Exception):
        pass

    def spy(starting_round=0):
        seen["start"] = starting_round
        seen["rows"] = PosteriorEstimatorTrainer.get_simulations(inf, starting_round)[0]
        raise Stop

    monkeypatch.setattr(inf, "get_simulations", spy)
    with pytest.raises(Stop):
        inf.train()
    assert seen["start"] == 2 and seen["rows"].shape == (sizes[2], 2) and (seen["rows"] == 7.0).all()
    # unchanged for NPE-C: everything, or everything but the prior's round
    other = NPE(_prior())
    other._round = 2
    assert (other._get_start_index(False), other._get_start_index(True)) == (0, 1)
    other._round = 0
    assert other._get_start_index(True) == 0


class _Stub:
    def __init__(self, mog, default_x):
        self._mog, self.default_x = mog, default_x

    def get_mog_params(self, x):
        return self._mog


def test_the_four_proposal_cases_and_their_messages():
    inf = NPE_A(_prior(), num_components=2)
    mog = MoG.from_gaussian(torch.zeros(2), torch.eye(2))
    # 1: an NPE_A_Posterior
    est = build_mdn(torch.randn(50, 2), torch.randn(50, 3), num_components=2, hidden_features=8)
    post = NPE_A_Posterior(est, _prior(), proposal_mog=mog)
    with pytest.raises(ValueError, match="Proposal posterior must have a default_x set for NPE-A correction"):
        inf._get_proposal_mog(post)
    post.set_default_x(torch.zeros(2, 3))
    with pytest.raises(ValueError, match="NPE-A requires default_x batch size of 1, got 2. NPE-A only supports single"):
        inf._get_proposal_mog(post)
    post.set_default_x(torch.zeros(1, 3))
    post._get_corrected_mog = lambda x: mog
    assert inf._get_proposal_mog(post) is mog
    # 2: a MultivariateNormal
    got = inf._get_proposal_mog(MultivariateNormal(torch.tensor([1.0, 2.0]), 0.25 * torch.eye(2)))
    assert got.num_components == 1 and torch.allclose(got.means[0, 0], torch.tensor([1.0, 2.0]))
    assert torch.allclose(got.precisions[0, 0], 4.0 * torch.eye(2))
    # 3: a MoG
    assert torch.equal(inf._get_proposal_mog(mog).means, mog.means)
    # 4: anything with get_mog_params
    assert torch.equal(inf._get_proposal_mog(_Stub(mog, torch.zeros(1, 3))).means, mog.means)
    with pytest.raises(ValueError, match=r"Proposal has get_mog_params\(\) but no default_x set"):
        inf._get_proposal_mog(_Stub(mog, None))
    with pytest.raises(ValueError, match="NPE-A requires default_x batch size of 1, got 3."):
        inf._get_proposal_mog(_Stub(mog, torch.zeros(3, 3)))
    with pytest.raises(TypeError, match=r"Proposal's get_mog_params\(\) must return MoG, got Tensor."):
        inf._get_proposal_mog(_Stub(torch.zeros(1), torch.zeros(1, 3)))
    with pytest.raises(TypeError, match="For multi-round NPE-A, proposal must be one of: NPE_A_Posterior, "
                                        "MultivariateNormal, MoG, or an object with get_mog_params.. method. Got "
                                        "BoxUniform."):
        inf._get_proposal_mog(BoxUniform(-torch.ones(2), torch.ones(2)))


def test_z_scored_prior_mog_against_a_hand_computation():
    mean, cov = torch.tensor([0.5, -1.0]), torch.tensor([[2.0, 0.3], [0.3, 0.5]])
    theta = torch.randn(200, 2) * torch.tensor([3.0, 0.2]) + torch.tensor([1.0, -2.0])
    est = build_mdn(theta, torch.randn(200, 3), num_components=2, hidden_features=8)
    shift, scale = est.net.zstats[:2], est.net.zstats[2:4]
    assert torch.allclose(shift, theta.mean(0), atol=1e-5) and (scale - theta.std(0)).abs().max() < 0.05
    got = NPE_A(MultivariateNormal(mean, cov))._compute_z_scored_prior_mog(est)
    z_cov = torch.tensor([[cov[0, 0] / scale[0] ** 2, cov[0, 1] / (scale[0] * scale[1])],
                          [cov[1, 0] / (scale[0] * scale[1]), cov[1, 1] / scale[1] ** 2]])
    assert got.num_components == 1 and torch.allclose(got.means[0, 0], (mean - shift) / scale, atol=1e-6)
    assert torch.allclose(got.precisions[0, 0], torch.linalg.inv(z_cov), rtol=1e-4, atol=1e-5)
    plain = build_mdn(theta, torch.randn(200, 3), num_components=2, hidden_features=8, z_score_x="none")
    got = NPE_A(MultivariateNormal(mean, cov))._compute_z_scored_prior_mog(plain)
    assert torch.allclose(got.means[0, 0], mean) and torch.allclose(got.precisions[0, 0], torch.linalg.inv(cov), atol=1e-5)
    assert NPE_A(BoxUniform(-torch.ones(2), torch.ones(2)))._compute_z_scored_prior_mog(est) is None
    with pytest.raises(TypeError, match="Prior must be MultivariateNormal or BoxUniform, got Independent"):
        NPE_A(torch.distributions.Independent(torch.distributions.Normal(torch.zeros(2), 1.0), 1)
              )._compute_z_scored_prior_mog(est)


def test_build_posterior_rules():
    inf = NPE_A(_prior(), num_components=2)
    with pytest.raises(ValueError, match="NPE_A only supports sample_with='direct', got 'mcmc'. The corrected "
                                         "posterior is a Mixture of Gaussians"):
        inf.build_posterior(sample_with="mcmc")
    theta, x = torch.randn(60, 2), torch.randn(60, 3)
    est = build_mdn(theta, x, num_components=2, hidden_features=8)
    inf.append_simulations(theta, x)
    first = inf.build_posterior(est)
    assert isinstance(first, NPE_A_Posterior) and not first._apply_correction and first._proposal_mog is None
    inf.append_simulations(theta, x, proposal=MultivariateNormal(torch.zeros(2), 0.5 * torch.eye(2)))
    second = inf.build_posterior(est)
    assert second._apply_correction and second._proposal_mog.num_components == 1 and second._prior_mog is not None
    with pytest.raises(TypeError, match="NPE_A requires MixtureDensityEstimator, got Linear"):
        inf.build_posterior(torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="map"):
        second.map()


# ------------------------------------------------------------------------------------------------ the posterior
def _stubbed_posterior(prior, D=2, K=3, L=2, rows_seed=0):
    """An NPE_A_Posterior whose network mixture is a fixed function of x (the MDN itself needs the device)."""
    theta = torch.randn(100, D) * 0.5 + 0.2
    est = build_mdn(theta, torch.randn(100, 3), num_components=K, hidden_features=8)
    g = torch.Generator().manual_seed(rows_seed)
    p = oracle.mixture(g, 1, L, D, 0.5, 1.0, 0.5)
    bank = oracle.mixture(g, 64, K, D, 2.0, 4.0, 0.5)

    def get_uncorrected_mog(x):
        idx = (x.reshape(x.shape[0], -1).sum(-1).abs() * 1000).long() % 64       # the mixture depends on the row of x
        return MoG(*(t[idx] for t in bank))

    est.get_uncorrected_mog = get_uncorrected_mog
    return NPE_A_Posterior(est, prior, proposal_mog=MoG(*p)), est, bank, p


def test_posterior_applies_the_correction_and_the_prior_support():
    prior = BoxUniform(-2.0 * torch.ones(2), 2.0 * torch.ones(2))
    post, est, bank, p = _stubbed_posterior(prior)
    xs = torch.randn(3, 3)
    shift, scale = est.net.zstats[:2], est.net.zstats[2:4]
    mog = post.get_mog_params(xs)
    assert mog.num_components == 6 and mog.logits.shape == (3, 6)
    theta = torch.rand(5, 3, 2) - 0.5
    batched = post.log_prob_batched(theta, xs, norm_posterior=False)
    assert batched.shape == (5, 3) and torch.isfinite(batched).all()
    for b in range(3):
        single = post.log_prob(theta[:, b], x=xs[b : b + 1], norm_posterior=False)
        assert row_parity(batched[:, b], single)["exceed_frac"] == 0.0
        ref = oracle.log_prob(mog.logits[b : b + 1], mog.means[b : b + 1], mog.precisions[b : b + 1],
                              mog.precision_factors[b : b + 1], theta[:, b], shift, scale)
        assert row_parity(single, ref)["exceed_frac"] == 0.0
    outside = post.log_prob(torch.tensor([[3.0, 0.0], [0.1, 0.1]]), x=xs[:1], norm_posterior=False)
    assert outside[0] == -float("inf") and torch.isfinite(outside[1])
    normed = post.log_prob(torch.tensor([[0.1, 0.1]]), x=xs[:1])
    assert torch.isfinite(normed).all() and (normed >= outside[1] - 1e-6).all()       # divided by an acceptance rate <= 1
    torch.manual_seed(0)
    draws = post.sample((500,), x=xs[:1], show_progress_bars=False)
    assert draws.shape == (500, 2) and (draws.abs() <= 2).all()
    many = post.sample_batched((4,), xs, show_progress_bars=False)
    assert many.shape == (4, 3, 2)
    # the draws follow the corrected mixture of their own observation, not the network's
    big = post.sample_batched((4000,), xs, show_progress_bars=False, reject_outside_prior=False)
    w = torch.softmax(mog.logits, -1)
    want = ((w[..., None] * mog.means).sum(1)) * scale + shift
    assert (big.mean(0) - want).abs().max() < 0.08
    with pytest.raises(ValueError, match="batchsize == 1"):
        post.sample((2,), x=xs, show_progress_bars=False)
    with pytest.raises(ValueError, match="batchsize == 1"):
        post.log_prob(theta[:, 0], x=xs)
    with pytest.raises(NotImplementedError, match="map"):
        post.map(x=xs[:1])
