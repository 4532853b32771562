"""Conditional posterior analysis on the host route: sbi_amd.analysis / sbi_amd.utils.conditional_density_utils against
the reference's recorded outputs (tests/golden/conditional_reference.pt, tools/make_golden_conditional.py) and the fp64
restatement tests/cond_oracle.py.

Bounds: the project's row bound |d| <= 1e-5 (1 + |ref|) against the reference's fp32 correlation coefficient (over 200
random cases of the recorded family the reference alone stays within 2.6e-6 of fp64: 4x margin), 1e-6 against fp64.

The slice sampler has no host path (tests/test_mcmc_cpu.py pins its refusal), so the statistical check of conditional
MCMC lives in tests/test_conditional_gpu.py; here the three objects are driven through the same host-side pieces
`MCMCPosterior` composes them with (`unconstrained_potential`, `proposal_init`)."""

import math
import os

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd import analysis
from sbi_amd.analysis import (ConditionedMDN, conditional_corrcoeff, conditional_density_grids, conditional_potential,
                              eval_conditional_density)
from sbi_amd.utils import conditional_density_utils as cdu
from sbi_amd.utils.conditional_density_utils import (ConditionedPotential, RestrictedPriorForConditional,
                                                     RestrictedTransformForConditional, compute_corrcoeff,
                                                     condition_mog, extract_and_transform_mog)
from tests import cond_oracle, parity_log

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conditional_reference.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


class Gaussian:
    """The density the golden was recorded with (tools/make_golden_conditional.py): element-wise fp32 in a fixed order,
    hence bit-identical log-probs on any machine."""

    def __init__(self, mean, prec, const):
        self.mean, self.prec, self.const = mean, prec, const

    def log_prob(self, theta):
        d = theta - self.mean
        q = torch.zeros_like(d[:, 0])
        for a in range(d.shape[1]):
            for b in range(d.shape[1]):
                q = q + self.prec[a, b] * d[:, a] * d[:, b]
        return self.const - 0.5 * q


def row_bound(ref):
    return 1e-5 * (1.0 + abs(float(ref)))


def test_probs_and_raw_log_probs_equal_the_reference(golden):
    g4 = golden["gaussian4"]
    dens = Gaussian(g4["mean"], g4["prec"], g4["const"])
    for e in g4["grids"]:
        args = (dens, g4["conditions"][:1], g4["limits"], e["dim1"], e["dim2"])
        probs = eval_conditional_density(*args, resolution=e["R"])
        raw = eval_conditional_density(*args, resolution=e["R"], return_raw_log_prob=True)
        assert probs.shape == e["probs"].shape == ((e["R"],) if e["dim1"] == e["dim2"] else (e["R"], e["R"]))
        assert raw.shape == e["raw"].shape
        torch.testing.assert_close(raw, e["raw"], rtol=1e-6, atol=0.0)
        torch.testing.assert_close(probs, e["probs"], rtol=1e-6, atol=0.0)
        assert float(probs.max()) == 1.0


def test_rho_within_the_row_bound_of_the_reference_and_1e6_of_fp64(golden):
    cases = [(e["probs"], golden["gaussian4"]["limits"][[e["dim1"], e["dim2"]]], e) for e in golden["gaussian4"]["grids"]
             if e["dim1"] != e["dim2"]]
    cases += [(e["probs"], golden["family"]["limits"], e) for e in golden["family"]["cases"]]
    assert {e["R"] for _, _, e in cases} == {20, 50} and len(cases) >= 12
    worst_ref = worst_64 = 0.0
    for probs, lim, e in cases:
        rho = compute_corrcoeff(probs, lim)
        assert rho.shape == () and rho.dtype == probs.dtype
        d_ref, d_64 = abs(float(rho) - float(e["rho_ref"])), abs(float(rho) - e["rho_fp64"])
        worst_ref, worst_64 = max(worst_ref, d_ref / row_bound(e["rho_ref"])), max(worst_64, d_64)
        print(f"R={e['R']} rho={float(rho):+.7f} |d ref|={d_ref:.2e} |d fp64|={d_64:.2e}")
        assert d_ref <= row_bound(e["rho_ref"])
        assert d_64 <= 1e-6
    parity_log.record("conditional_host_rho", "golden", worst_over_row_bound=worst_ref, worst_vs_fp64=worst_64)


def test_correlation_matrix_golden_symmetry_subset_and_averaging(golden):
    g4, gc = golden["gaussian4"], golden["corrcoeff"]
    dens = Gaussian(g4["mean"], g4["prec"], g4["const"])
    full = conditional_corrcoeff(dens, g4["limits"], g4["conditions"], resolution=50)
    assert full.shape == (4, 4) and full.dtype == torch.float32
    assert torch.equal(full, full.T) and torch.equal(torch.diagonal(full), torch.ones(4))
    assert ((full - gc["full"]).abs() <= 1e-5 * (1 + gc["full"].abs())).all()
    sub = conditional_corrcoeff(dens, g4["limits"], g4["conditions"], subset=gc["subset"], resolution=50)
    assert sub.shape == (3, 3)
    assert ((sub - gc["sub"]).abs() <= 1e-5 * (1 + gc["sub"].abs())).all()
    assert torch.equal(sub, full[gc["subset"]][:, gc["subset"]])
    # a non-sorted subset: entry (a, b) is the coefficient of (subset[a], subset[b])
    unsorted = [2, 0, 3]
    got = conditional_corrcoeff(dens, g4["limits"], g4["conditions"], subset=unsorted, resolution=50)
    assert torch.equal(got, full[unsorted][:, unsorted])
    # the mean over the conditions (taken in fp64 here, in fp32 by the reference)
    singles = torch.stack([conditional_corrcoeff(dens, g4["limits"], c[None], resolution=50) for c in g4["conditions"]])
    torch.testing.assert_close(full, singles.double().mean(0).float(), rtol=0, atol=1.2e-7)
    assert (singles[0] - singles[1]).abs().max() > 1e-4          # the conditions do differ
    # one dimension: nothing to correlate
    assert torch.equal(conditional_corrcoeff(dens, g4["limits"], g4["conditions"], subset=[1]), torch.ones(1, 1))


@pytest.mark.parametrize("shift", [0.0, 100.0, 1000.0])
def test_host_formula_survives_shifted_limits(golden, shift):
    """The reference loses 2.5e-2 at +100 and returns inf around 1000; the centred fp64 sums do not care."""
    fam = golden["family"]
    lim = fam["limits"] + shift
    worst = 0.0
    for e in fam["cases"]:
        R = e["R"]
        axes = torch.stack([torch.linspace(float(lim[d, 0]), float(lim[d, 1]), R) for d in range(2)])
        logp = torch.log(e["probs"]).reshape(1, R * R)
        want = cond_oracle.grid_moments(logp, axes, [(0, 1)])[0][0]
        got = compute_corrcoeff(torch.exp(logp - logp.max()).reshape(R, R), lim)
        worst = max(worst, abs(float(got) - float(want)))
        assert abs(float(got) - float(want)) <= 1e-6
        if shift == 0.0:
            assert abs(float(got) - e["rho_fp64"]) <= 1e-6
    print(f"shift {shift}: worst |host - oracle| = {worst:.2e}")
    parity_log.record("conditional_host_shifted", f"shift{int(shift)}", worst_abs=worst)


def test_degenerate_grids_give_nan_not_inf():
    lim = torch.tensor([[-2.0, 2.0], [-1.0, 3.0]])
    one_cell = torch.zeros(5, 5)
    one_cell[2, 3] = 1.0
    with_nan = torch.rand(5, 5)
    with_nan[0, 0] = float("nan")
    for p in (one_cell, with_nan, torch.zeros(5, 5), torch.full((5, 5), float("inf"))):
        assert torch.isnan(compute_corrcoeff(p, lim))
    assert torch.isfinite(compute_corrcoeff(torch.rand(5, 5), lim))


def test_density_grids_match_the_single_calls(golden):
    g4 = golden["gaussian4"]
    dens = Gaussian(g4["mean"], g4["prec"], g4["const"])
    diag, off, pairs = conditional_density_grids(dens, g4["conditions"][:1], g4["limits"], subset=[3, 0, 1],
                                                 resolution=20)
    assert diag.shape == (3, 20) and off.shape == (3, 20, 20) and pairs == [(0, 3), (0, 1), (1, 3)]
    for a, d in enumerate([3, 0, 1]):
        assert torch.equal(diag[a], eval_conditional_density(dens, g4["conditions"][:1], g4["limits"], d, d, 20))
    for q, (d1, d2) in enumerate(pairs):
        assert d1 < d2
        assert torch.equal(off[q], eval_conditional_density(dens, g4["conditions"][:1], g4["limits"], d1, d2, 20))
    with pytest.raises(ValueError, match="batch size > 1"):
        conditional_density_grids(dens, g4["conditions"], g4["limits"])


# ---------------------------------------------------------------------------------------------------- mixtures
def test_condition_mog_agrees_with_the_reference(golden):
    """The reference evaluates in fp32 (matrix products and one 2 x 2 solve per component, precisions of condition
    number < 1e3 here): 1e-4 relative / 1e-5 absolute covers its rounding; the fp64 result is cast back to fp32."""
    cm = golden["condition_mog"]
    logits, means, precfs, sumlogdiag = condition_mog(cm["condition"], cm["dims"], cm["logits"], cm["means"],
                                                      cm["precfs"])
    assert logits.shape == (1, 3) and means.shape == (1, 3, 2) and precfs.shape == (1, 3, 2, 2)
    assert means.dtype == torch.float32
    torch.testing.assert_close(logits, cm["out_logits"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(means, cm["out_means"], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(precfs, cm["out_precfs"], rtol=1e-6, atol=0)
    torch.testing.assert_close(sumlogdiag, cm["out_sumlogdiag"], rtol=1e-4, atol=1e-5)
    assert abs(float(torch.logsumexp(logits, -1))) < 1e-6
    with pytest.raises(ValueError, match="batch size > 1"):
        condition_mog(cm["condition"].repeat(2, 1), cm["dims"], cm["logits"], cm["means"], cm["precfs"])


class _OneGaussianMDN:
    """The surface `extract_and_transform_mog` reads, backed by a fixed K = 1 mixture in z-scored space."""

    def __init__(self, mean_z, prec_z, shift=None, scale=None):
        from sbi_amd.neural_nets.estimators.mdn import MoG

        U = torch.linalg.cholesky(prec_z).T
        self._mog = MoG(logits=torch.zeros(1, 1), means=mean_z.reshape(1, 1, -1), precisions=prec_z[None, None],
                        precision_factors=U[None, None].contiguous())
        self.has_input_transform = shift is not None
        self._transform_shift, self._transform_scale = shift, scale
        self.seen = None

    def get_uncorrected_mog(self, context):
        self.seen = context
        return self._mog


def test_conditioned_mdn_is_the_analytic_conditional_and_mog_condition_still_raises():
    from sbi_amd.neural_nets.estimators.mdn import MoG

    torch.manual_seed(3)
    A = torch.randn(3, 3, dtype=torch.float64)
    cov_z = (A @ A.T + 0.5 * torch.eye(3, dtype=torch.float64))
    shift, scale = torch.tensor([0.5, -1.0, 2.0]), torch.tensor([2.0, 0.5, 1.5])
    mean_z = torch.tensor([0.3, -0.2, 0.1])
    mdn = _OneGaussianMDN(mean_z, torch.linalg.inv(cov_z).float(), shift, scale)
    x_o = torch.zeros(1, 2)
    condition = torch.tensor([[9.0, 9.0, 2.6]])          # the entries at the free dimensions are ignored
    cmdn = ConditionedMDN(mdn, x_o, condition, dims_to_sample=[0, 1])
    assert mdn.seen is x_o
    # theta = z * scale + shift: mean and covariance in theta space, then the textbook Gaussian conditional
    mu = (mean_z * scale + shift).double()
    cov = cov_z * torch.outer(scale, scale).double()
    k = cov[:2, 2:] @ torch.linalg.inv(cov[2:, 2:])
    want = MultivariateNormal(mu[:2] + (k @ (condition[0, 2:].double() - mu[2:])), cov[:2, :2] - k @ cov[2:, :2])
    theta = want.sample((64,)).float()
    got = cmdn.log_prob(theta)
    assert got.shape == (64,)
    torch.testing.assert_close(got.double(), want.log_prob(theta.double()), rtol=0, atol=2e-4)
    assert cmdn.log_prob(theta[0]).shape == (1,)
    draws = cmdn.sample((4000,))
    assert draws.shape == (4000, 2)
    # 4000 independent draws: 5 standard errors of the mean
    se = want.covariance_matrix.diagonal().sqrt() / math.sqrt(4000)
    assert ((draws.double().mean(0) - want.mean).abs() <= 5 * se).all()
    logits, means, precfs, sld = extract_and_transform_mog(mdn, x_o)
    assert logits.shape == (1, 1) and means.shape == (1, 1, 3) and precfs.shape == (1, 1, 3, 3) and sld.shape == (1, 1)
    with pytest.raises(ValueError, match="context must be provided"):
        extract_and_transform_mog(mdn)
    with pytest.raises(NotImplementedError):
        MoG(logits=torch.zeros(1, 1), means=torch.zeros(1, 1, 2), precisions=torch.eye(2)[None, None]).condition(
            condition, [0])


# ---------------------------------------------------------------------------------------------------- potentials
class _GaussPotential:
    """A potential with the package's potential surface: log N(theta; mean, cov), x_o only stored."""

    def __init__(self, mean, cov, device="cpu"):
        self.device = device
        self.d = MultivariateNormal(mean.to(device), cov.to(device))
        self._x_o = None
        self.calls = []

    def set_x(self, x_o, x_is_iid=False):
        self._x_o = x_o
        self.calls.append((x_o, x_is_iid))

    def __call__(self, theta, track_gradients=True):
        self.last_theta = theta
        with torch.set_grad_enabled(track_gradients):
            return self.d.log_prob(theta)


def test_conditioned_potential_prior_and_transform():
    from sbi_amd.inference.posteriors.mcmc_posterior import unconstrained_potential
    from sbi_amd.samplers.mcmc import proposal_init
    from sbi_amd.utils.sbiutils import mcmc_transform
    from sbi_amd.utils.torchutils import BoxUniform

    mean, cov = torch.tensor([0.1, 0.4, -0.2]), torch.tensor([[1.0, 0.5, 0.2], [0.5, 1.5, -0.3], [0.2, -0.3, 0.8]])
    pot = _GaussPotential(mean, cov)
    prior = BoxUniform(-3 * torch.ones(3), 3 * torch.ones(3))
    tf = mcmc_transform(prior)
    condition = torch.tensor([0.3, -0.7, 1.1])
    dims = [2, 0]
    cpot, rtf, rprior = conditional_potential(pot, tf, prior, condition, dims)
    assert isinstance(cpot, ConditionedPotential) and isinstance(rtf, RestrictedTransformForConditional)
    assert isinstance(rprior, RestrictedPriorForConditional)
    assert cpot.device == "cpu" and cpot.condition.shape == (1, 3)
    theta = torch.tensor([[0.5, -0.5], [1.0, 2.0], [-1.0, 0.0], [0.2, 0.3], [2.5, -2.5]])
    out = cpot(theta, track_gradients=False)
    full = condition.repeat(5, 1)
    full[:, dims] = theta
    assert out.shape == (5,) and torch.equal(pot.last_theta, full) and torch.equal(out, pot.d.log_prob(full))
    assert cpot(theta[0]).shape == (1,)                       # an unbatched theta is batched
    with pytest.raises(ValueError, match="Condition with batch size > 1 not supported."):
        ConditionedPotential(pot, torch.zeros(2, 3), dims)
    # x_o handling is forwarded
    with pytest.raises(ValueError, match="No observed data is available"):
        cpot.x_is_iid
    with pytest.raises(ValueError, match="No observed data is available."):
        cpot.x_o
    assert cpot.return_x_o() is None
    x = torch.tensor([[1.0, 2.0]])
    cpot.set_x(x, x_is_iid=False)
    assert torch.equal(pot.calls[-1][0], x) and pot.calls[-1][1] is False and cpot.x_is_iid is False
    assert torch.equal(cpot.x_o, x) and torch.equal(cpot.return_x_o(), x)
    cpot.x_o = 2 * x
    assert torch.equal(pot._x_o, 2 * x) and cpot.x_is_iid is True
    # the restricted prior: free dimensions out, the full prior's log_prob in
    torch.manual_seed(5)
    s = rprior.sample((7,))
    torch.manual_seed(5)
    assert s.shape == (7, 2) and torch.equal(s, prior.sample((7,))[:, dims])
    assert torch.equal(rprior.log_prob(full), prior.log_prob(full))
    # the restricted transform: free dimensions through the full transform, the Jacobian over ALL dimensions
    u = rtf(theta)
    assert u.shape == (5, 2) and torch.equal(u, tf(full)[:, dims])
    back = rtf.inv(u)
    torch.testing.assert_close(back, theta, rtol=1e-5, atol=1e-6)
    full_u = condition.repeat(5, 1)
    full_u[:, dims] = u
    lad = rtf.log_abs_det_jacobian(theta, u)
    assert lad.shape == (5,) and torch.equal(lad, tf.log_abs_det_jacobian(full, full_u))
    per_dim = -tf.inv.base_transform.log_abs_det_jacobian(full_u, full)      # (5, 3): each dimension's share
    torch.testing.assert_close(lad, per_dim.sum(-1), rtol=1e-5, atol=1e-6)
    assert not torch.allclose(lad, per_dim[:, dims].sum(-1), atol=1e-3)       # not the free dimensions' share alone
    # the pieces MCMCPosterior composes: chains start in transformed space, the walk evaluates the constrained point
    init = proposal_init(rprior, transform=rtf, num_chains=6)
    assert init.shape == (6, 2)
    walk = unconstrained_potential(cpot, rtf, "cpu")
    got = walk(u)
    torch.testing.assert_close(got, pot.d.log_prob(full) - lad, rtol=1e-5, atol=1e-5)
    # gradients flow to the free parameters on the eager route
    th = theta.clone().requires_grad_(True)
    cpot(th, track_gradients=True).sum().backward()
    assert th.grad is not None and th.grad.shape == (5, 2) and bool((th.grad != 0).all())


def test_every_declared_cond_symbol_is_exported_and_bound():
    import ctypes
    import re

    from sbi_amd import _build, _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sbi_amd_cond.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sbi_amd_\w+)\s*\(", text)))
    assert declared == ["sbi_amd_cond_expand", "sbi_amd_cond_grid_fill", "sbi_amd_cond_grid_moments"]
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    for s in declared:
        assert hasattr(lib, s), f"{s} declared in include/sbi_amd_cond.h but not exported"
    assert set(declared) == set(_lib.exported_symbols_cond()), "ctypes binding and header disagree"
    assert not set(declared) & set(_lib.exported_symbols())
    # refusals are host-side answers: nothing is launched, no device is needed
    loaded = _lib.load()
    assert loaded.sbi_amd_cond_grid_fill(None, None, None, 3, 4, 1, 2, 0, 1, None, None) == _lib.E_BADARG
    assert loaded.sbi_amd_cond_grid_moments(None, None, None, 3, 4, 1, 0, 1, None, None, None, None) == _lib.E_BADARG
    assert loaded.sbi_amd_cond_expand(None, None, None, 1, 3, 1, None, None) == _lib.E_BADARG


def test_routes_and_envelope_are_host_side_decisions():
    assert cdu.in_envelope(64, 1024) and not cdu.in_envelope(65, 50) and not cdu.in_envelope(10, 1025)
    assert analysis.conditional_density.force_loop is False
    with pytest.raises(RuntimeError, match="bad argument"):
        cdu._check_pairs([(1, 1)], 3, 2)
    with pytest.raises(RuntimeError, match="bad argument"):
        cdu._check_pairs([(0, 1)], 3, 1)
    with pytest.raises(RuntimeError, match="bad argument"):
        cdu._check_pairs([(0, 3)], 3, 2)
    cdu._check_pairs([(2, 0), (0, 1)], 3, 2)
