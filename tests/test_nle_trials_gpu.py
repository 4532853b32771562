"""sbi_amd_nsf_log_prob_trials: NLE's log-likelihood over iid trials, sum_i log q(x_i | theta_c) per theta, without
materialising the (trial, theta) pairs (the reference expands x_o, likelihood_based_potential.py:186-236).  Held to
(i) the fp64 oracle sum, (ii) sbi_amd_nsf_log_prob on the materialised theta-major pairs, bit for bit per row,
(iii) determinism: repeated calls and theta permutations.  Shapes reach both kernel families (cooperative at <= 12 288
rows, throughput above)."""
import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.nsf_flow import _log_prob_call, log_prob_trials_call
from tests.helpers import make_inputs, matched_pair

pytestmark = pytest.mark.gpu

# (flow input = x-dim, condition = theta-dim): the estimator of NLE models q(x | theta)
CONFIGS = [
    dict(D=10, C=10),
    dict(D=7, C=3, hidden_features=32, num_bins=8, num_transforms=3),
    dict(D=1, C=3),                                   # x-dim 1: the context spline map of a scalar summary statistic
]
TRIALS = [1, 3, 16, 17, 100]
THETAS = [1, 20, 10_000]
ORACLE_THETAS = 160          # theta rows of a 10 000-theta call held to the fp64 oracle (all rows: bit-exact paired)


def _ids(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@pytest.fixture(scope="module", params=CONFIGS, ids=_ids)
def pair(request):
    kw = dict(request.param)
    D, C = kw.pop("D"), kw.pop("C")
    oracle, est, _, _ = matched_pair(D=D, C=C, **kw)
    return oracle.to("cuda").double(), est, D, C


def _data(num_trials, num_theta, D, C):
    inp, cond = make_inputs(max(num_trials, num_theta), D, C, seed=7 + num_trials)
    return inp[:num_trials].cuda().contiguous(), cond[:num_theta].cuda().contiguous()


@pytest.mark.parametrize("num_theta", THETAS)
@pytest.mark.parametrize("num_trials", TRIALS)
def test_trials_sum_matches_oracle_and_paired_rows(pair, num_trials, num_theta):
    oracle, est, D, C = pair
    x_trials, theta = _data(num_trials, num_theta, D, C)
    loglik, rows = log_prob_trials_call(est.net, x_trials, theta, want_rows=True)
    torch.cuda.synchronize()
    n = num_trials * num_theta
    assert loglik.shape == (num_theta,) and rows.shape == (n,)

    # (ii) the materialised theta-major pairs through sbi_amd_nsf_log_prob: row c * num_trials + i = (x_i, theta_c)
    x_mat = x_trials.repeat(num_theta, 1).contiguous()
    th_mat = theta.repeat_interleave(num_trials, dim=0).contiguous()
    paired, _ = _log_prob_call(est.net, x_mat, th_mat, False)
    assert torch.equal(rows, paired), f"per-row values differ from the paired call ({(rows != paired).sum()} rows)"

    # (i) the fp64 oracle, summed over the trials in fp64
    sel = torch.arange(num_theta, device="cuda")
    if num_theta > ORACLE_THETAS:
        sel = torch.randperm(num_theta, generator=torch.Generator().manual_seed(num_trials))[:ORACLE_THETAS].cuda()
    with torch.no_grad():
        xs = x_trials.double().repeat(sel.numel(), 1)
        ts = theta[sel].double().repeat_interleave(num_trials, dim=0)
        ref_rows = oracle.log_prob(xs, ts)[0].reshape(sel.numel(), num_trials)
    ref = ref_rows.sum(1)
    tol = 4e-5 * (1.0 + ref_rows.abs()).sum(1)
    err = (loglik[sel].double() - ref).abs()
    assert bool((err <= tol).all()), f"max err {float(err.max()):.3e}, tol {float(tol.min()):.3e}"


@pytest.mark.parametrize("num_trials,num_theta", [(3, 20), (17, 20), (100, 10_000), (1, 10_000)])
def test_trials_sum_is_deterministic_and_permutation_equivariant(pair, num_trials, num_theta):
    _, est, D, C = pair
    x_trials, theta = _data(num_trials, num_theta, D, C)
    a, _ = log_prob_trials_call(est.net, x_trials, theta)
    b, _ = log_prob_trials_call(est.net, x_trials, theta)
    assert torch.equal(a, b)
    perm = torch.randperm(num_theta, generator=torch.Generator().manual_seed(5)).cuda()
    c, _ = log_prob_trials_call(est.net, x_trials, theta[perm].contiguous())
    assert torch.equal(c, a[perm])


def test_both_kernel_families_are_reached():
    _, est, _, _ = matched_pair(D=10, C=10)
    lib = _lib.load()
    cfg = est.net.hyper.c_config()
    kinds = {lib.sbi_amd_nsf_image_kind(cfg, t * m, 0) for t in TRIALS for m in THETAS}
    assert kinds == {0, 1}


def test_wide_config_is_refused_and_the_potential_falls_back():
    from sbi_amd.inference.potentials.likelihood_based_potential import (LikelihoodBasedPotential,
                                                                         log_likelihoods_over_trials_generic)
    from sbi_amd.utils.torchutils import BoxUniform

    D, C = 5, 4
    _, est, _, _ = matched_pair(D=D, C=C, hidden_features=100)
    lib = _lib.load()
    cfg = est.net.hyper.c_config()
    assert lib.sbi_amd_nsf_log_prob_trials_workspace_floats(cfg, 5, 20) == _lib.E_UNSUPPORTED
    x_trials, theta = _data(5, 20, D, C)
    out = torch.empty(20, device="cuda")
    rc = lib.sbi_amd_nsf_log_prob_trials(cfg, None, None, _lib.ptr(x_trials), 5, _lib.ptr(theta), 20, _lib.ptr(out),
                                         None, None, None)
    assert rc == _lib.E_UNSUPPORTED
    assert log_prob_trials_call(est.net, x_trials, theta) is None
    assert est.log_prob_iid_trials(x_trials, theta) is None
    prior = BoxUniform(-3 * torch.ones(C, device="cuda"), 3 * torch.ones(C, device="cuda"))
    pot = LikelihoodBasedPotential(est, prior, x_trials, device="cuda")
    got = pot(theta, track_gradients=False)
    with torch.no_grad():
        ref = log_likelihoods_over_trials_generic(x_trials, theta, est) + prior.log_prob(theta)
    assert torch.equal(got, ref)


def test_bad_arguments_are_refused():
    D, C = 4, 3
    _, est, _, _ = matched_pair(D=D, C=C, hidden_features=32, num_transforms=2)
    lib = _lib.load()
    cfg = est.net.hyper.c_config()
    x_trials, theta = _data(4, 8, D, C)
    out = torch.empty(8, device="cuda")
    P = _lib.ptr
    assert lib.sbi_amd_nsf_log_prob_trials_workspace_floats(cfg, 0, 8) == _lib.E_BADARG
    assert lib.sbi_amd_nsf_log_prob_trials_workspace_floats(cfg, 4, 8) == 32
    # no workspace and no per-row output: nowhere to put the rows
    from sbi_amd.neural_nets.estimators.nsf_flow import packed_weights

    packed = packed_weights(est.net, rows=32)
    assert lib.sbi_amd_nsf_log_prob_trials(cfg, P(packed), P(est.net.zstats), P(x_trials), 4, P(theta), 8, P(out),
                                           None, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_nsf_log_prob_trials(cfg, P(packed), P(est.net.zstats), P(x_trials), 0, P(theta), 8, P(out),
                                           P(out), None, None) == _lib.E_BADARG
    assert lib.sbi_amd_nsf_log_prob_trials(cfg, P(packed), P(est.net.zstats), P(x_trials), 4, P(theta), 0, P(out),
                                           None, None, None) == 0
