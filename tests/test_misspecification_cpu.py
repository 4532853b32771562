"""Misspecification diagnostics and the MMD metrics without a GPU: the C ABI's host-side checks, the eager-torch
fallback against the fp64 oracle (tests/mmd_oracle.py), the split selection against the Python permutation restatement,
and the public functions' behaviour.  The device route: tests/test_mmd_kernel_gpu.py, tests/test_misspecification_gpu.py.

Bounds (from the eager fp32 composition's own error against fp64 on centred data, about 1.3e-7 / 2.7e-7): bandwidth
within 1e-6 relative, MMD within 2e-6 absolute -- unchanged on inputs shifted by +100, where a Gram-form distance is
20 - 100 times outside them."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import torch

from sbi_amd import _build, _lib
from sbi_amd.diagnostics import (
    calc_misspecification_logprob,
    calc_misspecification_mmd,
    calculate_baseline_mmd,
    calculate_p_misspecification,
    compute_rbf_mmd,
    compute_rbf_mmd_median_heuristic,
    median_heuristic,
    rbf_kernel,
)
from sbi_amd.utils import metrics
from sbi_amd.utils.mmd_splits import rbf_splits, split_indices
from tests import mmd_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW_RTOL, MMD_ATOL = 1e-6, 2e-6
E = inspect.Parameter.empty


def defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items()}


def test_header_and_binding_agree_for_the_mmd_family():
    text = open(os.path.join(ROOT, "include", "sbi_amd_mmd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sbi_amd_\w+)\s*\(", text)))
    assert declared == sorted(_lib.exported_symbols_mmd()) == ["sbi_amd_mmd_rbf_splits"]
    others = (_lib.exported_symbols() + _lib.exported_symbols_sir() + _lib.exported_symbols_maf_affine() +
              _lib.exported_symbols_mnle() + _lib.exported_symbols_mdn() + _lib.exported_symbols_lc2st() +
              _lib.exported_symbols_npse())
    assert not set(declared) & set(others)
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    for name in declared:
        assert hasattr(lib, name)


def test_bad_arguments_are_refused_on_the_host():
    """Nothing is launched: the pointers below are not device memory, and no device is needed."""
    fn = _lib.load().sbi_amd_mmd_rbf_splits
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(pool=p, N=8, D=2, idx=None, seed=0, off=0, S=4, M=6, n_a=2, pair_set=0, median_set=0, bw=None,
              floor=0.0, out=p, stream=None)

    def call(**kw):
        a = {**ok, **kw}
        return fn(a["pool"], a["N"], a["D"], a["idx"], a["seed"], a["off"], a["S"], a["M"], a["n_a"], a["pair_set"],
                  a["median_set"], a["bw"], a["floor"], a["out"], a["stream"])

    assert call(pool=None) == _lib.E_BADARG
    assert call(out=None) == _lib.E_BADARG
    assert call(n_a=6) == _lib.E_BADARG and call(n_a=7) == _lib.E_BADARG and call(n_a=0) == _lib.E_BADARG
    assert call(M=1, n_a=1) == _lib.E_BADARG
    assert call(S=-1) == _lib.E_BADARG
    assert call(D=0) == _lib.E_BADARG
    assert call(pair_set=2) == _lib.E_BADARG and call(median_set=-1) == _lib.E_BADARG
    assert call(floor=-1.0) == _lib.E_BADARG and call(floor=float("nan")) == _lib.E_BADARG
    assert call(M=9, n_a=2) == _lib.E_BADARG                    # idx == NULL: a split cannot exceed the pool
    assert call(S=0) == 0                                         # a no-op
    assert call(N=20000, M=15361, D=1, n_a=5) == _lib.E_UNSUPPORTED    # past the LDS staging budget
    assert call(N=20000, M=1397, D=10, n_a=5) == _lib.E_UNSUPPORTED    # 1397 * 11 = 15 367 > 15 360


def test_signatures_follow_the_reference():
    assert defaults(rbf_kernel) == dict(x=E, y=E, bandwidth=E)
    assert defaults(median_heuristic) == dict(x=E, y=E)
    assert defaults(compute_rbf_mmd) == dict(x=E, y=E, bandwidth=1.0, mode="biased")
    assert defaults(compute_rbf_mmd_median_heuristic) == dict(x=E, y=E, mode="biased")
    assert defaults(calculate_baseline_mmd) == dict(n_obs=E, y=E, n_shuffle=1000, max_samples=1000, mode="biased",
                                                    seed=None)
    assert defaults(calculate_p_misspecification) == dict(x_obs=E, x=E, n_shuffle=1000, max_samples=1000,
                                                          mode="biased", seed=None)
    assert defaults(calc_misspecification_mmd) == dict(x_obs=E, x=E, inference=None, mode="x_space", n_shuffle=1000,
                                                       max_samples=1000, mmd_mode="biased", seed=None)
    assert defaults(calc_misspecification_logprob) == dict(x_val=E, x_o=E, estimator=E, alpha=0.05)
    assert defaults(metrics.unbiased_mmd_squared) == dict(x=E, y=E, scale=None)
    assert defaults(metrics.biased_mmd) == dict(x=E, y=E, scale=None)
    assert defaults(metrics.biased_mmd_hypothesis_test) == dict(x=E, y=E, alpha=0.05)
    assert defaults(metrics.unbiased_mmd_squared_hypothesis_test) == dict(x=E, y=E, alpha=0.05)


@pytest.mark.parametrize("N,D,n_obs,M", [(70, 5, 3, 67), (40, 1, 1, 40), (64, 3, 63, 64)])
@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_fallback_matches_the_fp64_oracle(N, D, n_obs, M, shift):
    g = torch.Generator().manual_seed(N)
    y = 2 * torch.randn(N, D, generator=g) + 1 + shift
    S, seed = 4, 1234 + N
    idx = split_indices(N, M, seed, S)
    for s in range(S):
        want = mmd_oracle.split_rows(N, M, seed, s)
        assert idx[s].tolist() == want and len(set(want)) == M
    got_sums = rbf_splits(y, S, M, n_obs, 0, 0, seed=seed)
    for mode in ("biased", "unbiased"):
        base = calculate_baseline_mmd(n_obs, y, n_shuffle=S, max_samples=M, mode=mode, seed=seed)
        assert base.shape == (S,) and base.dtype == torch.float32
        for s in range(S):
            o = mmd_oracle.sums(y[idx[s]], n_obs, 0, 0)
            assert abs(got_sums[s, 0].item() - o[0].item()) <= BW_RTOL * o[0].item()
            want = mmd_oracle.mmd_from_sums(o, n_obs, M - n_obs, mode)
            if np.isfinite(want):
                assert abs(base[s].item() - want) <= MMD_ATOL, (mode, s, base[s].item(), want)
            else:       # a one-row set in the unbiased estimator: the formula divides by zero
                assert not np.isfinite(base[s].item())


def test_split_offset_and_explicit_indices_select_the_same_splits():
    y = torch.randn(50, 3)
    all_ = rbf_splits(y, 6, 20, 4, 1, 1, seed=9)
    tail = rbf_splits(y, 3, 20, 4, 1, 1, seed=9, split_offset=3)
    assert torch.equal(all_[3:], tail)
    idx = split_indices(50, 20, 9, 6)
    assert torch.equal(rbf_splits(y, 6, 20, 4, 1, 1, idx=idx), all_)
    # a non-finite row poisons its split alone
    y2 = y.clone()
    y2[idx[2, 7]] = float("nan")
    got = rbf_splits(y2, 6, 20, 4, 1, 1, idx=idx)
    hit = [(idx[s] == idx[2, 7]).any().item() for s in range(6)]
    for s in range(6):
        assert torch.isnan(got[s]).all() if hit[s] else torch.equal(got[s], all_[s])


def test_metrics_match_their_fp64_restatements():
    g = torch.Generator().manual_seed(3)
    for nx, ny, d, shift in [(30, 41, 3, 0.0), (17, 2, 1, 0.0), (50, 50, 6, 100.0)]:
        x = 2 * torch.randn(nx, d, generator=g) + 1 + shift
        y = 1.5 * torch.randn(ny, d, generator=g) + shift
        for scale in (None, 0.7, 3.0):
            b = metrics.biased_mmd(x, y, scale)
            u = metrics.unbiased_mmd_squared(x, y, scale)
            assert b.dim() == 0 and u.dim() == 0
            # sqrt amplifies the error of its argument by 1 / (2 sqrt): the bound is set on the squared MMD
            assert abs(b.item() ** 2 - mmd_oracle.biased_mmd(x, y, scale) ** 2) <= MMD_ATOL
            assert abs(u.item() - mmd_oracle.unbiased_mmd_squared(x, y, scale)) <= 2 * MMD_ATOL    # 2 (kxx + ...)
    # identical samples, strict lower triangles: every median candidate but the cross diagonal is positive
    x = torch.randn(12, 2, generator=g)
    assert abs(metrics.unbiased_mmd_squared(x, x).item() - mmd_oracle.unbiased_mmd_squared(x, x)) <= 2 * MMD_ATOL
    # all rows equal: the median is 0 and the 1e-8 floor keeps the kernel finite: every term is exp(0)
    c = torch.ones(5, 2)
    assert metrics.unbiased_mmd_squared(c, c).item() == pytest.approx(2 * (0.5 + 0.5 - 1.0), abs=1e-6)
    with pytest.raises(AssertionError, match="size 1"):
        metrics.unbiased_mmd_squared(torch.randn(1, 2), torch.randn(5, 2))
    with pytest.raises(AssertionError, match="size 1"):
        metrics.unbiased_mmd_squared(torch.randn(5, 2), torch.randn(1, 2))
    # without a floor a zero bandwidth gives what the formula gives: 0 / 0 on the zero distances
    assert torch.isnan(metrics.biased_mmd(c, c))


def test_hypothesis_test_helpers():
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(40, 3, generator=g), torch.randn(40, 3, generator=g) + 0.5
    m, thr = metrics.biased_mmd_hypothesis_test(x, y, alpha=0.1)
    assert m == metrics.biased_mmd(x, y).item()
    assert thr == pytest.approx(np.sqrt(2 / 40) * (1 + np.sqrt(-2 * np.log(0.1))))
    m, thr = metrics.unbiased_mmd_squared_hypothesis_test(x, y)
    assert m == metrics.unbiased_mmd_squared(x, y).item()
    assert thr == pytest.approx((4 / np.sqrt(40)) * np.sqrt(-np.log(0.05)))
    with pytest.raises(AssertionError):
        metrics.biased_mmd_hypothesis_test(x, y[:10])
    with pytest.raises(AssertionError):
        metrics.unbiased_mmd_squared_hypothesis_test(x, y[:10])


def test_small_helpers_match_the_formula():
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(9, 4, generator=g) + 100, torch.randn(13, 4, generator=g) + 100
    d = torch.cdist(x.double(), y.double(), compute_mode="donot_use_mm_for_euclid_dist")
    bw = median_heuristic(x, y)
    assert isinstance(bw, float) and abs(bw - torch.median(d).item()) <= BW_RTOL * bw
    k = rbf_kernel(x, y, 1.3)
    assert k.shape == (9, 13) and torch.allclose(k.double(), torch.exp(-d**2 / (2 * 1.3**2)), atol=1e-6)
    for mode in ("biased", "unbiased"):
        want = mmd_oracle.mmd_from_sums(mmd_oracle.sums(torch.cat((x, y)), 9, 0, 0, bandwidth=1.3), 9, 13, mode)
        assert abs(compute_rbf_mmd(x, y, 1.3, mode).item() - want) <= MMD_ATOL
        got = compute_rbf_mmd_median_heuristic(x, y, mode)
        assert got.dim() == 0 and abs(got.item() - mmd_oracle.misspecification_mmd(x, y, mode)) <= MMD_ATOL
    with pytest.raises(ValueError, match="mode should be either biased or unbiased"):
        compute_rbf_mmd(x, y, 1.0, "other")


def test_mmd_test_accepts_the_same_distribution_and_rejects_a_shift():
    """Under H_0 the p-value is uniform on [0, 1], so one draw in twenty falls below 0.05 by construction: the data are
    a fixed draw (eight consecutive generator seeds gave p = 0.17 ... 0.98 here, the shifted observations 0.0 each
    time)."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2000, 4, generator=g)
    x_obs = torch.randn(20, 4, generator=g)
    p, (base, mmd) = calc_misspecification_mmd(x_obs, x, n_shuffle=200, max_samples=300, seed=42)
    assert base.shape == (200,) and mmd.dim() == 0
    assert p > 0.05
    assert p == 1 - (base < mmd).sum().item() / 200
    p, (base, mmd) = calc_misspecification_mmd(x_obs + 3, x, n_shuffle=200, max_samples=300, seed=42)
    assert p == 0.0 and base.shape == (200,)
    # the observed statistic is the fp64 formula on (x_obs, x[:max_samples])
    assert abs(mmd.item() - mmd_oracle.misspecification_mmd(x_obs + 3, x[:300])) <= MMD_ATOL


class _Net:
    def __init__(self, embedding_net):
        self.embedding_net = embedding_net


class _Inference:
    def __init__(self, embedding_net=None, trained=True):
        self._neural_net = _Net(embedding_net) if trained else None


def test_embedding_mode_errors_and_warning():
    g = torch.Generator().manual_seed(13)
    x, x_obs = torch.randn(120, 6, generator=g), torch.randn(8, 6, generator=g) + 1
    lin = torch.nn.Linear(6, 3)
    kw = dict(n_shuffle=16, max_samples=50, seed=5)
    p_e, (b_e, m_e) = calc_misspecification_mmd(x_obs, x, inference=_Inference(lin), mode="embedding", **kw)
    with torch.no_grad():
        p_x, (b_x, m_x) = calc_misspecification_mmd(lin(x_obs), lin(x), **kw)
    assert p_e == p_x and torch.equal(b_e, b_x) and torch.equal(m_e, m_x) and not b_e.requires_grad
    with pytest.raises(ValueError, match="inference should not be None if mode is 'embedding'"):
        calc_misspecification_mmd(x_obs, x, mode="embedding", **kw)
    with pytest.raises(ValueError, match="No neural net found. The inference object must be trained"):
        calc_misspecification_mmd(x_obs, x, inference=_Inference(trained=False), mode="embedding", **kw)
    with pytest.raises(ValueError, match="mode should be either 'x_space' or 'embedding'"):
        calc_misspecification_mmd(x_obs, x, mode="latent", **kw)
    with pytest.warns(UserWarning, match="The embedding net might be the identity function"):
        p_i, (b_i, _) = calc_misspecification_mmd(x_obs, x, inference=_Inference(torch.nn.Identity()),
                                                  mode="embedding", **kw)
    p_plain, (b_plain, _) = calc_misspecification_mmd(x_obs, x, **kw)
    assert p_i == p_plain and torch.equal(b_i, b_plain)
    with pytest.raises(AttributeError, match="embedding_net attribute is None"):
        calc_misspecification_mmd(x_obs, x, inference=_Inference(None), mode="embedding", **kw)


def test_sample_count_errors():
    y = torch.randn(30, 2)
    with pytest.raises(ValueError, match="n of observed samples should be less than n of synthetic samples"):
        calculate_baseline_mmd(31, y)
    with pytest.raises(ValueError, match=r"\(30\).*= 30"):
        calculate_baseline_mmd(30, y)
    with pytest.raises(ValueError, match=r"\(12\).*= 10"):
        calculate_baseline_mmd(12, y, max_samples=10)
    with pytest.raises(ValueError, match="mode should be either biased or unbiased"):
        calculate_baseline_mmd(3, y, mode="other")


def test_seed_none_follows_torch_manual_seed_and_seeds_differ():
    y = torch.randn(80, 3)
    torch.manual_seed(123)
    a = calculate_baseline_mmd(5, y, n_shuffle=8, max_samples=40)
    torch.manual_seed(123)
    b = calculate_baseline_mmd(5, y, n_shuffle=8, max_samples=40)
    c = calculate_baseline_mmd(5, y, n_shuffle=8, max_samples=40)
    assert torch.equal(a, b) and not torch.equal(a, c)
    s1 = calculate_baseline_mmd(5, y, n_shuffle=8, max_samples=40, seed=1)
    s2 = calculate_baseline_mmd(5, y, n_shuffle=8, max_samples=40, seed=2)
    assert torch.equal(s1, calculate_baseline_mmd(5, y, n_shuffle=8, max_samples=40, seed=1))
    assert not torch.equal(s1, s2)
    torch.manual_seed(7)
    p1 = calculate_p_misspecification(y[:5] + 0.3, y[5:], n_shuffle=8, max_samples=40)[0]
    torch.manual_seed(7)
    assert p1 == calculate_p_misspecification(y[:5] + 0.3, y[5:], n_shuffle=8, max_samples=40)[0]


class _Gaussian:
    """Stub marginal estimator: an analytic isotropic normal, sampling from a (possibly different) location."""

    def __init__(self, dim, sample_loc=0.0):
        self.d = torch.distributions.MultivariateNormal(torch.zeros(dim), torch.eye(dim))
        self.sample_loc = sample_loc

    def log_prob(self, x):
        return self.d.log_prob(x)

    def sample(self, shape):
        return self.d.sample(shape) + self.sample_loc


def test_logprob_test_on_an_analytic_estimator():
    g = torch.Generator().manual_seed(17)
    x_val = torch.randn(200, 2, generator=g)
    est = _Gaussian(2)
    lp = est.log_prob(x_val)
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # a well-specified estimator does not warn
        p, rej = calc_misspecification_logprob(x_val, torch.zeros(1, 2), est)
    assert p.item() == 1.0 and not bool(rej)        # the mode has the highest log-probability
    x_o = torch.tensor([[1.5, -1.0]])
    p, rej = calc_misspecification_logprob(x_val, x_o, est, alpha=0.5)
    want = (lp <= est.log_prob(x_o).item()).float().mean()
    assert p == want and bool(rej) == bool(want < 0.5)
    assert bool(calc_misspecification_logprob(x_val, x_o, est, alpha=want.item() + 1e-3)[1])
    assert not bool(calc_misspecification_logprob(x_val, x_o, est, alpha=want.item())[1])
    with pytest.warns(UserWarning, match="results might not be meaningful"):
        calc_misspecification_logprob(x_val, x_o, _Gaussian(2, sample_loc=3.0))
