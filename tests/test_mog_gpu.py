"""The NPE-A mixture kernels (csrc/mog.hip, include/sbi_amd_mog.h) on the device against fp64: the restatement
tests/npe_a_oracle.py and the recorded outputs of the real sbi functions (tests/golden/npe_a_reference.pt).

Bound: the project's row parity |d| <= 1e-5 (1 + |ref|) on every entry of all four outputs of the correction, of
log_prob and of sample with given components.  Inputs follow the recipe of npe_a_oracle.recipe (density factor
diagonal U(2, 4), proposal U(0.5, 1), prior U(0.2, 0.3)): the corrected precisions have minimum eigenvalue >= 1.6
and the eager fp32 route is within 4.1e-6 (1 + |ref|) of fp64 (both measured on the host at the five shapes).  Shapes
(D, K, L): (1, 3, 1), (3, 4, 2), (10, 10, 10), (16, 16, 4) and (10, 10, 100) -- M = 1000 is past one LDS group of the
log_prob kernel (32 components) and past the MDN kernels' 16; B and n in {1, 17, 333}: one partial 16-pair workgroup,
one partial 16-row tile, more than one workgroup (256 rows) of the log_prob kernel.

The ill-conditioned case (smallest corrected eigenvalue about 1e-3) does not owe 1e-5: its bound is four times the
error of the eager fp32 route on the same inputs, measured in the same test."""

import functools
import os

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators import mog_ops
from sbi_amd.neural_nets.estimators.mdn import MoG
from sbi_amd.utils.parity import row_parity
from tests import npe_a_oracle as oracle
from tests import parity_log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "npe_a_reference.pt")

# (D, K, L, B, prop_rows, prior)
CASES = [(1, 3, 1, 333, 333, True), (1, 3, 1, 1, 1, False), (3, 4, 2, 333, 1, False), (3, 4, 2, 17, 17, True),
         (10, 10, 10, 17, 1, True), (10, 10, 10, 333, 1, False), (16, 16, 4, 17, 17, True), (16, 16, 4, 1, 1, False),
         (10, 10, 100, 1, 1, True), (10, 10, 100, 17, 17, False)]
NAMES = ("logits", "means", "precisions", "factors")


def cuda(*ts):
    return tuple(None if t is None else t.cuda().contiguous() for t in ts)


@functools.lru_cache(maxsize=None)
def solved(case):
    """Inputs, the fp64 restatement and the kernel's outputs of one case (computed once, never written to)."""
    D, K, L, B, rows, prior = case
    d, p, m0, P0 = oracle.recipe(D, K, L, B, rows, prior)
    ref = oracle.correct(d, p, m0, P0)
    got = mog_ops.correct_kernel(*cuda(d[0], d[1], d[2], p[0], p[1], p[2], m0, P0))
    torch.cuda.synchronize()
    return d, p, m0, P0, ref, got


@pytest.mark.parametrize("case", CASES, ids=str)
def test_correct_matches_fp64(case):
    d, p, m0, P0, ref, got = solved(case)
    assert got[4].dtype == torch.int32 and not got[4].any()
    for name, g, r in zip(NAMES, got, ref):
        par = row_parity(g.cpu(), r)
        print(case, name, par["worst_scaled"])
        parity_log.record("mog_correct", f"{case} {name}", worst_scaled=par["worst_scaled"], max_abs=par["max_abs"])
        assert torch.isfinite(g).all() and par["exceed_frac"] == 0.0, (name, par)
    assert torch.equal(got[3], torch.triu(got[3]))


@pytest.mark.parametrize("zscore", [False, True])
@pytest.mark.parametrize("n", [1, 17, 333])
@pytest.mark.parametrize("case", [c for c in CASES if c[3] > 1 or c[2] == 100], ids=str)
def test_log_prob_matches_fp64(case, n, zscore):
    D, K, L, B = case[:4]
    mix = tuple(t.float() for t in solved(case)[4])           # the fp32 mixture both sides evaluate
    g = torch.Generator().manual_seed(n + D)
    shift = 0.3 * torch.randn(D, generator=g) if zscore else None
    scale = 0.5 + torch.rand(D, generator=g) if zscore else None
    for rows in {1, B}:
        m = tuple(t[:rows].contiguous() for t in mix)
        theta = 0.6 * torch.randn(n if rows == 1 else min(n, 2) * rows, D, generator=g)
        if zscore:
            theta = theta * scale + shift
        ref = oracle.log_prob(*m, theta, shift, scale)
        got = mog_ops.log_prob_kernel(*cuda(*m, theta, shift, scale)).cpu()
        par = row_parity(got, ref)
        print(case, n, rows, zscore, par["worst_scaled"])
        parity_log.record("mog_log_prob", f"{case} n={theta.shape[0]} mog_rows={rows} zscore={zscore}",
                          worst_scaled=par["worst_scaled"], max_abs=par["max_abs"])
        assert torch.isfinite(got).all() and par["exceed_frac"] == 0.0, (rows, par)


@pytest.mark.parametrize("zscore", [False, True])
@pytest.mark.parametrize("case", [c for c in CASES if c[3] > 1 or c[2] == 100], ids=str)
def test_sample_matches_fp64_and_selects_by_the_cumulative_weights(case, zscore):
    D, K, L, B = case[:4]
    M = K * L
    mix = tuple(t.float() for t in solved(case)[4])
    g = torch.Generator().manual_seed(7 + D)
    shift = 0.3 * torch.randn(D, generator=g) if zscore else None
    scale = 0.5 + torch.rand(D, generator=g) if zscore else None
    for rows, n in ((1, 333), (B, 3 * B + 1)):
        logits, means, _, fac = (t[:rows].contiguous() for t in mix)
        zeta = torch.randn(n, D, generator=g)
        comp = torch.randint(0, M, (n,), generator=g, dtype=torch.int32)
        ref = oracle.sample(means, fac, comp, zeta, shift, scale)
        got = mog_ops.sample_kernel(*cuda(logits, means, fac, zeta), comp=comp.cuda(), shift=cuda(shift)[0],
                                    scale=cuda(scale)[0]).cpu()
        par = row_parity(got, ref)
        parity_log.record("mog_sample", f"{case} n={n} mog_rows={rows} zscore={zscore}",
                          worst_scaled=par["worst_scaled"])
        assert par["exceed_frac"] == 0.0, (rows, par)
        # selection by u: exact agreement with the fp64 cumulative sum away from the boundaries, and at both ends
        u = torch.rand(n, generator=g)
        u[0], u[-1] = 0.0, torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
        k, dist = oracle.select(logits, u)
        keep = dist > 1e-6
        keep[0] = keep[-1] = True
        by_u = mog_ops.sample_kernel(*cuda(logits, means, fac, zeta, u)).cpu()
        by_k = mog_ops.sample_kernel(*cuda(logits, means, fac, zeta), comp=k.to(torch.int32).cuda()).cpu()
        assert keep.float().mean() > 0.9 and torch.equal(by_u[keep], by_k[keep])
        assert torch.equal(mog_ops.select_components(logits, u)[keep], k[keep])


@pytest.mark.parametrize("key", ["d1k3l1_prior", "d1k3l1_uniform", "d3k4l2_prior", "d3k4l2_uniform"])
def test_matches_the_recorded_outputs_of_the_reference_functions(key):
    c = torch.load(GOLDEN)[key]
    d, p = (tuple(t.float() for t in c[k]) for k in ("density", "proposal"))
    prior = None
    if "prior_mean" in c:
        prior = MoG.from_gaussian(c["prior_mean"].float(), c["prior_cov"].float()).to("cuda")
        for got, want in zip((prior.logits, prior.means, prior.precisions, prior.precision_factors), c["from_gaussian"]):
            assert row_parity(got.cpu(), want)["exceed_frac"] == 0.0
    post = mog_ops.correct_for_proposal(MoG(*cuda(*d)), MoG(*cuda(*p)), prior)
    assert post.logits.is_cuda
    for name, got, want in zip(NAMES, (post.logits, post.means, post.precisions, post.precision_factors),
                               c["corrected"]):
        par = row_parity(got.cpu(), want)
        parity_log.record("mog_golden", f"{key} {name}", worst_scaled=par["worst_scaled"])
        assert par["exceed_frac"] == 0.0, (name, par)
    # log_prob and sample of the RECORDED corrected mixture (fp32 copies of it), so each kernel is pinned on its own
    rec = MoG(*cuda(*(t.float() for t in c["corrected"])))
    for theta, want in ((c["theta"], c["log_prob"]), (c["theta"][0], c["log_prob_2d"])):
        got = rec.log_prob(theta.float().cuda())
        assert got.shape == want.shape and row_parity(got.cpu(), want)["exceed_frac"] == 0.0
    B, S = c["choices"].shape
    comp = c["choices"].T.reshape(-1).to(torch.int32)                       # rows sample-major: i = s B + b
    zeta = c["z"][..., 0].transpose(0, 1).reshape(S * B, -1).float()
    got = mog_ops.sample_kernel(rec.logits, rec.means, rec.precision_factors, zeta.cuda(), comp=comp.cuda())
    assert row_parity(got.cpu().reshape(S, B, -1), c["samples"])["exceed_frac"] == 0.0
    # fed the recorded choices, the kernel uses exactly those components: a draw with zeta = 0 is the chosen mean
    picked = mog_ops.sample_kernel(rec.logits, rec.means, rec.precision_factors, torch.zeros_like(zeta).cuda(),
                                   comp=comp.cuda())
    row = torch.arange(S * B) % B
    assert torch.equal(picked.cpu(), rec.means.cpu()[row, comp.long()])


def test_batch_slices_are_bit_identical():
    case = (10, 10, 10, 333, 1, False)
    d, p, m0, P0, ref, got = solved(case)
    a, b = 37, 250
    part = mog_ops.correct_kernel(*cuda(d[0][a:b], d[1][a:b], d[2][a:b], p[0], p[1], p[2]))
    assert all(torch.equal(x, y[a:b]) for x, y in zip(part, got))
    case = (3, 4, 2, 17, 17, True)
    d, p, m0, P0, ref, got = solved(case)
    part = mog_ops.correct_kernel(*cuda(d[0][3:9], d[1][3:9], d[2][3:9], p[0][3:9], p[1][3:9], p[2][3:9], m0, P0))
    assert all(torch.equal(x, y[3:9]) for x, y in zip(part, got))
    g = torch.Generator().manual_seed(3)
    for case in ((10, 10, 100, 1, 1, True), (3, 4, 2, 17, 17, True)):
        D, B = case[0], case[3]
        mix = tuple(t.contiguous() for t in solved(case)[5][:4])
        theta = (0.6 * torch.randn(20 * B + 600, D, generator=g)).cuda()
        zeta = torch.randn(theta.shape[0], D, generator=g).cuda()
        u = torch.rand(theta.shape[0], generator=g).cuda()
        lo = 5 * B                                                    # (a slice that keeps row i on mixture i % B)
        hi = lo + B * (293 if B == 1 else 40)
        full = mog_ops.log_prob_kernel(*mix, theta)
        assert torch.equal(mog_ops.log_prob_kernel(*mix, theta[lo:hi].contiguous()), full[lo:hi])
        full = mog_ops.sample_kernel(mix[0], mix[1], mix[3], zeta, u)
        assert torch.equal(mog_ops.sample_kernel(mix[0], mix[1], mix[3], zeta[lo:hi].contiguous(),
                                                 u[lo:hi].contiguous()), full[lo:hi])


def test_a_non_positive_definite_row_sets_only_its_own_status():
    case = (3, 4, 2, 17, 17, True)
    d, p, m0, P0, ref, good = solved(case)
    D, K, L = case[:3]
    g = torch.Generator().manual_seed(5)
    bad_row = oracle.mixture(g, 1, L, D, 0.5, 1.0, 0.5)
    A = bad_row[3].clone()
    i = torch.arange(D)
    A[..., i, i] = 5.0                                            # proposal sharper than the density: S is indefinite
    pl, pm, pP = p[0].clone(), p[1].clone(), p[2].clone()
    pP[5] = (A.transpose(-1, -2) @ A)[0]
    got = mog_ops.correct_kernel(*cuda(d[0], d[1], d[2], pl, pm, pP, m0, P0))
    status = got[4].cpu()
    assert status[5] == 1 and status.count_nonzero() == 1          # 1 + the first failing j (j = 0)
    others = torch.arange(17) != 5
    assert all(torch.equal(x[others], y[others]) for x, y in zip(got[:4], good[:4]))
    assert all(torch.isfinite(x).all() for x in got[:4])
    with pytest.raises(ValueError, match="Posterior precision matrix is not positive definite"):
        mog_ops.correct_for_proposal(MoG(*cuda(d[0], d[1], d[2])), MoG(*cuda(pl, pm, pP)), None)


def test_envelope_refusals_and_empty_calls():
    lib = _lib.load()
    t = torch.zeros(64, device="cuda")
    P = _lib.ptr(t)
    st = _lib.current_stream(t.device)
    for K, L, D in ((4, 2, 17), (65537, 1, 3), (257, 256, 3)):
        bad = _lib.E_UNSUPPORTED if D == 17 or K * L > 65536 else None
        assert lib.sbi_amd_mog_correct_workspace_bytes(1, K, L, D, 1) == bad
        assert lib.sbi_amd_mog_correct(P, P, P, 1, K, P, P, P, 1, L, D, None, None, 1e-6, P, P, P, P, P, P, st) == bad
        assert lib.sbi_amd_mog_log_prob(P, P, P, P, 1, K * L, D, P, 1, None, None, P, st) == bad
        assert lib.sbi_amd_mog_sample(P, P, P, 1, K * L, D, P, None, P, 1, None, None, P, P, st) == bad
    assert lib.sbi_amd_mog_correct(P, P, P, 0, 4, P, P, P, 1, 2, 3, None, None, 1e-6, P, P, P, P, P, P, st) == 0
    assert lib.sbi_amd_mog_log_prob(P, P, P, P, 1, 8, 3, P, 0, None, None, P, st) == 0
    assert lib.sbi_amd_mog_sample(P, P, P, 1, 8, 3, P, None, P, 0, None, None, P, P, st) == 0
    assert lib.sbi_amd_mog_correct(P, P, P, 2, 4, P, P, P, 3, 2, 3, None, None, 1e-6, P, P, P, P, P, P, st) == _lib.E_BADARG
    assert not mog_ops.in_envelope(17, 8) and not mog_ops.in_envelope(3, 65537) and mog_ops.in_envelope(16, 65536)
    torch.cuda.synchronize()
    assert not t.any()


def test_ill_conditioned_correction_is_within_four_times_the_eager_fp32_error():
    """Proposal factor diagonal scaled until the smallest corrected eigenvalue is about 1e-3 (bisection in fp64 on
    the host).  Recorded on the MI355X: see profiles/parity_npe_a.json (mog_ill_conditioned)."""
    D, K, L, B = 3, 4, 2, 17
    g = torch.Generator().manual_seed(21)
    d = oracle.mixture(g, B, K, D, 2.0, 4.0, 0.5)
    state = g.get_state()

    def proposal(t):
        g.set_state(state)
        return oracle.mixture(g, 1, L, D, 0.5, 1.0, 0.5, diag_scale=t)

    def min_eig(t):
        return oracle.min_eigenvalue(d, proposal(t))

    lo, hi = 1.0, 8.0
    assert min_eig(lo) > 1e-3 > min_eig(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if min_eig(mid) > 1e-3 else (lo, mid)
    p = proposal(lo)
    assert 0.9e-3 <= min_eig(lo) <= 1.5e-3
    ref = oracle.correct(d, p)
    args = cuda(d[0], d[1], d[2], p[0], p[1], p[2])
    got = mog_ops.correct_kernel(*args)
    eager = mog_ops.correct_eager(*args)
    assert not got[4].any() and not eager[4].any()
    for name, gk, ge, r in zip(NAMES, got, eager, ref):
        err_k, err_e = row_parity(gk.cpu(), r)["worst_scaled"] * 1e-5, row_parity(ge.cpu(), r)["worst_scaled"] * 1e-5
        print(f"ill-conditioned {name}: kernel {err_k:.3e} eager fp32 {err_e:.3e}")
        parity_log.record("mog_ill_conditioned", name, kernel=err_k, eager_fp32=err_e)
        assert err_k <= 4.0 * err_e, (name, err_k, err_e)
