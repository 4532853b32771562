"""sbi_amd_mixture_lse (csrc/mixture_lse.hip) on the device against the fp64 oracle (tests/abc_oracle.py), and the
bit-level properties include/sbi_amd_abc.h promises.

Bound: the project's row parity, |d| <= 1e-5 (1 + |ref|) on every entry (`row_parity` with its defaults,
exceed_frac == 0).  The eager fp32 composition of the same formula (`mixture_lse_torch` on the host) is held to the same
bound on the same inputs: an input family too wild for fp32 then fails as a yardstick instead of loosening the bound.
Shapes are sampled from M in {1, 2, 63, 64, 65, 255, 256, 257, 1025}, N in {1, 2, 63, 64, 65, 255, 256, 257, 1000,
4097}, D in {1, 2, 3, 10, 31, 32}, H in {1, 10, 16}: around the 64 queries of a workgroup, the 256 centres of a tile,
the four D and four H buckets of the kernel's template."""

import functools
import math

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.utils.kde import mixture_lse_torch
from sbi_amd.utils.parity import row_parity
from tests import abc_oracle, parity_log

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 2, 2, 10), (63, 63, 3, 16), (64, 64, 10, 1), (65, 65, 31, 10), (255, 255, 32, 16),
          (256, 256, 1, 1), (257, 257, 2, 10), (1025, 1000, 3, 16), (64, 4097, 10, 1), (65, 1000, 32, 10),
          (63, 4097, 31, 16), (256, 2, 3, 10), (2, 257, 10, 16)]
FAMILIES = ["normal", "shift100", "wide", "logw"]


def launch(q, c, log_w=None, whiten=None, half_width=None, scale=None, q_group=None, c_group=None, H=None, rc_want=0,
           out=None, M=None, N=None, D=None):
    """One kernel launch through the binding; never the fallback."""
    lib = _lib.load()
    M = q.shape[0] if M is None else M
    N = c.shape[0] if N is None else N
    D = q.shape[1] if D is None else D
    H = (1 if scale is None else scale.shape[0]) if H is None else H
    if out is None:
        out = torch.full((H, max(M, 0)), -7.0, dtype=torch.float32, device="cuda")
    rc = lib.sbi_amd_mixture_lse(_lib.ptr(q), M, _lib.ptr(c), N, D, _lib.ptr(log_w), _lib.ptr(whiten),
                                 _lib.ptr(half_width), _lib.ptr(scale), H, _lib.ptr(q_group), _lib.ptr(c_group),
                                 _lib.ptr(out), _lib.current_stream(out.device))
    assert rc == rc_want, rc
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def inputs(M, N, D, H, family):
    """(q, c, log_w, whiten, scale) on the host, fp32; built once per case and never modified."""
    g = torch.Generator().manual_seed(1000 * M + 7 * N + 31 * D + H + len(family))
    q, c = torch.randn(M, D, generator=g), torch.randn(N, D, generator=g)
    a = torch.randn(D, D, generator=g)
    cov = a @ a.T / D + 0.5 * torch.eye(D)
    chol = torch.linalg.cholesky(cov.double())
    whiten = torch.linalg.solve_triangular(chol, torch.eye(D, dtype=torch.float64), upper=False).float().contiguous()
    scale = torch.linspace(0.5, 2.0, H) if H > 1 else torch.ones(1)
    log_w = None
    if family == "shift100":
        q, c = q + 100.0, c + 100.0
    elif family == "wide":
        q = 30.0 * q
        scale = torch.tensor([1.0, 100.0]).repeat(H)[:H].contiguous()
    elif family == "logw":
        raw = torch.randn(N, generator=g)
        if N > 1:
            raw[torch.rand(N, generator=g) < 0.3] = -math.inf
            raw[0] = 0.0
        log_w = torch.log_softmax(raw, dim=0)
    return q, c, log_w, whiten, scale


def dev(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N,D,H", SHAPES)
def test_gaussian_mode_matches_the_fp64_oracle(M, N, D, H, family):
    q, c, log_w, whiten, scale = inputs(M, N, D, H, family)
    want = abc_oracle.mixture_lse(q, c, log_w, whiten, None, scale)
    got = launch(dev(q), dev(c), dev(log_w), dev(whiten), None, dev(scale)).cpu()
    eager = mixture_lse_torch(q, c, log_w, whiten, None, scale)
    pk, pe = row_parity(got, want), row_parity(eager, want)
    print(f"M={M} N={N} D={D} H={H} {family}: kernel worst_scaled={pk['worst_scaled']:.3e} "
          f"eager worst_scaled={pe['worst_scaled']:.3e} min_ref={float(want.min()):.4g}")
    parity_log.record("mixture_lse_vs_fp64", f"M{M}_N{N}_D{D}_H{H}_{family}", kernel_worst_scaled=pk["worst_scaled"],
                      eager_worst_scaled=pe["worst_scaled"], tol=1e-5)
    assert torch.isfinite(want).all() and torch.isfinite(got).all()
    assert pe["exceed_frac"] == 0, pe          # the yardstick: eager fp32 itself is inside the bound
    assert pk["exceed_frac"] == 0, pk


def test_identity_whitening_is_the_null_pointer_route():
    q, c, log_w, _, scale = inputs(65, 257, 3, 10, "logw")
    want = abc_oracle.mixture_lse(q, c, log_w, None, None, scale)
    got = launch(dev(q), dev(c), dev(log_w), None, None, dev(scale)).cpu()
    assert row_parity(got, want)["exceed_frac"] == 0


@pytest.mark.parametrize("N", [20, 21, 257, 1000])
def test_leave_fold_out_groups(N):
    from sbi_amd.utils.kde import kfold_ids

    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, 2, generator=g)
    folds = kfold_ids(N, 20)
    scale = 1.0 / torch.linspace(0.1, 0.5, 10) ** 2
    want = abc_oracle.mixture_lse(x, x, None, None, None, scale, folds, folds)
    got = launch(dev(x), dev(x), None, None, None, dev(scale), dev(folds), dev(folds)).cpu()
    p = row_parity(got, want)
    print(f"N={N} groups: worst_scaled={p['worst_scaled']:.3e}")
    assert p["exceed_frac"] == 0, p
    assert row_parity(mixture_lse_torch(x, x, None, None, None, scale, folds, folds), want)["exceed_frac"] == 0
    # a query whose group holds every centre has nothing to sum: exactly -inf, in every scale
    one = torch.zeros(N, dtype=torch.int32)
    qg = torch.arange(3, dtype=torch.int32) - 1                      # groups -1, 0, 1: only the middle query matches
    got = launch(dev(x[:3]), dev(x), None, None, None, dev(scale), dev(qg), dev(one)).cpu()
    assert (got[:, 1] == -math.inf).all() and torch.isfinite(got[:, [0, 2]]).all()


def test_box_mode_on_a_dyadic_grid():
    """Points and half widths on a 1/8 grid: every bound c -+ v is exact in fp32.  Query 0 sits exactly on c_0 - v
    (inside), query 1 exactly on c_0 + v (outside in that dimension), query 2 far from every centre (-inf)."""
    g = torch.Generator().manual_seed(3)
    for N, D in [(1, 1), (65, 2), (300, 3), (257, 10)]:
        c = torch.randint(-16, 17, (N, D), generator=g).float() / 8
        q = torch.randint(-16, 17, (70, D), generator=g).float() / 8
        v = torch.randint(4, 12, (D,), generator=g).float() / 8
        q[0], q[1], q[2] = c[0] - v, c[0], 50.0
        q[1, D - 1] = c[0, D - 1] + v[D - 1]
        log_w = torch.log_softmax(torch.randn(N, generator=g), dim=0)
        want = abc_oracle.mixture_lse(q, c, log_w, None, v)
        got = launch(dev(q), dev(c), dev(log_w), None, dev(v), None).cpu()
        assert got[0, 2].item() == -math.inf and want[0, 2].item() == -math.inf
        fin = torch.isfinite(want[0])
        assert torch.equal(torch.isfinite(got[0]), fin) and (got[0][~fin] == -math.inf).all()
        assert fin[0], "the query on the lower bound is inside"
        assert row_parity(got[0][fin], want[0][fin])["exceed_frac"] == 0
        if N == 1:
            assert not fin[1], "the query on the upper bound is outside"
        eager = mixture_lse_torch(q, c, log_w, None, v, None)
        assert torch.equal(torch.isfinite(eager[0]), fin)
        assert row_parity(eager[0][fin], want[0][fin])["exceed_frac"] == 0


def test_a_query_does_not_depend_on_the_launch_around_it():
    q, c, log_w, whiten, scale = (dev(t) for t in inputs(1025, 1000, 3, 16, "normal"))
    full = launch(q, c, log_w, whiten, None, scale)
    part = launch(q[:65].contiguous(), c, log_w, whiten, None, scale)
    assert torch.equal(full[:, :65], part)
    # the same rows further down the grid give the same bits
    moved = launch(torch.cat((q[100:700], q[:65])).contiguous(), c, log_w, whiten, None, scale)
    assert torch.equal(moved[:, 600:], part)


def test_nan_query_poisons_its_row_only():
    q, c, log_w, whiten, scale = (dev(t) for t in inputs(257, 257, 2, 10, "normal"))
    clean = launch(q, c, log_w, whiten, None, scale)
    dirty = q.clone()
    dirty[70, 1] = math.nan
    got = launch(dirty, c, log_w, whiten, None, scale)
    assert torch.isnan(got[:, 70]).all()
    keep = torch.arange(257, device="cuda") != 70
    assert torch.equal(got[:, keep], clean[:, keep])
    v = torch.full((2,), 0.5, device="cuda")
    got = launch(dirty, c, log_w, None, v, None)
    assert torch.isnan(got[0, 70]) and not torch.isnan(got[0, keep]).any()


def test_weight_minus_infinity_removes_a_centre():
    q, c, _, whiten, scale = (dev(t) for t in inputs(65, 65, 31, 10, "normal"))
    lw = torch.zeros(65, device="cuda")
    lw[10:] = -math.inf
    got = launch(q, c, lw, whiten, None, scale)
    want = launch(q, c[:10].contiguous(), None, whiten, None, scale)
    assert torch.equal(got, want)


def test_return_codes_and_nothing_launched():
    q, c, scale = torch.randn(4, 33, device="cuda"), torch.randn(5, 33, device="cuda"), torch.ones(17, device="cuda")
    kw = dict(scale=scale)
    for args in (dict(D=33, H=1), dict(D=3, H=17)):
        out = launch(q, c, rc_want=_lib.E_UNSUPPORTED, **kw, **args)
        assert (out == -7.0).all()
    out = torch.full((1, 4), -7.0, device="cuda")
    lib = _lib.load()
    st = _lib.current_stream(out.device)
    P = _lib.ptr
    bad = [
        (None, 4, P(c), 5, 3, P(scale), 1, P(out)), (P(q), 4, None, 5, 3, P(scale), 1, P(out)),
        (P(q), 4, P(c), 5, 3, P(scale), 1, None), (P(q), 4, P(c), 5, 3, None, 1, P(out)),
        (P(q), -1, P(c), 5, 3, P(scale), 1, P(out)), (P(q), 4, P(c), 0, 3, P(scale), 1, P(out)),
        (P(q), 4, P(c), 5, 0, P(scale), 1, P(out)),
    ]
    for qq, M, cc, N, D, sc, H, oo in bad:
        assert lib.sbi_amd_mixture_lse(qq, M, cc, N, D, None, None, None, sc, H, None, None, oo, st) == _lib.E_BADARG
    assert lib.sbi_amd_mixture_lse(P(q), 0, P(c), 5, 3, None, None, None, P(scale), 1, None, None, P(out), st) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()
