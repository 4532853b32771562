"""sbi_amd_mmd_rbf_splits (csrc/mmd.hip) on the device against the fp64 oracle (tests/mmd_oracle.py), and the
bit-level properties include/sbi_amd_mmd.h promises.

Bounds: bandwidth within 1e-6 relative, MMD (biased and unbiased normalisation of the sums) within 2e-6 absolute of fp64
-- about 8 x the eager fp32 composition's own error on centred data (1.3e-7 / 2.7e-7), and the SAME bounds on inputs
shifted by +100, where that composition (cdist's Gram form) is 20 - 100 x outside them: the test that distances are
differences.  For the strict-lower-triangle sums (pair_set 1) the MMD-like combination checked is the one
`unbiased_mmd_squared` uses without its factor 2.  Measured errors go to the parity artifact (tests/parity_log.py ->
profiles/parity_mmd.json).  Shapes are the smallest at which each mechanism can break: M off and on the wave size, a
one-row A, a one-row B, D = 1, odd D, the widest D, even and odd populations."""

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.utils.mmd_splits import STAGE_FLOATS, rbf_splits, split_indices
from tests import mmd_oracle, parity_log

pytestmark = pytest.mark.gpu
BW_RTOL, MMD_ATOL = 1e-6, 2e-6
SHAPES = [(2, 1, 1), (67, 3, 5), (64, 63, 3), (65, 1, 1), (200, 37, 64), (129, 64, 10)]


def launch(pool, S, M, n_a, pair_set, median_set, idx=None, seed=0, split_offset=0, bandwidth=None, bw_floor=0.0):
    """One kernel launch through the binding; never the fallback."""
    lib = _lib.load()
    dev = pool.device
    idx32 = None if idx is None else idx.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.full((S, 4), -7.0, dtype=torch.float32, device=dev)
    rc = lib.sbi_amd_mmd_rbf_splits(_lib.ptr(pool), pool.shape[0], pool.shape[1], _lib.ptr(idx32), seed, split_offset,
                                    S, M, n_a, pair_set, median_set, _lib.ptr(bandwidth), bw_floor, _lib.ptr(out),
                                    _lib.current_stream(dev))
    assert rc == 0, rc
    return out


def combos(s, n_a, n_b, pair_set):
    """The statistics built from [bw, S_aa, S_bb, S_ab] (fp64), each O(1): what the 2e-6 bound applies to."""
    s = s.double()
    cross = s[3] / (n_a * n_b)
    if pair_set == 0:
        vals = [s[1] / n_a**2 + s[2] / n_b**2 - 2 * cross]                      # biased
        if n_a > 1 and n_b > 1:
            vals.append(s[1] / (n_a * (n_a - 1)) + s[2] / (n_b * (n_b - 1)) - 2 * cross)
        return vals
    kaa = s[1] / (n_a * (n_a - 1)) if n_a > 1 else s[1]                         # (an empty triangle sums to 0)
    kbb = s[2] / (n_b * (n_b - 1)) if n_b > 1 else s[2]
    return [kaa + kbb - cross]


@pytest.fixture(scope="module")
def pools():
    """One pool per shape (N = M + 9 rows, 2 randn + 1), shared and never modified."""
    g = torch.Generator().manual_seed(2024)
    return {(M, n_a, D): 2 * torch.randn(M + 9, D, generator=g) + 1 for M, n_a, D in SHAPES}


@pytest.mark.parametrize("shift", [0.0, 100.0])
@pytest.mark.parametrize("M,n_a,D", SHAPES)
def test_sums_and_bandwidth_match_the_fp64_oracle(pools, M, n_a, D, shift):
    pool = pools[(M, n_a, D)] + shift
    N, S, seed = pool.shape[0], 3, 77
    idx = split_indices(N, M, seed, S)
    dpool = pool.cuda()
    worst_bw, worst_mmd = 0.0, 0.0
    for pair_set in (0, 1):
        for median_set in (0, 1):
            got = launch(dpool, S, M, n_a, pair_set, median_set, seed=seed).cpu()
            for s in range(S):
                want = mmd_oracle.sums(pool[idx[s]], n_a, pair_set, median_set)
                if want[0].item() == 0.0:
                    # (M = 2 with the diagonals in the population: the lower median of {0, 0, d} is 0.)  No relative
                    # error exists: the bandwidth must be exactly 0 and the sums what the formula gives there, NaN
                    # where a zero distance is summed (0 / 0) and exactly 0 elsewhere
                    assert got[s, 0].item() == 0.0
                    assert torch.equal(torch.isnan(got[s, 1:]), torch.isnan(want[1:]))
                    assert (got[s, 1:][~torch.isnan(got[s, 1:])] == 0.0).all()
                    continue
                bw_err = abs(got[s, 0].item() - want[0].item()) / want[0].item()
                errs = [abs(a.item() - b.item())
                        for a, b in zip(combos(got[s], n_a, M - n_a, pair_set), combos(want, n_a, M - n_a, pair_set))]
                worst_bw, worst_mmd = max(worst_bw, bw_err), max(worst_mmd, *errs)
                print(f"M={M} n_a={n_a} D={D} shift={shift} ps={pair_set} ms={median_set} s={s} "
                      f"bw_rel={bw_err:.3e} mmd_abs={max(errs):.3e}")
    parity_log.record("mmd_kernel_vs_fp64", f"M{M}_na{n_a}_D{D}_shift{int(shift)}", bw_rel=worst_bw,
                      mmd_abs=worst_mmd, bw_bound=BW_RTOL, mmd_bound=MMD_ATOL)
    assert worst_bw <= BW_RTOL and worst_mmd <= MMD_ATOL


@pytest.mark.parametrize("k", [-20, 0, 20])
def test_integer_grid_bandwidth_is_bit_exact(k):
    """Small integer coordinates (scaled by 2^k): every d^2 is an exact fp32 number, with many ties, duplicate rows and
    zero distances.  The selected element must be the one torch.median picks, to the bit; the scale moves its leading
    digit between radix passes."""
    g = torch.Generator().manual_seed(5 + k)
    for M, n_a, D in [(67, 30, 3), (64, 1, 2), (130, 65, 1)]:
        rows = torch.randint(-3, 4, (M, D), generator=g).float()
        rows[M // 2:M // 2 + 5] = rows[0]                       # duplicate rows in both sets
        rows = rows * 2.0**k
        idx = torch.arange(M).reshape(1, M)
        a, b = rows[:n_a].double(), rows[n_a:].double()
        for pair_set in (0, 1):
            for median_set in (0, 1):
                got = launch(rows.cuda(), 1, M, n_a, pair_set, median_set, idx=idx).cpu()[0, 0]
                if median_set == 0:
                    want = torch.median(torch.cdist(a, b)).float()
                else:
                    want = torch.tensor(mmd_oracle.sums(rows, n_a, pair_set, 1)[0].item()).float()
                assert got.item() == want.item(), (M, n_a, D, pair_set, median_set, got.item(), want.item())


def test_a_split_does_not_depend_on_the_launch_around_it(pools):
    M, n_a, D = 67, 3, 5
    dpool = pools[(M, n_a, D)].cuda()
    N = dpool.shape[0]
    full = launch(dpool, 37, M, n_a, 0, 1, seed=11)
    for s in (0, 17, 36):
        assert torch.equal(launch(dpool, 1, M, n_a, 0, 1, seed=11, split_offset=s)[0], full[s])
    # explicit indices from the Python restatement of the permutation give the same bits as idx == NULL
    idx = torch.tensor([mmd_oracle.split_rows(N, M, 11, s) for s in range(10)])
    assert torch.equal(idx, split_indices(N, M, 11, 10))
    assert torch.equal(launch(dpool, 10, M, n_a, 0, 1, idx=idx), full[:10])
    assert torch.equal(launch(dpool, 5, M, n_a, 0, 1, seed=11, split_offset=5), full[5:10])
    assert torch.equal(launch(dpool, 1, M, n_a, 0, 1, idx=idx[7:8]), full[7:8])


def test_given_bandwidth_and_floor(pools):
    M, n_a, D = 129, 64, 10
    pool = pools[(M, n_a, D)]
    idx = torch.arange(M).reshape(1, M).repeat(2, 1)
    bw = torch.tensor([0.8, 5.0])
    for pair_set in (0, 1):
        got = launch(pool.cuda(), 2, M, n_a, pair_set, 1, idx=idx, bandwidth=bw.cuda(), bw_floor=9.0).cpu()
        for s in range(2):
            want = mmd_oracle.sums(pool[:M], n_a, pair_set, 1, bandwidth=bw[s].item())
            assert got[s, 0].item() == bw[s].item()               # a given bandwidth is used as is: no floor
            for a, b in zip(combos(got[s], n_a, M - n_a, pair_set), combos(want, n_a, M - n_a, pair_set)):
                assert abs(a.item() - b.item()) <= MMD_ATOL
    # all rows equal: the median is 0; the floor takes effect and every term is exp(0) = 1
    same = torch.full((12, 3), 2.5).cuda()
    idx = torch.arange(12).reshape(1, 12)
    got = launch(same, 1, 12, 5, 1, 1, idx=idx, bw_floor=1e-8).cpu()[0]
    assert got.tolist() == [pytest.approx(1e-8, rel=1e-7), 10.0, 21.0, 35.0]
    # without a floor: bw == 0 and the formula's 0 * inf on every (zero) distance
    got = launch(same, 1, 12, 5, 0, 0, idx=idx).cpu()[0]
    assert got[0].item() == 0.0 and torch.isnan(got[1:]).all()


def test_nan_poisons_its_split_only(pools):
    M, n_a, D = 67, 3, 5
    pool = pools[(M, n_a, D)]
    N = pool.shape[0]
    idx = split_indices(N, M, 3, 6)
    clean = launch(pool.cuda(), 6, M, n_a, 1, 0, idx=idx)
    # a row only split 2 uses: give split 2 a private copy of one of its rows
    dirty = torch.cat((pool, pool[idx[2, 40]].reshape(1, D)))
    dirty[N, 1] = float("nan")
    idx2 = idx.clone()
    idx2[2, 40] = N
    got = launch(dirty.cuda(), 6, M, n_a, 1, 0, idx=idx2)
    assert torch.isnan(got[2]).all()
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(got[keep], clean[keep])
    # an index outside the pool is refused in the same way, without reading there
    idx3 = idx.clone()
    idx3[4, 0] = N + 5
    got = launch(pool.cuda(), 6, M, n_a, 1, 0, idx=idx3)
    assert torch.isnan(got[4]).all() and torch.equal(got[[0, 1, 2, 3, 5]], clean[[0, 1, 2, 3, 5]])


def test_past_the_lds_budget_is_unsupported_and_nothing_runs():
    lib = _lib.load()
    M, D = 1397, 10                                              # 1397 * 11 = 15 367 > 15 360
    assert M * (D | 1) > STAGE_FLOATS >= (M - 1) * (D | 1)
    pool = torch.randn(M, D).cuda()
    out = torch.full((1, 4), -7.0, device="cuda")
    rc = lib.sbi_amd_mmd_rbf_splits(_lib.ptr(pool), M, D, None, 0, 0, 1, M, 5, 0, 0, None, 0.0, _lib.ptr(out),
                                    _lib.current_stream(pool.device))
    assert rc == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    # the host route falls back instead of raising
    got = rbf_splits(pool, 1, M, 5, 0, 0, seed=1)
    want = rbf_splits(pool.cpu(), 1, M, 5, 0, 0, seed=1)
    assert got.is_cuda and torch.allclose(got.cpu(), want, rtol=1e-5)
