"""csrc/sir.hip through the C ABI (include/sbi_amd_sir.h): the selection step of sampling-importance-resampling.

The reference's rule (sbi/samplers/importance/sir.py:59-63) is restated here in fp64 torch -- softmax over the
candidates, cumsum, first index whose cumulative weight is >= u -- and the kernel must pick the same candidate on every
row that is not within 1e-5 of a boundary in cumulative weight (the kernel works in fp32; on a boundary the pick is a
matter of rounding, and the kernel's two deliberate departures from the reference live exactly there)."""
import numpy as np
import pytest
import torch

from sbi_amd import _lib
from tests.mcmc_restatement import philox4x32_10, u01

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIR_TAG = 0x53495231


def run(log_p, log_q, cand, u=None, seed=0, row_offset=0, out=None, want_lse=True, want_dead=True):
    """One launch on device tensors; returns (out, idx, row_lse, n_dead) on the host."""
    lib = _lib.load()
    B, K = log_p.shape
    D = cand.shape[-1]
    log_p, cand = log_p.contiguous(), cand.contiguous()
    log_q = None if log_q is None else log_q.contiguous()
    if out is None:
        out = torch.full((B, D), float("nan"), device=DEV)
    idx = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((B,), 123.0, device=DEV) if want_lse else None
    dead = torch.zeros(1, dtype=torch.int32, device=DEV) if want_dead else None
    rc = lib.sbi_amd_sir_resample(_lib.ptr(log_p), _lib.ptr(log_q), _lib.ptr(cand), B, K, D, _lib.ptr(u), seed,
                                  row_offset, _lib.ptr(out), _lib.ptr(idx), _lib.ptr(lse), _lib.ptr(dead),
                                  _lib.current_stream(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), idx.cpu(), None if lse is None else lse.cpu(), None if dead is None else int(dead.item())


def fp64_rule(log_p, log_q, u):
    """(index of the first cumulative softmax weight >= u, the cumulative weights, logsumexp) in fp64 on the host."""
    lw = log_p.double() if log_q is None else log_p.double() - log_q.double()
    c = torch.softmax(lw, dim=-1).cumsum(dim=-1)
    hit = c >= u.double().unsqueeze(-1)
    idx = torch.where(hit.any(-1), torch.argmax(hit.to(torch.int8), dim=-1), torch.full((lw.shape[0],), -1))
    return idx, c, torch.logsumexp(lw, dim=-1)


KS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 129, 1000, 4097, 10_000, 20_000, 40_960]
DS = [1, 3, 16, 17, 65]


@pytest.mark.parametrize("K", KS)
def test_parity_with_the_fp64_rule(K):
    """B = 1, 2, 5 and 257 at this K (B = 4096 too up to K = 129), D cycling through {1, 3, 16, 17, 65}; the
    rows of all B together are the case whose left-out fraction is bounded.  The (K, B, D) grid is sampled, not
    crossed: D is assigned per (K, B) in rotation and falls back to 3 where the candidates would pass 30 M floats
    (D > 64 still meets both kernels: K = 64 and 65 at small B, K = 10 000 at B = 5).
    K = 20 000 and 40 960 are rows of more than 64 KiB, which need the raised dynamic-LDS
    limit, up to the largest row the kernel takes (exactly 160 KiB); B = 33 there instead of 257."""
    s = 3.0 if K <= 1000 else (10.0 if K == 4097 else 30.0)
    Bs = ([1, 2, 5, 257] if K <= 10_000 else [1, 2, 5, 33]) + ([4096] if K <= 129 else [])
    g = torch.Generator().manual_seed(1000 + K)
    rows = left_out = 0
    for j, B in enumerate(Bs):
        D = DS[(KS.index(K) + j) % len(DS)]
        if B * K * D > 30_000_000:          # (keep the candidates of the largest shapes small: D does not matter there)
            D = 3
        lw = torch.randn(B, K, generator=g) * s
        if K <= 129:          # a proposal term on a 1/4 grid: log_p - log_q stays within an ulp of the intended weight
            log_q = torch.round(torch.randn(B, K, generator=g) * 8) / 4
            log_p = lw + log_q
        else:
            log_q, log_p = None, lw
        cand = torch.randn(B, K, D, generator=g)
        u = torch.rand(B, generator=g)
        want, c64, lse64 = fp64_rule(log_p, log_q, u)
        keep = ((c64 - u.double().unsqueeze(-1)).abs() >= 1e-5).all(-1)
        rows += B
        left_out += int((~keep).sum())
        out, idx, lse, dead = run(log_p.to(DEV), None if log_q is None else log_q.to(DEV), cand.to(DEV), u.to(DEV))
        assert dead == 0
        assert ((idx >= 0) & (idx < K)).all()
        assert torch.equal(idx[keep].long(), want[keep]), (K, B, D)
        picked = cand[torch.arange(B), idx.long()]
        assert torch.equal(out[keep], picked[keep]), (K, B, D)       # bit for bit
        assert torch.equal(out, picked)                              # ... and the boundary rows copy what they picked
        err = (lse.double() - lse64).abs()
        assert (err <= 1e-5 * (1 + lse64.abs())).all(), (K, B, float(err.max()))
    print(f"K={K}: {left_out}/{rows} rows within 1e-5 of a boundary")
    assert left_out <= 0.02 * rows, (K, left_out, rows)


def test_dead_rows_and_zero_weights():
    inf = float("inf")
    for K in (7, 64, 200):
        g = torch.Generator().manual_seed(K)
        B, D = 12, 5
        log_p = torch.randn(B, K, generator=g)
        log_q = torch.randn(B, K, generator=g)
        log_p[1] = -inf                                  # all -inf
        log_p[3, K // 2] = float("nan")                  # one NaN
        log_p[5, K - 1] = inf                            # one +inf
        log_p[7, 2] = -inf
        log_q[7, 2] = -inf                               # -inf - -inf = NaN
        dead_rows = [1, 3, 5, 7]
        cand = torch.randn(B, K, D, generator=g)
        u = torch.rand(B, generator=g)
        sentinel = torch.full((B, D), -1234.5, device=DEV)
        out, idx, lse, dead = run(log_p.to(DEV), log_q.to(DEV), cand.to(DEV), u.to(DEV), out=sentinel)
        assert dead == len(dead_rows)
        live = torch.ones(B, dtype=torch.bool)
        live[dead_rows] = False
        assert (idx[dead_rows] == -1).all() and (idx[live] >= 0).all()
        assert (out[dead_rows] == -1234.5).all()                       # untouched
        # row_lse of a dead row: its maximum (-inf / +inf) without a NaN, NaN with one; live rows: logsumexp
        assert lse[1] == -inf and lse[5] == inf and torch.isnan(lse[3]) and torch.isnan(lse[7])
        want_lse = torch.logsumexp(log_p.double() - log_q.double(), -1)[live]
        assert ((lse[live].double() - want_lse).abs() <= 1e-5 * (1 + want_lse.abs())).all()
        assert torch.equal(out[live], cand[torch.arange(B), idx.long().clamp(min=0)][live])
        # without the optional outputs the launch is the same
        out2, idx2, _, _ = run(log_p.to(DEV), log_q.to(DEV), cand.to(DEV), u.to(DEV), want_lse=False, want_dead=False)
        assert torch.equal(idx2, idx)


def test_a_row_that_does_not_fit_the_lds_is_refused_not_degraded():
    lib = _lib.load()
    B, K, D = 2, 40_961, 1
    lp, cand = torch.zeros(B, K, device=DEV), torch.zeros(B, K, D, device=DEV)
    out, idx = torch.zeros(B, D, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    rc = lib.sbi_amd_sir_resample(_lib.ptr(lp), None, _lib.ptr(cand), B, K, D, None, 0, 0, _lib.ptr(out), _lib.ptr(idx),
                                  None, None, _lib.current_stream(torch.device(DEV)))
    assert rc == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (idx.cpu() == -7).all()                                      # nothing was launched
    from sbi_amd.samplers.importance import sir_select

    with pytest.raises(NotImplementedError, match="40960"):
        sir_select(lp, None, cand)


@pytest.mark.parametrize("K", [4, 33, 64, 65, 300])
def test_a_candidate_of_weight_zero_is_never_picked(K):
    inf = float("inf")
    g = torch.Generator().manual_seed(K)
    patterns = []
    for lead, tail in ((1, 0), (0, 1), (1, 1), (K - 1, 0), (0, K - 1), (K // 2, K - K // 2 - 1)):
        row = torch.randn(K, generator=g)
        row[:lead] = -inf
        if tail:
            row[K - tail:] = -inf
        patterns.append(row)
    sparse = torch.randn(K, generator=g)
    sparse[torch.rand(K, generator=g) < 0.7] = -inf
    sparse[K // 3] = 0.0
    patterns.append(sparse)
    us = [0.0, 1.0 - 2.0**-24, 0.5, 2.0**-24]
    log_p = torch.stack([p for p in patterns for _ in us])
    u = torch.tensor(us * len(patterns))
    B = log_p.shape[0]
    cand = torch.arange(B * K, dtype=torch.float32).reshape(B, K, 1)
    out, idx, lse, dead = run(log_p.to(DEV), None, cand.to(DEV), u.to(DEV))
    assert dead == 0 and (idx >= 0).all()
    assert torch.isfinite(log_p[torch.arange(B), idx.long()]).all()
    # u = 0 picks the first candidate of positive weight, u = 1 - 2^-24 the last one (these rows hold no tiny weights)
    finite = torch.isfinite(log_p)
    first = torch.argmax(finite.to(torch.int8), dim=-1)
    last = K - 1 - torch.argmax(finite.flip(-1).to(torch.int8), dim=-1)
    assert torch.equal(idx[0::4].long(), first[0::4])
    want, c64, _ = fp64_rule(log_p, None, u)
    away = ((c64 - u.double().unsqueeze(-1)).abs() >= 1e-5).all(-1)
    assert torch.equal(idx[away].long(), want[away])
    assert (idx[1::4].long() <= last[1::4]).all()


def test_one_candidate_and_a_missing_proposal_term():
    g = torch.Generator().manual_seed(3)
    lp1 = torch.randn(300, 1, generator=g) * 50
    cand1 = torch.randn(300, 1, 4, generator=g)
    out, idx, lse, dead = run(lp1.to(DEV), None, cand1.to(DEV), torch.rand(300, generator=g).to(DEV))
    assert (idx == 0).all() and dead == 0 and torch.equal(out, cand1[:, 0]) and torch.equal(lse, lp1[:, 0])
    for K in (6, 64, 150):
        lp = torch.randn(40, K, generator=g) * 3
        cand = torch.randn(40, K, 3, generator=g)
        u = torch.rand(40, generator=g)
        a = run(lp.to(DEV), None, cand.to(DEV), u.to(DEV))
        b = run(lp.to(DEV), torch.zeros(40, K, device=DEV), cand.to(DEV), u.to(DEV))
        assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("K", [5, 32, 100])
def test_position_independence_and_repeatability(K):
    g = torch.Generator().manual_seed(50 + K)
    n, D, B = 7, 6, 257
    lp7, lq7 = torch.randn(n, K, generator=g) * 3, torch.randn(n, K, generator=g)
    lp7[2, 0] = -float("inf")
    cand7, u7 = torch.randn(n, K, D, generator=g), torch.rand(n, generator=g)
    alone = run(lp7.to(DEV), lq7.to(DEV), cand7.to(DEV), u7.to(DEV))
    again = run(lp7.to(DEV), lq7.to(DEV), cand7.to(DEV), u7.to(DEV))
    for a, b in zip(alone[:3], again[:3]):
        assert torch.equal(a, b)
    for where in (torch.arange(n), torch.arange(n) + 3, torch.arange(n) + B - n,
                  torch.tensor([0, 1, 63, 64, 130, 255, 256]), torch.tensor([256, 12, 51, 50, 200, 13, 128])):
        lp, lq = torch.randn(B, K, generator=g) * 3, torch.randn(B, K, generator=g)
        cand, u = torch.randn(B, K, D, generator=g), torch.rand(B, generator=g)
        lp[where], lq[where], cand[where], u[where] = lp7, lq7, cand7, u7
        out, idx, lse, _ = run(lp.to(DEV), lq.to(DEV), cand.to(DEV), u.to(DEV))
        assert torch.equal(idx[where], alone[1])
        assert torch.equal(lse[where].view(torch.int32), alone[2].view(torch.int32))      # bit for bit
        assert torch.equal(out[where], alone[0])


def host_uniforms(seed, row0, n):
    row = np.arange(n, dtype=np.uint64) + np.uint64(row0)
    words = philox4x32_10((row & np.uint64(0xFFFFFFFF), row >> np.uint64(32), 0, SIR_TAG),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return torch.from_numpy(np.asarray(u01(words[0]), dtype=np.float32))


@pytest.mark.parametrize("K", [8, 64, 200])
def test_in_kernel_uniforms_are_the_documented_philox_stream(K):
    g = torch.Generator().manual_seed(K)
    B, D = 500, 2
    seed = (0x1234ABCD << 32) | 0x9E3779B9
    lp = (torch.randn(B, K, generator=g) * 2).to(DEV)
    cand = torch.randn(B, K, D, generator=g).to(DEV)
    for off in (0, 77, (1 << 32) - 100):                 # the last one crosses into the high counter word
        inside = run(lp, None, cand, None, seed, off)
        given = run(lp, None, cand, host_uniforms(seed, off, B).to(DEV))
        assert torch.equal(inside[1], given[1]) and torch.equal(inside[0], given[0])
    # row_offset = a on rows [0, n) is rows [a, a + n) of a run at offset 0 (same inputs on those rows)
    a, n = 123, 200
    whole = run(lp, None, cand, None, seed, 0)
    part = run(lp[a:a + n].contiguous(), None, cand[a:a + n].contiguous(), None, seed, a)
    assert torch.equal(part[1], whole[1][a:a + n])
    other = run(lp, None, cand, None, seed + 1, 0)
    assert not torch.equal(other[1], whole[1])


def test_selection_frequencies_follow_the_weights():
    B, K = 200_000, 8
    lw = torch.tensor([0.3, -1.2, 2.0, -float("inf"), 0.0, 1.1, -3.0, 0.7])
    p = torch.softmax(lw.double(), dim=0)
    lp = lw.repeat(B, 1).to(DEV)
    cand = torch.arange(K, dtype=torch.float32).repeat(B, 1).unsqueeze(-1).to(DEV)
    out, idx, _, dead = run(lp, None, cand, None, seed=20_240_607)
    assert dead == 0
    freq = torch.bincount(idx.long(), minlength=K).double() / B
    bound = 5 * torch.sqrt(p * (1 - p) / B)
    print("frequencies", freq.tolist(), "softmax", p.tolist())
    assert ((freq - p).abs() <= bound).all(), (freq - p).abs() / bound.clamp(min=1e-300)
    assert freq[3] == 0
