"""GPU parity of the mixture-density-network kernels (csrc/mdn_kernel.h, mdn.hip) over the edges of their envelope and
over every path of the host side's plan that tests/test_mdn_gpu.py does not reach: the configurations of
tests/mdn_envelope.py (every maximum, every minimum, both sides of the 13 / 16 K-step switch, H = 1, K = 1, C = 63 / 64,
D = 4 against 5, head widths on and one past a 16-column gradient plane), row counts on 1, 2 and 4 waves per workgroup,
training passes over one, two and three split-K chunks of the weight-gradient kernel, condition rows shared by
x[i % x_rows] with 1 < x_rows < n and x_rows > n, the second trip of the looping one-observation kernels, softplus above
its threshold of 20, the ends of the component selection, and log_prob far in the tail.

Reference: the eager restatement (tests/mdn_oracle.py) in fp64 on identical weights, evaluated in row chunks, with the
fp32 restatement supplying its own distance from it.  Bounds (docstring of tests/mdn_envelope.py) are the project's and
are not fitted to what the kernels give.  Rows left out of a sample-by-u comparison are chosen from the fp64 restatement
alone; their cap and every other condition on the references is checked in tests/test_mdn_envelope_cpu.py as well.
Every measured distance is recorded with tests/parity_log.py under mdn_envelope_*."""
import pytest
import torch

from sbi_amd.neural_nets.estimators.mdn import (mdn_components_call, mdn_log_prob_call, mdn_loss_fwd_bwd,
                                                mdn_sample_call)
from tests.mdn_envelope import (BCAST_CONFIGS, BCAST_LOG_PROB_ROWS, BCAST_SAMPLE_ROWS, CHUNK_CONFIGS, CHUNK_ROWS,
                                CONFIGS, NEW_CONFIGS, POOL_ROWS, ROWS, SELECT_CONFIGS, SOFTPLUS_CONFIGS,
                                SOFTPLUS_SHIFT, WAVE_CONFIGS, WAVE_ROWS, XROWS_CASES, bcast_grid_and_trips,
                                bcast_subset, errs, large_pool, mdn_pair_gpu, nchunks, ref_components, ref_log_prob,
                                ref_pick, ref_sample, row_chunks, sample_draws, softplus_fraction, softplus_theta,
                                training_distances, training_reference, training_weights, waves)
from tests.parity_log import record

pytestmark = pytest.mark.gpu

assert [waves(CONFIGS[c], n) for c in WAVE_CONFIGS for n in WAVE_ROWS] == [1, 2, 2, 4] * len(WAVE_CONFIGS)
assert waves(CONFIGS["corner"], 16321) == 4
assert [nchunks(n) for n in CHUNK_ROWS] == [1, 1, 1, 2, 3]
assert bcast_grid_and_trips(BCAST_LOG_PROB_ROWS, False) == (512, 2)
assert bcast_grid_and_trips(BCAST_SAMPLE_ROWS, True) == (512, 2)

WAVE_CASES = [(name, n) for name in WAVE_CONFIGS for n in WAVE_ROWS] + [("corner", 16321)]


def _x(one_x):
    return "one_x" if one_x else "paired"


def _dev(t):
    return t.cuda().contiguous()


# ------------------------------------------------------------------ shared comparisons (test_mdn_gpu.py's assertions)
def _held_to_fp64(rec, what, got, r32, r64):
    e_hip, e_ref = errs(got, r32, r64)
    rec[what + "_hip_vs_f64"], rec[what + "_o32_vs_f64"] = e_hip, e_ref
    print(f"{what}: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} max|ref|={r64.abs().max():.1f}")
    assert torch.isfinite(got).all(), what
    assert e_hip <= 2.0 * e_ref + 1e-5, what


def _components(rec, pair, x):
    """Mixture components of the condition rows x, compared chunk by chunk (the factors are n x K x (D + U))."""
    o32, o64, est = pair[:3]
    got = mdn_components_call(est.net, _dev(x))
    worst = {}
    for s, e in row_chunks(x.shape[0]):
        r32, r64 = ref_components(o32, x[s:e]), ref_components(o64, x[s:e])
        for name, g, a, b in zip(("logits", "means", "factors"), got, r32, r64):
            assert torch.isfinite(g[s:e]).all(), name
            e_hip, e_ref = errs(g[s:e], a, b)
            worst[name] = (max(worst.get(name, (0.0, 0.0))[0], e_hip), max(worst.get(name, (0.0, 0.0))[1], e_ref))
    for name, (e_hip, e_ref) in worst.items():
        rec[name + "_hip_vs_f64"], rec[name + "_o32_vs_f64"] = e_hip, e_ref
        print(f"{name}: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
        assert e_hip <= 2.0 * e_ref + 1e-5, name


def _log_prob(rec, what, pair, theta, x, x_dev=None, near_fp32=False):
    """log_prob of (theta, x) against both restatements; `x_dev`: the condition rows handed to the kernel when they are
    not the reference's (x[i % x_rows])."""
    o32, o64, est = pair[:3]
    r32, r64 = ref_log_prob(o32, theta, x), ref_log_prob(o64, theta, x)
    got = mdn_log_prob_call(est.net, _dev(theta), _dev(x if x_dev is None else x_dev)).cpu()
    rec[what + "_max_abs_ref"] = r64.abs().max().item()
    _held_to_fp64(rec, what, got, r32, r64)
    if near_fp32:
        rec[what + "_hip_vs_o32"] = (got - r32).abs().max().item()
        assert (got - r32).abs().max() <= 1e-5 + 1e-5 * r32.abs().max(), what
    return got


def _sample_comp(rec, pair, comp, zeta, x, x_dev=None):
    o32, o64, est = pair[:3]
    r32, r64 = ref_sample(o32, comp, zeta, x), ref_sample(o64, comp, zeta, x)
    got = mdn_sample_call(est.net, _dev(zeta), _dev(x if x_dev is None else x_dev), comp=_dev(comp.to(torch.int32)))
    _held_to_fp64(rec, "sample", got, r32, r64)
    return got


def _sample_u(rec, pair, u, zeta, x, x_dev=None, rows=None):
    """sample with the component picked from u: the fp64 restatement's pick, rows on a cumulative boundary left out
    (at most 1 %); `rows`: compare this subset only."""
    o32, o64, est = pair[:3]
    got = mdn_sample_call(est.net, _dev(zeta), _dev(x if x_dev is None else x_dev), u=_dev(u))
    if rows is not None:
        got, u, zeta, x = got[rows.cuda()], u[rows], zeta[rows], (x if x.shape[0] == 1 else x[rows])
    comp, keep = ref_pick(o64, u, x)
    left_out = int((~keep).sum())
    rec["sample_u_left_out"] = left_out
    assert left_out <= u.shape[0] // 100
    if int(keep.sum()) == 0:
        return
    r32, r64 = ref_sample(o32, comp, zeta, x), ref_sample(o64, comp, zeta, x)
    _held_to_fp64(rec, "sample_u", got[keep.cuda()], r32[keep], r64[keep])


def _train_run(net, theta, x, w, uniform):
    n = theta.shape[0]
    grad = torch.full_like(net.flat_params.data, float("nan"))
    ws = torch.full((net.train_workspace_floats(n),), float("nan"), device="cuda")
    losses, gth = mdn_loss_fwd_bwd(net, theta, x, w, uniform, grad, want_grad_theta=True, workspace=ws)
    torch.cuda.synchronize()
    return losses, grad, gth


def _training(group, tag, pair, theta, x, w, x_dev=None, uniform=0.0, offset=True):
    """The training pass on a NaN-filled gradient buffer and a NaN-filled workspace of exactly
    train_workspace_floats(n) floats against fp64 autograd of sum_i w_i loss_i; a second call and (offset) the same
    rows as the tail of longer buffers give the same bits.  w = None: `uniform` for every row."""
    o32, o64, est = pair[:3]
    net, n, D = est.net, theta.shape[0], theta.shape[1]
    w_ref = torch.full((n,), uniform) if w is None else w
    loss_ref, gref, gth_ref = training_reference(o64, theta, x, w_ref)
    _, g32, gth32 = training_reference(o32, theta, x, w_ref)
    o32_rel = (g32 - gref).abs().max().item() / gref.abs().max().item()
    o32_th = (gth32 - gth_ref).abs().max().item() / gth_ref.abs().max().item()
    tc, xc = _dev(theta), _dev(x if x_dev is None else x_dev)
    wc = None if w is None else _dev(w)
    losses, grad, gth = _train_run(net, tc, xc, wc, uniform)
    assert torch.isfinite(grad).all() and torch.isfinite(gth).all() and torch.isfinite(losses).all()
    e_loss = (losses.cpu().double() - loss_ref).abs().max().item()
    rel, worst, worst_key, e_th = training_distances(net, grad, gth, gref, gth_ref)
    record(group, tag, max_abs_loss_err=e_loss, max_abs_loss_ref=loss_ref.abs().max().item(), rel_grad_err_vs_f64=rel,
           worst_block_rel_err=worst, worst_block=worst_key, rel_grad_theta_err=e_th, o32_rel_grad_err_vs_f64=o32_rel,
           o32_rel_grad_theta_err=o32_th)
    print(f"loss {e_loss:.3e} (max|ref| {loss_ref.abs().max():.1f}) grad rel {rel:.3e} worst block {worst:.3e} "
          f"({worst_key}) d/dtheta rel {e_th:.3e}; fp32 restatement: grad rel {o32_rel:.3e} d/dtheta rel {o32_th:.3e}")
    assert e_loss <= 1e-5 + 1e-5 * loss_ref.abs().max().item()
    assert worst <= 3e-4, worst_key
    assert rel <= 2e-4 and e_th <= 3e-4
    l2, g2, t2 = _train_run(net, tc, xc, wc, uniform)
    assert torch.equal(grad, g2) and torch.equal(gth, t2) and torch.equal(losses, l2)
    if offset:
        k = n + 3
        big_t = torch.cat([torch.randn(k, D, device="cuda"), tc]).contiguous()
        big_w = None if wc is None else torch.cat([torch.rand(k, device="cuda"), wc]).contiguous()
        big_x = xc if xc.shape[0] != n else torch.cat([torch.randn(k, xc.shape[1], device="cuda"), xc]).contiguous()
        l3, g3, t3 = _train_run(net, big_t[k:], big_x if xc.shape[0] != n else big_x[k:],
                                None if wc is None else big_w[k:], uniform)
        assert torch.equal(grad, g3) and torch.equal(gth, t3) and torch.equal(losses, l3)
    return losses, grad, gth


def _forward_entry_points(group, tag, pair, theta, stress, x, est_loss=False, near_fp32=True):
    """components, log_prob (in-distribution and stress rows), sample for given components, sample by u.
    `near_fp32`: (theta, x) are rows of the distribution the estimator was standardised on, where log_prob also stays
    within 1e-5 + 1e-5 max|ref| of the fp32 restatement."""
    n, (D, K) = theta.shape[0], (pair[0].D, pair[0].K)
    rec = {}
    try:
        _components(rec, pair, x)
        got = _log_prob(rec, "in-distribution", pair, theta, x, near_fp32=near_fp32)
        if est_loss:          # loss = -log_prob through the estimator surface, (B,) without a sample dimension
            loss = pair[2].loss(_dev(theta), _dev(x)).cpu()
            assert loss.shape == (n,) and torch.equal(loss, -got)
        _log_prob(rec, "stress", pair, stress, x)
        comp, zeta, u = sample_draws(n, D, K)
        _sample_comp(rec, pair, comp, zeta, x)
        _sample_u(rec, pair, u, zeta, x)
    finally:
        record(group, tag, **rec)


# ------------------------------------------------------------------ 1. envelope edges, one wave
@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", NEW_CONFIGS)
def test_envelope_edges_forward_entry_points(name, n, one_x):
    pair = mdn_pair_gpu(*CONFIGS[name])
    theta_d, x_d = pair[3:]
    x = x_d[:1] if one_x else x_d[:n]
    _forward_entry_points("mdn_envelope_edges", f"{name} n{n} {_x(one_x)}", pair, theta_d[:n],
                          3.0 * theta_d[POOL_ROWS - n:], x, est_loss=not one_x)


@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", NEW_CONFIGS)
def test_envelope_edges_training_pass(name, n, one_x):
    pair = mdn_pair_gpu(*CONFIGS[name])
    theta_d, x_d = pair[3:]
    w = torch.linspace(0.5, 1.5, n) / n if n > 1 else torch.ones(1)
    _training("mdn_envelope_edges_train", f"{name} n{n} {_x(one_x)}", pair, theta_d[:n],
              x_d[:1] if one_x else x_d[:n], w)


# ------------------------------------------------------------------ 2. wave counts
@pytest.mark.parametrize("name, n", WAVE_CASES, ids=[f"{c}-n{n}" for c, n in WAVE_CASES])
def test_wave_counts_forward_entry_points(name, n):
    """1, 2 and 4 waves per workgroup of the paired kernels (the wrappers raise unless the launch returns 0: at the
    corner that is the 4-wave launch with ~150 KiB of LDS).  With C = D the large pool is the distribution of the
    estimator's own pool (x = theta + noise); at the corner its mixing matrix is another draw, so the rows are not
    in-distribution and only the fp64 rule applies."""
    D, C = CONFIGS[name][:2]
    pair = mdn_pair_gpu(*CONFIGS[name])
    theta, x = large_pool(name, n)
    _forward_entry_points("mdn_envelope_waves", f"{name} n{n} waves{waves(CONFIGS[name], n)}", pair, theta,
                          3.0 * theta.flip(0), x, est_loss=True, near_fp32=C == D)


@pytest.mark.parametrize("name, n", WAVE_CASES, ids=[f"{c}-n{n}" for c, n in WAVE_CASES])
def test_wave_counts_training_pass(name, n):
    """Non-uniform row weights with exact zeros; 16 and 32 partial-gradient slabs."""
    pair = mdn_pair_gpu(*CONFIGS[name])
    theta, x = large_pool(name, n)
    _training("mdn_envelope_waves_train", f"{name} n{n} waves{waves(CONFIGS[name], n)}", pair, theta, x,
              training_weights(n))


def test_wave_counts_training_pass_with_a_uniform_weight():
    """row_weight = NULL: every row weighs `uniform_weight`."""
    n = 8161
    pair = mdn_pair_gpu(*CONFIGS["defaults"])
    theta, x = large_pool("defaults", n)
    _training("mdn_envelope_waves_train", f"defaults n{n} uniform", pair, theta, x, None, uniform=1.0 / n)


# ------------------------------------------------------------------ 3. chunk edges of the weight gradient
@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("n", CHUNK_ROWS)
@pytest.mark.parametrize("name", CHUNK_CONFIGS)
def test_weight_gradient_chunk_edges(name, n, one_x):
    pair = mdn_pair_gpu(*CONFIGS[name])
    theta, x = large_pool(name, max(CHUNK_ROWS))
    _training("mdn_envelope_chunks", f"{name} n{n} chunks{nchunks(n)} {_x(one_x)}", pair, theta[:n],
              x[:1] if one_x else x[:n], training_weights(n))


# ------------------------------------------------------------------ 4. x_rows modulo
@pytest.mark.parametrize("n, x_rows", XROWS_CASES, ids=[f"n{n}-x{r}" for n, r in XROWS_CASES])
@pytest.mark.parametrize("name", ["defaults", "ksh16"])
def test_condition_rows_are_taken_modulo_x_rows(name, n, x_rows):
    pair = mdn_pair_gpu(*CONFIGS[name])
    net = pair[2].net
    D, C, H, K = CONFIGS[name]
    theta_d, x_d = pair[3:]
    theta, xs = theta_d[:n], x_d[:x_rows]
    xm = xs[torch.arange(n) % x_rows]                  # the rows the ABI promises
    tag = f"{name} n{n} x_rows{x_rows}"
    comp, zeta, u = sample_draws(n, D, K)
    rec = {}
    try:
        got = _log_prob(rec, "log_prob", pair, theta, xm, x_dev=xs)
        assert torch.equal(got, mdn_log_prob_call(net, _dev(theta), _dev(xm)).cpu())
        got = _sample_comp(rec, pair, comp, zeta, xm, x_dev=xs)
        assert torch.equal(got, mdn_sample_call(net, _dev(zeta), _dev(xm), comp=_dev(comp.to(torch.int32))))
        _sample_u(rec, pair, u, zeta, xm, x_dev=xs)
        assert torch.equal(mdn_sample_call(net, _dev(zeta), _dev(xs), u=_dev(u)),
                           mdn_sample_call(net, _dev(zeta), _dev(xm), u=_dev(u)))
    finally:
        record("mdn_envelope_x_rows", tag, **rec)
    w = training_weights(n)
    losses, grad, gth = _training("mdn_envelope_x_rows_train", tag, pair, theta, xm, w, x_dev=xs, offset=False)
    l2, g2, t2 = _train_run(net, _dev(theta), _dev(xm), _dev(w), 0.0)
    assert torch.equal(grad, g2) and torch.equal(gth, t2) and torch.equal(losses, l2)


# ------------------------------------------------------------------ 5. broadcast loop
@pytest.mark.parametrize("name", BCAST_CONFIGS)
def test_one_observation_log_prob_on_the_second_trip(name):
    n = BCAST_LOG_PROB_ROWS
    pair = mdn_pair_gpu(*CONFIGS[name])
    net = pair[2].net
    theta = large_pool(name, n)[0]
    x1 = pair[4][7:8]
    got = mdn_log_prob_call(net, _dev(theta), _dev(x1))
    assert torch.equal(got, mdn_log_prob_call(net, _dev(theta), _dev(x1.expand(n, -1))))
    rows = bcast_subset(n, False)
    r32, r64 = ref_log_prob(pair[0], theta[rows], x1), ref_log_prob(pair[1], theta[rows], x1)
    rec = {"log_prob_max_abs_ref": r64.abs().max().item()}
    try:
        _held_to_fp64(rec, "log_prob", got[rows.cuda()], r32, r64)
    finally:
        record("mdn_envelope_bcast", f"{name} log_prob n{n}", **rec)


@pytest.mark.parametrize("name", BCAST_CONFIGS)
def test_one_observation_sample_on_the_second_trip(name):
    n = BCAST_SAMPLE_ROWS
    pair = mdn_pair_gpu(*CONFIGS[name])
    net = pair[2].net
    D, C, H, K = CONFIGS[name]
    x1 = pair[4][7:8]
    xr = _dev(x1.expand(n, -1))
    comp, zeta, u = sample_draws(n, D, K)
    zc, uc, cc = _dev(zeta), _dev(u), _dev(comp.to(torch.int32))
    by_comp = mdn_sample_call(net, zc, _dev(x1), comp=cc)
    assert torch.equal(by_comp, mdn_sample_call(net, zc, xr, comp=cc))
    assert torch.equal(mdn_sample_call(net, zc, _dev(x1), u=uc), mdn_sample_call(net, zc, xr, u=uc))
    rows = bcast_subset(n, True)
    rec = {}
    try:
        r32, r64 = ref_sample(pair[0], comp[rows], zeta[rows], x1), ref_sample(pair[1], comp[rows], zeta[rows], x1)
        _held_to_fp64(rec, "sample", by_comp[rows.cuda()], r32, r64)
        _sample_u(rec, pair, u, zeta, x1, rows=rows)
    finally:
        record("mdn_envelope_bcast", f"{name} sample n{n}", **rec)


# ------------------------------------------------------------------ 6. softplus above its threshold
@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("name", list(SOFTPLUS_CONFIGS))
def test_softplus_above_its_threshold(name, one_x):
    """A constant on the raw-diagonal bias of the odd components puts 20 % - 80 % of their raw diagonal entries above
    20 (asserted from the fp64 restatement alone): the forward is softplus's identity branch, the backward `sg = 1`.
    The rows are the pool's own and rows drawn from the mixture itself, on which the shifted components carry weight
    (tests/test_mdn_envelope_cpu.py: their gradient is a visible part of the reference gradient)."""
    n = 333
    frac = softplus_fraction(name)
    assert 0.2 <= frac <= 0.8
    pair = mdn_pair_gpu(*SOFTPLUS_CONFIGS[name], diag_shift=SOFTPLUS_SHIFT)
    D, C, H, K = SOFTPLUS_CONFIGS[name]
    theta_d, x_d = pair[3:]
    x = x_d[:1] if one_x else x_d[:n]
    own = softplus_theta(name, n, one_x)
    tag = f"{name} n{n} {_x(one_x)}"
    rec = {"share_above_20": frac}
    try:
        _components(rec, pair, x)
        _log_prob(rec, "pool", pair, theta_d[:n], x)
        _log_prob(rec, "own", pair, own, x)
        comp, zeta, u = sample_draws(n, D, K)
        _sample_comp(rec, pair, torch.arange(n) % K, zeta, x)
        _sample_u(rec, pair, u, zeta, x)
    finally:
        record("mdn_envelope_softplus", tag, **rec)
    _training("mdn_envelope_softplus_train", tag, pair, own, x, training_weights(n))


# ------------------------------------------------------------------ 7. selection ends
@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("name", SELECT_CONFIGS)
def test_selection_ends(name, one_x):
    """An out-of-range `comp` is clamped to [0, K - 1]; u = 0 picks component 0, and u just below 1, u = 1 and u > 1
    pick the last one (no weight of these mixtures is within 1e-3 of 0: tests/test_mdn_envelope_cpu.py)."""
    n = 81                                         # 6 row tiles of the paired kernel, 2 row groups of the sampler
    pair = mdn_pair_gpu(*CONFIGS[name])
    net = pair[2].net
    D, C, H, K = CONFIGS[name]
    x = _dev(pair[4][:1] if one_x else pair[4][:n])
    zeta = sample_draws(n, D, K)[1]
    zc = _dev(zeta)

    def by_comp(v):
        return mdn_sample_call(net, zc, x, comp=torch.full((n,), v, dtype=torch.int32, device="cuda"))

    def by_u(v):
        return mdn_sample_call(net, zc, x, u=torch.full((n,), v, dtype=torch.float32, device="cuda"))

    first, last = by_comp(0), by_comp(K - 1)
    rec = {}
    try:
        for which, comp in (("first", 0), ("last", K - 1)):
            c = torch.full((n,), comp)
            _held_to_fp64(rec, which, first if comp == 0 else last, ref_sample(pair[0], c, zeta, pair[4][:x.shape[0]]),
                          ref_sample(pair[1], c, zeta, pair[4][:x.shape[0]]))
    finally:
        record("mdn_envelope_selection", f"{name} {_x(one_x)}", **rec)
    for v in (-1, -2**31):
        assert torch.equal(by_comp(v), first), v
    for v in (K, K + 3, 2**31 - 1):
        assert torch.equal(by_comp(v), last), v
    assert torch.equal(by_u(0.0), first)
    below_one = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)).item()
    assert below_one < 1.0
    for v in (below_one, 1.0, 1.5):
        assert torch.equal(by_u(v), last), v


# ------------------------------------------------------------------ 8. far tail
@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("name", NEW_CONFIGS + ["defaults"])
def test_log_prob_far_in_the_tail(name, one_x):
    """log_prob at 10 theta: |log p| of 600 - 2400, the online log-sum-exp with every term far below zero."""
    n = 333
    pair = mdn_pair_gpu(*CONFIGS[name])
    theta_d, x_d = pair[3:]
    rec = {}
    try:
        _log_prob(rec, "far_tail", pair, 10.0 * theta_d[:n], x_d[:1] if one_x else x_d[:n])
    finally:
        record("mdn_envelope_far_tail", f"{name} n{n} {_x(one_x)}", **rec)
