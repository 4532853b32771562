"""GPU parity of the MNLE kernels (csrc/mnle_kernel.h, mnle.hip, mnle_k*.hip) over the edges of their envelope and
over the workgroup widths: the configurations of tests/mnle_envelope.py that tests/test_mnle_gpu.py does not reach
(three distinct widths, num_bins = 5, a variable with one category, 3 and 4 spline-context layers, no residual block,
16 transforms, widths one past a 16-tile, every envelope minimum), row counts on 1, 2 and 4 waves per workgroup,
training passes over more than one split-K chunk of the weight-gradient kernel, condition rows shared by c[i % c_rows],
and the optional arguments of the training entry point.

Reference: the eager restatement (tests/mnle_oracle.py) in fp64, with the fp32 restatement supplying its own distance
from it.  Bounds (docstring of tests/mnle_envelope.py) are the project's and are not fitted to what the kernels give.
The fixed kernel-versus-fp32 bound of tests/test_mnle_gpu.py (1e-5 + 1e-5 max|ref|) is NOT applied here: on `deep` the
fp32 restatement itself sits 1.5e-4 from fp64 at max|ref| 14.8, which is the size of that bound.
The rows left out of a comparison are chosen from the references alone and capped in tests/test_mnle_envelope_cpu.py.
Every measured distance is recorded with tests/parity_log.py under mnle_envelope_*."""
import functools
import itertools

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.mixed_density_estimator import (mnle_log_prob_call, mnle_loss_fwd_bwd,
                                                                    mnle_packed_weights, mnle_sample_call,
                                                                    mnle_trials_call, split_input)
from tests.mnle_envelope import (CONFIGS, LARGE_CONFIGS, LARGE_ROWS, NEW_CONFIGS, POOL_ROWS, TRAINABLE_NEW,
                                 joint_reference, mnle_pair_cpu, pool, sample_draws, sample_reference, smooth_rows,
                                 training_distances, training_reference)
from tests.parity_log import record

pytestmark = pytest.mark.gpu

ROWS = [1, 17, 333]


def waves_of(n):
    """mnle_waves() of csrc/mnle.hip: the largest workgroup (4, 2, 1 waves of 16 rows) that still yields 256 of them."""
    nw = 4
    while nw > 1 and (n + 16 * nw - 1) // (16 * nw) < 256:
        nw >>= 1
    return nw


# last / first row counts of 1, 2 and 4 waves per workgroup
WAVE_ROWS = [8160, 8161, 16320, 16321]
assert WAVE_ROWS[1] >= 8161 and WAVE_ROWS[3] >= 16321 and max(WAVE_ROWS) <= LARGE_ROWS
assert [waves_of(n) for n in WAVE_ROWS] == [1, 2, 2, 4]
TRIALS = (7, 2332)
assert TRIALS[0] * TRIALS[1] >= 16321 and waves_of(TRIALS[0] * TRIALS[1]) == 4

# training rows: one row, a ragged wave, the last row of a 128-row sub-chunk and one past it, the last row of a 512-row
# split-K chunk and one past it (two chunks, the second with a single row)
TRAIN_ROWS = [1, 17, 128, 129, 333, 512, 513]
LARGE_TRAIN_ROWS = [8161, 16321]
assert 129 in TRAIN_ROWS and max(TRAIN_ROWS) >= 513
assert min(LARGE_TRAIN_ROWS) >= 8161 and max(LARGE_TRAIN_ROWS) >= 16321
assert [waves_of(n) for n in LARGE_TRAIN_ROWS] == [2, 4]
TRAIN_CASES = ([(name, n, False) for name in TRAINABLE_NEW for n in TRAIN_ROWS]
               + [(name, n, True) for name in LARGE_CONFIGS for n in LARGE_TRAIN_ROWS])


def pair(name, log_x=False):
    o32, o64, est, theta, x = mnle_pair_cpu(name, log_x)
    return o32, o64, est.cuda(), theta, x


def _errs(got, ref32, ref64):
    return (got.double().cpu() - ref64).abs().max().item(), (ref32.double() - ref64).abs().max().item()


def _dev_rows(net, x):
    return split_input(net, x.cuda())


def _tag(log_x):
    return "log" if log_x else "linear"


# ------------------------------------------------------------------ a. log_prob / parts / logits
@pytest.mark.parametrize("log_x", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(NEW_CONFIGS))
def test_log_prob_parts_and_logits_are_held_to_fp64(name, n, log_x):
    o32, o64, est, theta_d, x_d = pair(name, log_x)
    net = est.net
    cats = CONFIGS[name][0]
    theta = theta_d[:n].contiguous()
    z0, z1 = net.zstats[0].item(), net.zstats[1].item()
    stress = x_d[POOL_ROWS - n:].clone()
    zt = torch.where(torch.arange(n) % 2 == 0, torch.tensor(12.0), torch.tensor(-12.0))     # beyond +- tail_bound
    stress[:, 0] = torch.exp((zt - z0) / z1) if log_x else (zt - z0) / z1
    for what, x in (("in-distribution", x_d[:n].contiguous()), ("stress", stress)):
        with torch.no_grad():
            d32, c32 = o32.parts(x, theta)
            d64, c64 = o64.parts(x.double(), theta.double())
            lg32, lg64 = o32.logits(x, theta), o64.logits(x.double(), theta.double())
        xc, idx, val = _dev_rows(net, x)
        th = theta.cuda()
        joint, logits = mnle_log_prob_call(net, xc, idx, val, th, 3, want_logits=True)
        disc = mnle_log_prob_call(net, None, idx, None, th, 1)
        cont = mnle_log_prob_call(net, xc, None, val, th, 2)
        for part, got, r32, r64 in (("joint", joint, d32 + c32, d64 + c64), ("discrete", disc, d32, d64),
                                    ("continuous", cont, c32, c64)):
            e_hip, e_ref = _errs(got, r32, r64)
            print(f"{what} {part}: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} max|ref|={r64.abs().max():.1f}")
            record("mnle_envelope_log_prob", f"{name} n{n} {_tag(log_x)} {what} {part}", max_abs_hip_vs_f64=e_hip,
                   max_abs_oracle32_vs_f64=e_ref, max_abs_ref=r64.abs().max().item())
            assert torch.isfinite(got).all()
            assert e_hip <= 2.0 * e_ref + 1e-5, part
        logits = logits.cpu()
        fin = torch.isfinite(lg64)
        assert torch.equal(torch.isneginf(logits), ~fin)          # -inf exactly beyond num_categories[v]
        e_hip = (logits.double()[fin] - lg64[fin]).abs().max().item()
        e_ref = (lg32.double()[fin] - lg64[fin]).abs().max().item()
        print(f"{what} logits: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
        record("mnle_envelope_log_prob", f"{name} n{n} {_tag(log_x)} {what} logits", max_abs_hip_vs_f64=e_hip,
               max_abs_oracle32_vs_f64=e_ref, max_abs_ref=lg64[fin].abs().max().item())
        assert e_hip <= 2.0 * e_ref + 1e-5
        for v, c in enumerate(cats):
            if c == 1:          # one category: a finite logit (its softmax is 1), nothing else
                assert torch.isfinite(logits[:, v, 0]).all() and torch.isneginf(logits[:, v, 1:]).all()
        if max(cats) == 1:
            assert (disc == 0).all()          # log 1, exactly
        assert torch.equal(est.log_prob(x.cuda(), th).cpu(), joint.cpu()[None])


# ------------------------------------------------------------------ b. probabilities
def test_categorical_probabilities_sum_to_one_with_a_one_category_variable():
    _, _, est, theta_d, _ = pair("uneven")
    cats = CONFIGS["uneven"][0]
    combos = list(itertools.product(*[range(c) for c in cats]))
    assert len(combos) == 12
    m = 7
    idx = torch.tensor(combos, dtype=torch.int32).repeat(m, 1).cuda().contiguous()             # theta-major blocks
    th = theta_d[:m].repeat_interleave(len(combos), 0).cuda().contiguous()
    lp = mnle_log_prob_call(est.net, None, idx, None, th, 1).reshape(m, len(combos))
    total = lp.double().exp().sum(1).cpu()
    print("sum of probabilities:", total.tolist())
    assert (total - 1.0).abs().max() <= 1e-5


# ------------------------------------------------------------------ c. sample
def _check_sample(key, tag, n, log_x, idx, xc, ref):
    """Indices equal the fp64 restatement's on the kept rows; the continuous column is held to 2 e_ref + 1e-5 where
    both restatements drew the same categories."""
    u, noise, idx64, x64, idx32, x32, keep = (t[:n] for t in ref)
    left_out = int((~keep).sum())
    assert left_out <= n // 100
    idx, xc = idx.cpu(), xc.cpu()
    assert torch.equal(idx.long()[keep], idx64[keep])
    same = keep & (idx32 == idx64).all(1)
    assert same.any()
    ref32 = torch.log(x32[:, 0]) if log_x else x32[:, 0]
    ref64 = torch.log(x64[:, 0]) if log_x else x64[:, 0]
    got = torch.log(xc) if log_x else xc
    e_hip, e_ref = _errs(got[same], ref32[same], ref64[same])
    print(f"left out {left_out}; |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
    record(key, tag, left_out=left_out, max_abs_hip_vs_f64=e_hip, max_abs_oracle32_vs_f64=e_ref)
    assert torch.isfinite(xc).all() and e_hip <= 2.0 * e_ref + 1e-5
    return keep


@pytest.mark.parametrize("log_x", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("name", list(NEW_CONFIGS))
def test_sample_follows_the_inverse_cdf_and_the_inverse_flow(name, log_x):
    _, _, est, theta_d, _ = pair(name, log_x)
    cats = CONFIGS[name][0]
    n = POOL_ROWS
    ref = sample_reference(name, log_x)
    u, noise, x64 = ref[0], ref[1], ref[3]
    idx, xc = mnle_sample_call(est.net, u.cuda(), noise.cuda(), theta_d.cuda())
    keep = _check_sample("mnle_envelope_sample", f"{name} n{n} {_tag(log_x)}", n, log_x, idx, xc, ref)
    for v, c in enumerate(cats):
        if c == 1:
            assert (idx[:, v] == 0).all()
    full = est.sample_given(u.cuda(), noise.cuda(), theta_d.cuda()).cpu()
    assert torch.equal(full[:, 0], xc.cpu())
    assert torch.equal(full[keep][:, 1:].double(), x64[keep][:, 1:])            # raw values, not indices


# ------------------------------------------------------------------ d. wave counts
@functools.lru_cache(maxsize=None)
def _wave_launch(name, n):
    """(log_prob, sampled indices, sampled continuous column) of the first n rows of the large pool, on the CPU."""
    _, _, est, _, _ = pair(name, True)
    theta, x = pool(name, True, True)
    u, noise = sample_draws(LARGE_ROWS, len(CONFIGS[name][0]))
    xc, idx, val = _dev_rows(est.net, x[:n].contiguous())
    th = theta[:n].cuda().contiguous()
    logp = mnle_log_prob_call(est.net, xc, idx, val, th)
    sidx, sx = mnle_sample_call(est.net, u[:n].cuda().contiguous(), noise[:n].cuda().contiguous(), th)
    return logp.cpu(), sidx.cpu(), sx.cpu()


@pytest.mark.parametrize("n", WAVE_ROWS)
@pytest.mark.parametrize("name", LARGE_CONFIGS)
def test_log_prob_and_sample_on_one_two_and_four_waves(name, n):
    logp, sidx, sx = _wave_launch(name, n)
    r32, r64 = joint_reference(name, True, True)
    e_hip, e_ref = _errs(logp, r32[:n], r64[:n])
    print(f"{waves_of(n)} waves, log_prob: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
    record("mnle_envelope_waves_log_prob", f"{name} n{n}", waves=waves_of(n), max_abs_hip_vs_f64=e_hip,
           max_abs_oracle32_vs_f64=e_ref, max_abs_ref=r64[:n].abs().max().item())
    assert torch.isfinite(logp).all() and e_hip <= 2.0 * e_ref + 1e-5
    _check_sample("mnle_envelope_waves_sample", f"{name} n{n}", n, True, sidx, sx, sample_reference(name, True, True))
    # a row's value does not depend on the workgroup width: bit for bit the one-wave launch on the rows they share
    b_logp, b_sidx, b_sx = _wave_launch(name, WAVE_ROWS[0])
    m = min(n, WAVE_ROWS[0])
    assert torch.equal(logp[:m], b_logp[:m]) and torch.equal(sidx[:m], b_sidx[:m]) and torch.equal(sx[:m], b_sx[:m])


def test_trials_on_four_waves_are_bit_identical_to_the_paired_kernel_in_trial_order():
    T, N = TRIALS
    _, _, est, _, x_d = pair("uneven", True)
    net = est.net
    x_o = x_d[100: 100 + T].cuda().contiguous()
    theta = pool("uneven", True, True)[0][:N].cuda().contiguous()
    xc, idx, val = _dev_rows(net, x_o)
    got = mnle_trials_call(net, xc, idx, val, theta)
    acc = torch.zeros(N, dtype=torch.float32, device="cuda")
    for t in range(T):      # explicit fp32 loop over the paired kernel's pair outputs, trial order
        acc = acc + mnle_log_prob_call(net, xc[t: t + 1].expand(N).contiguous(), idx[t: t + 1].expand(N, -1).contiguous(),
                                       val[t: t + 1].expand(N, -1).contiguous(), theta)
    assert torch.isfinite(got).all() and torch.equal(got, acc)
    assert torch.equal(est.log_prob_iid_trials(x_o, theta), got)


# ------------------------------------------------------------------ e. training pass
def _train(net, x, theta, w, uniform=0.0, want_grad_cond=True):
    """One training pass on NaN-filled outputs and workspace: (losses, grad, d / d theta)."""
    n = x.shape[0]
    xc, idx, val = _dev_rows(net, x)
    grad = torch.full_like(net.flat_params.data, float("nan"))
    ws = torch.full((net.train_workspace_floats(n),), float("nan"), device="cuda")
    losses, gth = mnle_loss_fwd_bwd(net, xc, idx, val, theta, w, uniform, grad, want_grad_cond=want_grad_cond,
                                    workspace=ws)
    torch.cuda.synchronize()
    return losses, grad, gth


@pytest.mark.parametrize("name, n, large", TRAIN_CASES, ids=[f"{name}-{n}" for name, n, _ in TRAIN_CASES])
def test_training_pass_matches_fp64_autograd_and_is_deterministic(name, n, large):
    o32, o64, est, _, _ = pair(name, True)
    net = est.net
    theta_p, x_p = pool(name, True, large)
    rows, left_out = smooth_rows(name, large)
    print(f"rows left out of the pool for a ReLU branch that differs between fp32 and fp64: {left_out}")
    assert left_out <= theta_p.shape[0] // 100 and rows.numel() >= n
    theta, x = theta_p[rows[:n]].contiguous(), x_p[rows[:n]].contiguous()
    w = torch.linspace(0.5, 1.5, n) / n if n > 1 else torch.ones(1)
    loss_ref, gref, gth_ref = training_reference(o64, x, theta, w)
    loss32, g32, gth32 = training_reference(o32, x, theta, w)

    xg, tg, wg = x.cuda(), theta.cuda(), w.cuda()
    losses, grad, gth = _train(net, xg, tg, wg)
    assert torch.isfinite(grad).all() and torch.isfinite(gth).all() and torch.isfinite(losses).all()
    e_loss = (losses.cpu().double() - loss_ref).abs().max().item()
    o_loss = (loss32 - loss_ref).abs().max().item()
    rel, worst, worst_key, e_th = training_distances(net, grad, gth, gref, gth_ref)
    o_rel, o_worst, o_key, o_th = training_distances(net, g32, gth32, gref, gth_ref)
    print(f"loss err {e_loss:.3e} (fp32 restatement {o_loss:.3e}, max |ref| {loss_ref.abs().max():.2f})")
    print(f"grad rel {rel:.3e} worst block {worst:.3e} ({worst_key}) d/dtheta rel {e_th:.3e}")
    print(f"fp32 restatement: grad rel {o_rel:.3e} worst block {o_worst:.3e} ({o_key}) d/dtheta rel {o_th:.3e}")
    record("mnle_envelope_train", f"{name} n{n}", waves=waves_of(n), chunks=(n + 511) // 512,
           max_abs_loss_err_vs_f64=e_loss, max_abs_loss_err_oracle32_vs_f64=o_loss,
           max_abs_loss=loss_ref.abs().max().item(), grad_rel_err_vs_f64=rel, grad_rel_err_oracle32_vs_f64=o_rel,
           worst_block_rel_err_vs_f64=worst, worst_block=worst_key, worst_block_rel_err_oracle32_vs_f64=o_worst,
           grad_theta_rel_err_vs_f64=e_th, grad_theta_rel_err_oracle32_vs_f64=o_th)
    assert e_loss <= 1e-5 + 1e-5 * loss_ref.abs().max().item()
    assert worst <= 3e-4, f"{worst_key}: {worst:.3e}"
    assert rel <= 2e-4 and e_th <= 3e-4
    masked = o32.flat_mask() == 0
    assert masked.any() and (grad.cpu()[masked] == 0).all()          # masked weight entries: exactly zero
    l2, g2, t2 = _train(net, xg, tg, wg)
    assert torch.equal(grad, g2) and torch.equal(gth, t2) and torch.equal(losses, l2)


# ------------------------------------------------------------------ f. broadcast conditions, weights, optional outputs
@pytest.mark.parametrize("c_rows", [1, 7])
def test_shared_condition_rows_equal_the_paired_call(c_rows):
    n = 333
    _, _, est, theta_d, x_d = pair("uneven", True)
    net = est.net
    xc, idx, val = _dev_rows(net, x_d[:n].contiguous())
    short = theta_d[:c_rows].cuda().contiguous()
    full = theta_d[torch.arange(n) % c_rows].cuda().contiguous()
    for parts in (1, 2, 3):
        assert torch.equal(mnle_log_prob_call(net, xc, idx, val, short, parts),
                           mnle_log_prob_call(net, xc, idx, val, full, parts)), parts
    u, noise = sample_draws(n, len(CONFIGS["uneven"][0]))
    u, noise = u.cuda(), noise.cuda()
    i_s, x_s = mnle_sample_call(net, u, noise, short)
    i_f, x_f = mnle_sample_call(net, u, noise, full)
    assert torch.equal(i_s, i_f) and torch.equal(x_s, x_f) and torch.isfinite(x_s).all()


def test_training_pass_with_shared_condition_rows_and_a_uniform_weight():
    n, c_rows = 333, 7
    _, _, est, theta_d, x_d = pair("uneven", True)
    net = est.net
    x = x_d[:n].cuda().contiguous()
    short = theta_d[:c_rows].cuda().contiguous()
    full = theta_d[torch.arange(n) % c_rows].cuda().contiguous()
    w = (torch.linspace(0.5, 1.5, n) / n).cuda()
    l_f, g_f, _ = _train(net, x, full, w)
    l_s, g_s, none = _train(net, x, short, w, want_grad_cond=False)
    assert none is None and torch.isfinite(g_f).all()
    assert torch.equal(g_s, g_f) and torch.equal(l_s, l_f)
    # row_weight = NULL with a uniform weight against the same weight spelled out per row
    uw = 1.0 / n
    l_u, g_u, t_u = _train(net, x, full, None, uniform=uw)
    l_e, g_e, t_e = _train(net, x, full, torch.full((n,), uw, device="cuda"))
    assert torch.isfinite(g_u).all() and g_u.abs().max() > 0
    assert torch.equal(g_u, g_e) and torch.equal(l_u, l_e) and torch.equal(t_u, t_e)
    # loss_out = NULL, through the library: the same gradient
    lib = _lib.load()
    xc, idx, val = _dev_rows(net, x)
    packed = mnle_packed_weights(net)
    st = _lib.current_stream(full.device)
    cfg = net.hyper.c_config()
    grad = torch.full_like(net.flat_params.data, float("nan"))
    ws = torch.full((net.train_workspace_floats(n),), float("nan"), device="cuda")
    rc = lib.sbi_amd_mnle_loss_fwd_bwd(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                       _lib.ptr(val), _lib.ptr(full), n, n, _lib.ptr(w), 0.0, None, _lib.ptr(grad),
                                       None, _lib.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(grad, g_f)
    # d / d condition needs one condition row per data row: refused without a launch
    grad.zero_()
    gc = torch.zeros(c_rows, net.hyper.C, device="cuda")
    rc = lib.sbi_amd_mnle_loss_fwd_bwd(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                       _lib.ptr(val), _lib.ptr(short), n, c_rows, _lib.ptr(w), 0.0, None,
                                       _lib.ptr(grad), _lib.ptr(gc), _lib.ptr(ws), st)
    torch.cuda.synchronize()
    assert rc == _lib.E_BADARG and (grad == 0).all() and (gc == 0).all()
