"""GPU parity of the L-C2ST classifier-ensemble kernels (csrc/lc2st_kernel.h) through the C ABI against the eager-torch
restatement tests/lc2st_oracle.py on identical row lists, initial weights and epoch orders; determinism and
independence of the members; the early-stopping bookkeeping; LC2ST / LC2ST_NF end to end on the linear Gaussian.

Shapes (D, Dx, H): the reference's default widths 10 D up to D = 10, and two wide ones, F = 64 with H = 120 and H = 128
with F = 7.  B = 200: 540 training rows give batches of 200 / 200 / 140 (the last one 4 chunks of 32 + 12 rows), one
member has exactly one full batch, one has 37 < B rows; validation sets of 60, 33 and 1 rows straddle the 32-row chunk.
The edges of the 16-wide tiles (F, H and D around a tile, the corner F = 64 with H = 128), the other batch sizes and
chunk counts, and evaluations of more than one 512-row block are in tests/test_lc2st_envelope_gpu.py."""
import numpy as np
import pytest
import torch

from sbi_amd.diagnostics import LC2ST, LC2ST_NF, LC2STState
from sbi_amd.diagnostics import lc2st as L
from tests import lc2st_oracle as O
from tests.parity_log import record

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 10), (2, 3, 20), (5, 5, 50), (10, 10, 100), (12, 52, 120), (3, 4, 128)]
SEED = 20240917
_CASES = {}


def _ids(s):
    return "D%d-Dx%d-H%d" % s


def make_members(R, sizes, F, rng, data):
    """Hand-made members over a shared matrix: member 0 learnable from column 0, member 1 with coin-flip labels, the rest
    learnable from the last column; row lists are random subsets (with their own order) of the R rows."""
    M = len(sizes)
    stride = max(nt + nv for nt, nv in sizes)
    rows = np.zeros((M, stride), np.int32)
    labels = np.zeros((M, stride), np.float32)
    for m, (nt, nv) in enumerate(sizes):
        idx = rng.permutation(R)[: nt + nv]
        rows[m, : nt + nv] = idx
        col = data[idx, 0 if m == 0 else F - 1].numpy()
        labels[m, : nt + nv] = rng.integers(0, 2, nt + nv) if m == 1 else (col + 0.5 * rng.standard_normal(nt + nv) > 0)
    ids = np.array([7, 3, 11, 0, 40][:M], np.int32)          # ids are not slots
    return L.Members(rows, labels, np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32),
                     ids, np.arange(M, dtype=np.int64) + 100)


def case(shape, **hyper_kw):
    """One shared case per shape: hyper-parameters, data, members, initial weights (computed once, never modified)."""
    key = (shape, tuple(sorted(hyper_kw.items())))
    if key not in _CASES:
        D, Dx, H = shape
        rng = np.random.default_rng(sum(shape))
        hyper = L.LC2STHyper(D=D, Dx=Dx, H=H, **hyper_kw)
        R = 700
        data = torch.from_numpy(rng.standard_normal((R, D + Dx)).astype(np.float32))
        sizes = [(540, 60), (330, 33), (37, 1)] + ([(200, 20), (233, 64)] if H in (20, 100) else [])
        members = make_members(R, sizes, D + Dx, rng, data)
        params0 = torch.stack([L.init_params(hyper, s) for s in members.init_seed])
        _CASES[key] = (hyper, data, members, params0)
    return _CASES[key]


def subset(members, sel):
    return L.Members(*(getattr(members, f)[sel] for f in ("rows", "labels", "n_train", "n_valid", "member_id",
                                                           "init_seed")))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_eval_matches_the_fp64_oracle(shape):
    hyper, data, members, params0 = case(shape)
    g = torch.Generator().manual_seed(3)
    params = params0[:3] * 2.0           # wider logits than the initial weights give
    n = 333
    x_o = torch.randn(hyper.Dx, generator=g)
    for group_size, per_group in ((1, False), (1, True), (3, False), (3, True)):
        groups = 3 // group_size
        theta = torch.randn(*((groups, n) if per_group else (n,)), hyper.D, generator=g)
        proba, score = L.lc2st_eval(hyper, params, theta, x_o, group_size)
        p64, s64 = O.eval_proba(hyper, params, theta, x_o, group_size, torch.float64)
        p32, s32 = O.eval_proba(hyper, params, theta, x_o, group_size, torch.float32)
        assert proba.shape == (groups, n) and score.shape == (groups,)
        e_p, r_p = (proba.cpu().double() - p64).abs().max().item(), (p32.double() - p64).abs().max().item()
        e_s, r_s = (score.cpu().double() - s64).abs().max().item(), (s32.double() - s64).abs().max().item()
        what = f"E{group_size}-{'per-group' if per_group else 'shared'}"
        record("lc2st_eval", _ids(shape) + " | " + what, proba_hip_vs_f64=e_p, proba_oracle32_vs_f64=r_p,
               score_hip_vs_f64=e_s, score_oracle32_vs_f64=r_s)
        print(f"{what}: proba |hip-f64|={e_p:.3e} |o32-f64|={r_p:.3e}; score {e_s:.3e} / {r_s:.3e}")
        assert e_p <= 2.0 * r_p + 1e-5 and e_s <= 2.0 * r_s + 1e-5


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_batch_grad_matches_fp64_autograd(shape):
    hyper, data, members, params0 = case(shape)
    run = L.TrainerRun(hyper, data, members, SEED, params0)
    worst_rel = worst_block = 0.0
    for epoch in (0, 3):
        for batch in range(3):
            loss, grad = run.batch_grad(params0, 0, epoch, batch)
            loss, grad = loss.cpu().double(), grad.cpu().double()
            for m in range(run.M):
                if batch * hyper.batch_size >= members.n_train[m]:      # past the member's last batch
                    assert torch.isnan(loss[m]) and (grad[m] == 0).all()
                    continue
                rows, lab = O.member_batch(members, m, hyper, SEED, epoch, batch)
                lref, gref = O.loss_and_grad(hyper, params0[m], data, rows, lab, torch.float64)
                assert torch.isfinite(grad[m]).all()
                assert (loss[m] - lref).abs() <= 1e-5 + 1e-5 * lref.abs(), (m, epoch, batch, loss[m], lref)
                scale = gref.abs().max().item()
                rel = (grad[m] - gref).abs().max().item() / scale
                worst_rel = max(worst_rel, rel)
                for (name, _), a, b in zip(hyper.param_shapes(), O.split_params(hyper, grad[m]),
                                           O.split_params(hyper, gref)):
                    e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale)
                    worst_block = max(worst_block, e)
                    assert e <= 3e-4, f"{name} member {m} epoch {epoch} batch {batch}: {e:.3e}"
                assert rel <= 2e-4, (m, epoch, batch, rel)
    # the validation rows as one batch
    loss, grad = run.batch_grad(params0, 1)
    for m in range(run.M):
        rows, lab = O.member_valid(members, m)
        lref, gref = O.loss_and_grad(hyper, params0[m], data, rows, lab, torch.float64)
        assert (loss[m].cpu().double() - lref).abs() <= 1e-5 + 1e-5 * lref.abs()
        assert (grad[m].cpu().double() - gref).abs().max() <= 2e-4 * gref.abs().max()
    record("lc2st_batch_grad", _ids(shape), rel_grad_err_vs_f64=worst_rel, worst_block_rel_err=worst_block)
    print(f"grad rel {worst_rel:.3e} worst block {worst_block:.3e}")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_first_step_moves_every_parameter_by_lr_against_the_gradient_sign(shape):
    """After exactly one step from zero moments Adam's update is lr g / (|g| + eps): -lr sign(g) up to eps / |g|, which
    is 1 % at |g| = 1e-6, so "-lr sign(g) to 1e-6 relative" cannot hold even in exact arithmetic.  For every parameter
    with |g64| > 1e-6 the test pins lr g / (|g| + eps) at the fp64 gradient to 1e-6 relative, plus what the number
    formats force: the fp32 rounding of the stored parameter (2^-24 |p|), and the expression's sensitivity
    eps |dg| / (|g| + eps)^2 to the fp32 gradient's own error dg, bounded by twice the fp32 oracle's error in the
    max norm of the entry's tensor (the project's usual bar is norm-wise: another fp32 summation order has errors of
    that size, not the same error entry by entry) -- never by the kernel's output."""
    hyper, data, members, params0 = case(shape)
    one = subset(members, [2])          # 37 training rows < B: one epoch is exactly one step
    run = L.TrainerRun(hyper, data, one, SEED, params0[2:3])
    run.launch(1)
    assert int(run.step[0]) == 1 and int(run.epoch[0]) == 1
    rows, lab = O.member_batch(one, 0, hyper, SEED, 0, 0)
    _, g64 = O.loss_and_grad(hyper, params0[2], data, rows, lab, torch.float64)
    _, g32 = O.loss_and_grad(hyper, params0[2], data, rows, lab, torch.float32)
    p_new = run.params[0].cpu().double()
    moved = p_new - params0[2].double()
    sel = g64.abs() > 1e-6
    assert sel.sum() > 0.3 * sel.numel()
    dg = torch.cat([2.0 * t.abs().max().expand(t.numel()) for t in O.split_params(hyper, g32.double() - g64)])[sel]
    g = g64[sel]
    want = -hyper.lr * g / (g.abs() + hyper.eps)
    tol = hyper.lr * (1e-6 + hyper.eps * dg / (g.abs() + hyper.eps) ** 2) + 2.0**-24 * p_new.abs()[sel]
    err = (moved[sel] - want).abs()
    print(f"first step: {int(sel.sum())} entries, worst err/tol {(err / tol).max():.3f}, "
          f"worst |moved + lr sign g| / lr {((moved[sel] + hyper.lr * torch.sign(g)).abs() / hyper.lr).max():.3e}")
    assert (torch.sign(moved[sel]) == -torch.sign(g)).all()
    assert (err <= tol).all(), (err / tol).max()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_three_epoch_trajectory_against_the_fp64_oracle(shape):
    """history over 3 epochs against the fp64 oracle.  The bar is 4 x what the fp32 oracle itself deviates from fp64 on
    the same run, plus 1e-5 -- a multiple, because the kernel's summation order is a different fp32 order, not a better
    one.  For the same reason the fp32 oracle's deviation is taken over its own order AND four re-orderings of the rows
    inside every batch (same mathematics, another fp32 order): Adam's early updates g / (|g| + eps) turn a last-bit
    difference of a near-zero gradient entry into a step of a different size, and at F = 64, H = 120 three of the four
    re-ordered fp32 oracles land 2.9e-4 from fp64 where the as-is one lands 1.6e-7 (measured on the CPU oracle alone;
    DESIGN.md section 7f).  A bar from the as-is order only would test the order, not the arithmetic."""
    hyper, data, members, params0 = case(shape, max_epochs=3)
    run = L.TrainerRun(hyper, data, members, SEED, params0).run(3)
    hist = run.history.cpu().double().numpy()
    dev_hip = dev_o32 = dev_reordered = 0.0
    for m in range(run.M):
        r64 = O.train_member(hyper, data, members, m, params0[m], SEED, 3, torch.float64)
        dev_hip = max(dev_hip, np.abs(hist[m] - r64["history"]).max())
        for reorder in (None, 1, 2, 3, 4):
            r32 = O.train_member(hyper, data, members, m, params0[m], SEED, 3, torch.float32, reorder=reorder)
            d = np.abs(r32["history"] - r64["history"]).max()
            if reorder is None:
                dev_o32 = max(dev_o32, d)
            dev_reordered = max(dev_reordered, d)
    assert np.isfinite(hist).all()
    record("lc2st_trajectory", _ids(shape), history_hip_vs_f64=dev_hip, history_oracle32_vs_f64=dev_o32,
           history_oracle32_reordered_vs_f64=dev_reordered)
    print(f"trajectory: |hip-f64|={dev_hip:.3e} |o32-f64|={dev_o32:.3e} |o32 reordered-f64|={dev_reordered:.3e}")
    assert dev_hip <= 4.0 * dev_reordered + 1e-5


def _state(run):
    return [t.cpu().clone() for t in (run.params, run.best_params, run.history, run.best_epoch, run.epoch, run.step,
                                      run.exp_avg, run.exp_avg_sq, run.best, run.misses, run.stopped)]


def _same(a, b):
    return all(torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0))
               for x, y in zip(a, b))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_runs_are_deterministic_and_members_independent(shape):
    hyper, data, members, params0 = case(shape, max_epochs=4)
    ref = _state(L.TrainerRun(hyper, data, members, SEED, params0).run(4))
    assert _same(ref, _state(L.TrainerRun(hyper, data, members, SEED, params0).run(4)))        # two runs
    assert _same(ref, _state(L.TrainerRun(hyper, data, members, SEED, params0).run(1)))        # 1 epoch per launch
    for m in range(len(members.n_train)):                                                       # each member alone
        alone = _state(L.TrainerRun(hyper, data, subset(members, [m]), SEED, params0[m:m + 1]).run(4))
        assert _same([t[m:m + 1] for t in ref], alone), m
    other = _state(L.TrainerRun(hyper, data, members, SEED + 1, params0).run(4))                # and the seed matters
    assert not torch.equal(ref[0], other[0])


@pytest.mark.parametrize("shape,lr", [(SHAPES[1], 0.003), (SHAPES[3], 0.002), (SHAPES[5], 0.002)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else f"lr{v}")
def test_early_stopping_bookkeeping(shape, lr):
    """patience 2, max_epochs 12: replaying the rule over the kernel's own history reproduces stopped / epoch /
    best_epoch exactly, and the returned classifier's validation loss (batch_grad on the validation rows) is the recorded
    one of its best epoch to 1e-6.  In general the best epoch need not hold min(history[:, :, 1]) -- an epoch that
    undercuts the best by less than the relative threshold 1e-4 is the minimum without being an improvement -- so the
    minimum is bounded by the threshold; in these cases every epoch's relative change is >= 1e-3 away from the threshold
    (fp64 oracle), so the best epoch IS the minimum and that is asserted as well."""
    hyper, data, members, params0 = case(shape, max_epochs=12, patience=2, lr=lr)
    sel = [0, 1]             # learnable labels / coin-flip labels; at these learning rates the fp64 oracle runs the
    # first for all 12 epochs and stops the second early, with every epoch's relative change >= 1e-3 away from the 1e-4
    # threshold (so fp32 rounding cannot flip a decision)
    run = L.TrainerRun(hyper, data, subset(members, sel), SEED, params0[sel]).run(5)
    hist = run.history.cpu().numpy()
    stopped, epoch, best_epoch = run.stopped.cpu().numpy(), run.epoch.cpu().numpy(), run.best_epoch.cpu().numpy()
    vloss, _ = run.batch_grad(run.best_params, 1)
    vloss = vloss.cpu().numpy()
    for m in range(2):
        n_done = int(np.isfinite(hist[m, :, 1]).sum())
        want = L.early_stopping_replay(hist[m, :n_done, 1], 2, 12)
        print(f"member {m}: epochs {epoch[m]} best_epoch {best_epoch[m]} valid {hist[m, :n_done, 1]}")
        assert (bool(stopped[m]), int(epoch[m]), int(best_epoch[m])) == want
        assert n_done == epoch[m] and np.isnan(hist[m, n_done:]).all()
        at_best, lowest = hist[m, best_epoch[m], 1], np.nanmin(hist[m, :, 1])
        assert abs(vloss[m] - at_best) <= 1e-6
        assert at_best * (1 - 1e-4) - 1e-7 <= lowest <= at_best
        assert abs(vloss[m] - lowest) <= 1e-6
    assert stopped.all()
    assert (epoch < 12).any() and (epoch == 12).any(), epoch


def test_a_row_list_longer_than_its_stride_is_refused_on_the_device():
    """n_train + n_valid > row_stride (the host API never builds that): the member is marked stopped untrained, its
    batch gradient is NaN / 0, nothing is read past the list, and the other members train as if alone."""
    hyper, data, members, params0 = case(SHAPES[1], max_epochs=2)
    ref = L.TrainerRun(hyper, data, members, SEED, params0).run(2)
    run = L.TrainerRun(hyper, data, members, SEED, params0)
    run.n_valid[1] = run.rows.shape[1]
    run.run(2)
    assert int(run.stopped[1]) == 1 and int(run.epoch[1]) == 0 and int(run.step[1]) == 0
    assert torch.equal(run.params[1], params0[1].cuda()) and torch.isnan(run.history[1]).all()
    keep = [0, 2, 3, 4]
    assert torch.equal(run.params[keep], ref.params[keep]) and torch.equal(run.epoch[keep], ref.epoch[keep])
    loss, grad = run.batch_grad(params0, 0, 0, 0)
    assert torch.isnan(loss[1]) and (grad[1] == 0).all() and torch.isfinite(loss[keep]).all()


# ---- end to end ------------------------------------------------------------------------------------------------------
X_OBS = [(0.0, 0.0), (1.0, -0.5), (-1.0, -1.0)]


def _linear_gaussian(n, shift, seed):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(n, 2, generator=g)
    x = theta + 0.5 * torch.randn(n, 2, generator=g)
    post = 0.8 * x + shift + 0.2**0.5 * torch.randn(n, 2, generator=g)
    theta_o = [0.8 * torch.tensor(xo) + shift + 0.2**0.5 * torch.randn(2000, 2, generator=g) for xo in X_OBS]
    return theta, x, post, theta_o


@pytest.mark.parametrize("shift", [0.0, 0.3], ids=["exact-posterior", "mean-shifted-by-0.3"])
def test_lc2st_on_the_linear_gaussian(shift):
    """prior N(0, I_2), x = theta + eps / 2: posterior N(0.8 x, 0.2 I).  The exact posterior is not rejected at any of
    three observations; a mean shift of 0.3 is, with T_obs above every null statistic."""
    theta, x, post, theta_o = _linear_gaussian(2000, shift, seed=5)
    lc = LC2ST(theta, x, post, seed=1, num_trials_null=20, classifier_kwargs=dict(max_epochs=60, patience=10))
    assert lc.state == LC2STState.INITIALIZED
    lc.train_on_observed_data().train_under_null_hypothesis()
    assert lc.state == LC2STState.READY and len(lc.trained_clfs_null) == 20
    for xo, th in zip(X_OBS, theta_o):
        xo = torch.tensor(xo)
        t_obs = lc.get_statistic_on_observed_data(th, xo)
        t_null = lc.get_statistics_under_null_hypothesis(th, xo).scores
        p = lc.p_value(th, xo)
        print(f"shift {shift} x_o {xo.tolist()}: T_obs {t_obs:.5f} max T_null {t_null.max():.5f} p {p:.3f}")
        assert isinstance(p, float) and t_null.shape == (20,)
        if shift == 0.0:
            assert p >= 0.05
            assert lc.reject_test(th, xo) is False
        else:
            assert p == 0.0 and t_obs > t_null.max()
            assert lc.reject_test(th, xo) is True


def test_lc2st_nf_on_a_trained_npe_and_null_classifier_reuse():
    from torch.distributions import MultivariateNormal

    from sbi_amd.inference import NPE
    from sbi_amd.neural_nets import NSFConfig

    theta_tr, x_tr, _, _ = _linear_gaussian(8000, 0.0, seed=7)       # the estimator's own training set
    theta, x, _, _ = _linear_gaussian(2000, 0.0, seed=6)             # the calibration set of the test (N = 2 000)
    torch.manual_seed(2)
    prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
    inf = NPE(prior=prior, density_estimator=NSFConfig(), device="cuda", show_progress_bars=False)
    est = inf.append_simulations(theta_tr, x_tr).train(training_batch_size=200)
    post = est.sample(torch.Size([1]), condition=x.cuda()).reshape(-1, 2).cpu()
    base = MultivariateNormal(torch.zeros(2), torch.eye(2))

    def inverse(th, xx):
        return est.inverse_transform(th.cuda(), xx.cuda()).cpu()

    kw = dict(num_eval=2000, seed=1, num_trials_null=20, classifier_kwargs=dict(max_epochs=60, patience=10))
    nf = LC2ST_NF(theta, x, post, flow_inverse_transform=inverse, flow_base_dist=base, **kw)
    assert nf.permutation is False and nf.state == LC2STState.INITIALIZED
    nf.train_under_null_hypothesis()
    assert nf.state == LC2STState.NULL_TRAINED
    nf.train_on_observed_data()
    x_o = torch.zeros(2)
    p, t_obs = nf.p_value(x_o), nf.get_statistic_on_observed_data(x_o)
    print(f"LC2ST_NF: T_obs {t_obs:.5f} p {p:.3f}")
    assert p >= 0.05
    # the null classifiers do not depend on the estimator: a second (deliberately shifted) one reuses them
    def inverse_shifted(th, xx):
        return inverse(th - 0.3, xx)

    nf2 = LC2ST_NF(theta, x, post + 0.3, flow_inverse_transform=inverse_shifted, flow_base_dist=base,
                   trained_clfs_null=nf.trained_clfs_null, **kw)
    assert nf2.state == LC2STState.NULL_TRAINED
    with pytest.raises(ValueError, match="already trained"):
        nf2.train_under_null_hypothesis()
    nf2.train_on_observed_data()
    assert nf2.state == LC2STState.READY
    assert 0.0 <= nf2.p_value(x_o) <= 1.0
