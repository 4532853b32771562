"""GPU parity of the L-C2ST kernels (csrc/lc2st_kernel.h) over the edges of their tile, chunk and row-block structure,
which tests/test_lc2st_gpu.py (one batch size, one evaluation size, six shapes) does not reach.  The cases and their
reasons are the table of tests/lc2st_envelope.py; tests/test_lc2st_envelope_cpu.py shows without a device that the
table hits every edge, that the bounds hold for the fp32 eager oracle alone with a factor 5 to spare, and that the
last live row and column of every weight gradient is large enough, at some case, for the bounds to notice its loss.

  (1) batch gradient against fp64 autograd at B = 1, 31, 32, 33, 64, 97, 200: each member's first and last batch at
      epochs 0 and 3, a batch index past the end (NaN loss, zero gradient), and the validation rows as one batch,
  (2) evaluation against the fp64 oracle at n = 1 .. 1025 (one to three row blocks of 512, full and partial) in the
      four group layouts; every run equals, bit for bit, the leading rows of the n = 1025 run,
  (3) the first Adam step of the 1-row and the 33-row member,
  (4) three-epoch trajectories at B = 32 and 33, all five members,
  (5) determinism, launch granularity and member independence at B = 33.

Every kernel call goes through `TrainerRun`, `TrainerRun.batch_grad` and `lc2st_eval`.  Bounds are those of
tests/test_lc2st_gpu.py.  Measured distances go to the parity log under lc2st_envelope_* (committed as
profiles/parity_lc2st_envelope.json)."""
import numpy as np
import pytest
import torch

from sbi_amd.diagnostics import lc2st as L
from tests import lc2st_envelope as env
from tests import lc2st_oracle as O
from tests.parity_log import record
from tests.test_lc2st_gpu import _same, _state, subset

pytestmark = pytest.mark.gpu

SHAPES = env.SHAPE_LIST
SEED = env.SEED
KEY = "lc2st_envelope_"


@pytest.mark.parametrize("shape", SHAPES, ids=env.shape_id)
def test_batch_grad_matches_fp64_autograd(shape):
    data, members, params0 = env.inputs(shape)
    refs = env.grad_references(shape)
    M = len(env.MEMBER_SIZES)
    worst_rel = worst_block = worst_loss = 0.0
    compared = set()

    def compare(h, key, loss_m, grad_m):
        nonlocal worst_rel, worst_block, worst_loss
        _, _, lref, gref = refs[key]
        assert torch.isfinite(grad_m).all(), key
        e_loss = (loss_m - lref).abs().item()
        worst_loss = max(worst_loss, e_loss / (env.LOSS_ABS + env.LOSS_REL * lref.abs().item()))
        assert e_loss <= env.LOSS_ABS + env.LOSS_REL * lref.abs(), (key, loss_m, lref)
        rel = (grad_m - gref).abs().max().item() / gref.abs().max().item()
        worst_rel = max(worst_rel, rel)
        for name, e in env.block_metric(h, grad_m, gref):
            worst_block = max(worst_block, e)
            assert e <= env.BLOCK_REL, f"{name} at (B, which, epoch, batch, member) = {key}: {e:.3e}"
        assert rel <= env.GRAD_REL, (key, rel)
        compared.add(key)

    for B in env.GRAD_BATCH_SIZES:
        h = env.hyper(shape, batch_size=B)
        run = L.TrainerRun(h, data, members, SEED, params0)
        for epoch in env.GRAD_EPOCHS:
            for batch in env.grad_batches(B):
                loss, grad = run.batch_grad(params0, 0, epoch, batch)
                loss, grad = loss.cpu().double(), grad.cpu().double()
                for m, (nt, _) in enumerate(env.MEMBER_SIZES):
                    if batch * B >= nt:                                   # past the member's last batch
                        assert torch.isnan(loss[m]) and (grad[m] == 0).all(), (B, epoch, batch, m)
                    elif (B, 0, epoch, batch, m) in refs:
                        compare(h, (B, 0, epoch, batch, m), loss[m], grad[m])
                    else:                                                 # another member's last batch
                        assert torch.isfinite(loss[m]) and torch.isfinite(grad[m]).all(), (B, epoch, batch, m)
    h = env.hyper(shape)
    loss, grad = L.TrainerRun(h, data, members, SEED, params0).batch_grad(params0, 1)     # the validation rows
    loss, grad = loss.cpu().double(), grad.cpu().double()
    for m in range(M):
        compare(h, (h.batch_size, 1, 0, 0, m), loss[m], grad[m])
    assert compared == set(refs)
    record(KEY + "batch_grad", env.shape_id(shape), rel_grad_err_vs_f64=worst_rel, worst_block_rel_err=worst_block,
           worst_loss_err_over_tolerance=worst_loss, cases=len(compared))
    print(f"{len(compared)} cases: grad rel {worst_rel:.3e} worst block {worst_block:.3e} "
          f"loss {worst_loss:.3f} of its tolerance")


@pytest.mark.parametrize("shape", SHAPES, ids=env.shape_id)
def test_eval_matches_the_fp64_oracle_and_row_blocks_do_not_depend_on_the_grid(shape):
    params, _, x_o = env.eval_inputs(shape)
    refs = env.eval_references(shape)
    h = env.hyper(shape)
    n_max = max(env.EVAL_SIZES)
    for group_size, per_group in env.EVAL_LAYOUTS:
        groups = 3 // group_size
        what = f"E{group_size}-{'per-group' if per_group else 'shared'}"
        got = {}
        worst = dict(e_p=0.0, r_p=0.0, e_s=0.0, r_s=0.0)
        for n in env.EVAL_SIZES:
            proba, score = L.lc2st_eval(h, params, env.eval_theta(shape, n, group_size, per_group), x_o, group_size)
            proba, score = proba.cpu(), score.cpu()
            p64, s64, p32, s32 = refs[(n, group_size, per_group)]
            assert proba.shape == (groups, n) and score.shape == (groups,)
            e_p, r_p = (proba.double() - p64).abs().max().item(), (p32.double() - p64).abs().max().item()
            e_s, r_s = (score.double() - s64).abs().max().item(), (s32.double() - s64).abs().max().item()
            print(f"{what} n={n}: proba |hip-f64|={e_p:.3e} |o32-f64|={r_p:.3e}; score {e_s:.3e} / {r_s:.3e}")
            for k, v in dict(e_p=e_p, r_p=r_p, e_s=e_s, r_s=r_s).items():
                worst[k] = max(worst[k], v)
            assert e_p <= 2.0 * r_p + 1e-5 and e_s <= 2.0 * r_s + 1e-5, (what, n)
            got[n] = proba
        record(KEY + "eval", env.shape_id(shape) + " | " + what, proba_hip_vs_f64=worst["e_p"],
               proba_oracle32_vs_f64=worst["r_p"], score_hip_vs_f64=worst["e_s"], score_oracle32_vs_f64=worst["r_s"])
        # a row's probability does not depend on the row block, the chunk or the grid it was computed in
        assert torch.equal(got[n_max][:, :512], got[512]), what
        for n in env.EVAL_SIZES:
            assert torch.equal(got[n_max][:, :n], got[n]), (what, n)


@pytest.mark.parametrize("shape", SHAPES, ids=env.shape_id)
def test_first_step_moves_every_parameter_by_lr_against_the_gradient_sign(shape):
    """As tests/test_lc2st_gpu.py's test of the same name (see there for the bound), for the member of one training
    row (inv_n = 1, a permutation of one element) and the member of 33 rows (a chunk and one row) at B = 64.  No shape
    is left out: tests/test_lc2st_envelope_cpu.py shows that more than 0.9 of the entries have |g64| > 1e-6 at every
    shape and both members, against the 0.3 required."""
    data, members, params0 = env.inputs(shape)
    h = env.hyper(shape, batch_size=env.FIRST_STEP_BATCH_SIZE)
    worst = 0.0
    for m in env.FIRST_STEP_MEMBERS:
        assert (shape, m) not in env.FIRST_STEP_LEFT_OUT
        one = subset(members, [m])
        run = L.TrainerRun(h, data, one, SEED, params0[m:m + 1])
        run.launch(1)
        assert int(run.step[0]) == 1 and int(run.epoch[0]) == 1
        rows, lab = O.member_batch(one, 0, h, SEED, 0, 0)
        _, g64 = O.loss_and_grad(h, params0[m], data, rows, lab, torch.float64)
        _, g32 = O.loss_and_grad(h, params0[m], data, rows, lab, torch.float32)
        p_new = run.params[0].cpu().double()
        moved = p_new - params0[m].double()
        sel = g64.abs() > 1e-6
        assert sel.sum() > 0.3 * sel.numel()
        dg = torch.cat([2.0 * t.abs().max().expand(t.numel()) for t in O.split_params(h, g32.double() - g64)])[sel]
        g = g64[sel]
        want = -h.lr * g / (g.abs() + h.eps)
        tol = h.lr * (1e-6 + h.eps * dg / (g.abs() + h.eps) ** 2) + 2.0**-24 * p_new.abs()[sel]
        err = (moved[sel] - want).abs()
        worst = max(worst, (err / tol).max().item())
        print(f"member {m}: {int(sel.sum())} of {sel.numel()} entries, worst err/tol {(err / tol).max():.3f}")
        assert (torch.sign(moved[sel]) == -torch.sign(g)).all()
        assert (err <= tol).all(), (m, (err / tol).max())
    record(KEY + "first_step", env.shape_id(shape), worst_err_over_tolerance=worst)


@pytest.mark.parametrize("shape", SHAPES, ids=env.shape_id)
def test_three_epoch_trajectory_against_the_fp64_oracle(shape):
    """The rule of tests/test_lc2st_gpu.py: 4 x the worst deviation of the as-is and four re-ordered fp32 oracles from
    fp64, plus 1e-5.  At these sizes (at most 97 rows, at most 4 steps per epoch) the fp32 oracles land about 1e-7
    from fp64 on the CPU (1.8e-6 at (32, 16, 48), the largest), so the 1e-5 floor decides the bound."""
    data, members, params0 = env.inputs(shape)
    numbers = {}
    for B in env.TRAJECTORY_BATCH_SIZES:
        h = env.hyper(shape, batch_size=B, max_epochs=3)
        run = L.TrainerRun(h, data, members, SEED, params0).run(3)
        hist = run.history.cpu().double().numpy()
        assert np.isfinite(hist).all()
        dev_hip = dev_o32 = dev_reordered = 0.0
        for m, (r64, as_is, reordered) in enumerate(env.trajectory_references(shape, B)):
            dev_hip = max(dev_hip, np.abs(hist[m] - r64).max())
            dev_o32, dev_reordered = max(dev_o32, as_is), max(dev_reordered, reordered)
        numbers.update({f"B{B}_history_hip_vs_f64": dev_hip, f"B{B}_history_oracle32_vs_f64": dev_o32,
                        f"B{B}_history_oracle32_reordered_vs_f64": dev_reordered})
        print(f"B={B}: |hip-f64|={dev_hip:.3e} |o32-f64|={dev_o32:.3e} |o32 reordered-f64|={dev_reordered:.3e}")
        assert dev_hip <= 4.0 * dev_reordered + 1e-5, B      # the 1e-5 floor decides: 4 x ~1e-7 is far below it
    record(KEY + "trajectory", env.shape_id(shape), **numbers)


@pytest.mark.parametrize("shape", SHAPES, ids=env.shape_id)
def test_runs_are_deterministic_and_members_independent(shape):
    data, members, params0 = env.inputs(shape)
    h = env.hyper(shape, batch_size=33, max_epochs=4)
    ref = _state(L.TrainerRun(h, data, members, SEED, params0).run(4))
    assert _same(ref, _state(L.TrainerRun(h, data, members, SEED, params0).run(4)))        # two runs
    assert _same(ref, _state(L.TrainerRun(h, data, members, SEED, params0).run(1)))        # 1 epoch per launch
    for m in range(len(env.MEMBER_SIZES)):                                                  # each member alone
        alone = _state(L.TrainerRun(h, data, subset(members, [m]), SEED, params0[m:m + 1]).run(4))
        assert _same([t[m:m + 1] for t in ref], alone), m
    assert int(ref[4].min()) == 4 and torch.isfinite(ref[2]).all()      # every member ran its four epochs
