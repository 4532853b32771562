#!/usr/bin/env python
"""Measure the L-C2ST classifier ensemble at the reference's default sizes and write profiles/lc2st_bench.json.

D = Dx = 10 (hidden 100), N = 10 000 calibration pairs, 1 + 100 members:
  * device milliseconds per epoch of one trainer launch, for several `epochs_this_launch` (all members alive);
  * wall time of `LC2ST.train_under_null_hypothesis()` (100 null members, defaults: up to 1 000 epochs, patience 50);
  * one evaluation of all 101 classifiers at 10 000 draws.
Baselines on the same GPU (eager torch, the tests' restatement of the same network and optimiser):
  (a) the members one after the other with `torch.optim.Adam` -- this STANDS IN for the reference's skorch path, which
      cannot be installed here; a few hundred steps of one member are timed and scaled to an epoch of 101 members;
  (b) the 101 members batched through `torch.bmm` with a hand-written Adam step over the stacked parameters.
No ratio is promised anywhere: the file holds what was measured, plus the fraction of the fp32 matrix peak that the
algorithmic FLOP count of an epoch amounts to.

`--profile-run` does a short trainer run and one evaluation only (no baselines), for
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_lc2st.py --profile-run
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sbi_amd.diagnostics import LC2ST  # noqa: E402
from sbi_amd.diagnostics import lc2st as L  # noqa: E402

PEAK_FP32_MATRIX_TFLOPS = 157.3     # MI355X data sheet, v_mfma_f32_16x16x4_f32


def make_problem(n, d, dx, seed=0):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(n, d, generator=g)
    x = torch.cat([theta, theta], 1)[:, :dx] + 0.5 * torch.randn(n, dx, generator=g)
    post = 0.8 * x[:, :d] + 0.2**0.5 * torch.randn(n, d, generator=g)
    return theta, x, post


def device_ms(fn, reps=1):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def flops_per_epoch(hyper, members):
    """Algorithmic: forward 2, d/dW 2 flop per weight and row, d/dactivation 2 per hidden-to-hidden and output weight;
    the validation pass is one more forward."""
    w = hyper.H * hyper.F + hyper.H * hyper.H + hyper.H
    train = float(members.n_train.sum()) * (4 * w + 2 * (hyper.H * hyper.H + hyper.H))
    return train + float(members.n_valid.sum()) * 2 * w


def eager_sequential_ms_per_step(hyper, data, members, steps=300):
    from tests import lc2st_oracle as O

    p = L.init_params(hyper, 1).cuda().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=hyper.lr, weight_decay=hyper.weight_decay)
    rows = torch.from_numpy(members.rows[0, : hyper.batch_size].astype(np.int64)).cuda()
    y = torch.from_numpy(members.labels[0, : hyper.batch_size]).cuda()

    def step():
        opt.zero_grad()
        torch.nn.functional.binary_cross_entropy_with_logits(O.logits(hyper, p, data[rows]), y).backward()
        opt.step()

    for _ in range(20):
        step()
    return device_ms(step, steps), wall_ms(step, steps)


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def eager_bmm_ms_per_step(hyper, data, members, steps=100):
    M, H, Fd, B = len(members.n_train), hyper.H, hyper.F, hyper.batch_size
    g = torch.Generator().manual_seed(0)
    ps = [((torch.rand(M, *s, generator=g) * 2 - 1) * 0.1).cuda().requires_grad_(True)
          for s in ((H, Fd), (1, H), (H, H), (1, H), (H, 1), (1, 1))]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    rows = torch.from_numpy(members.rows[:, :B].astype(np.int64)).cuda()
    y = torch.from_numpy(members.labels[:, :B]).cuda()
    t = [0]

    def step():
        X = data[rows]                                                   # (M, B, F)
        w1, b1, w2, b2, w3, b3 = ps
        h = torch.relu(torch.bmm(X, w1.transpose(1, 2)) + b1)
        h = torch.relu(torch.bmm(h, w2.transpose(1, 2)) + b2)
        z = (torch.bmm(h, w3) + b3)[..., 0]
        loss = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="none").mean(1).sum()
        grads = torch.autograd.grad(loss, ps)
        t[0] += 1
        bc1, bc2 = 1 - hyper.beta1 ** t[0], 1 - hyper.beta2 ** t[0]
        with torch.no_grad():
            for p, gr, m, v in zip(ps, grads, ms, vs):
                gr = gr + hyper.weight_decay * p
                m.lerp_(gr, 1 - hyper.beta1)
                v.mul_(hyper.beta2).addcmul_(gr, gr, value=1 - hyper.beta2)
                p.addcdiv_(m, v.sqrt() / bc2**0.5 + hyper.eps, value=-hyper.lr / bc1)

    for _ in range(10):
        step()
    return device_ms(step, steps), wall_ms(step, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--num-eval", type=int, default=10_000)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lc2st_bench.json"))
    a = ap.parse_args()
    theta, x, post = make_problem(a.n, a.dim, a.dim)
    lc = LC2ST(theta, x, post, seed=1, num_trials_null=a.trials)
    hyper = lc.hyper
    data, null_trials = lc._null_trials()
    members = L.build_members(a.n, 1, 1, 1, [(0, None, 0)] + null_trials)
    M = len(members.n_train)
    steps_per_epoch = int(np.ceil(members.n_train / hyper.batch_size).sum())
    theta_o = torch.randn(a.num_eval, a.dim)

    if a.profile_run:
        run = L.TrainerRun(hyper, data, members, 1)
        for _ in range(3):
            run.launch(4)
        L.lc2st_eval(hyper, run.params, theta_o, x[0])
        torch.cuda.synchronize()
        return

    res = {"config": dict(D=a.dim, Dx=a.dim, H=hyper.H, N=a.n, members=M, batch_size=hyper.batch_size,
                          steps_per_epoch_all_members=steps_per_epoch, rows_train=int(members.n_train[0]),
                          rows_valid=int(members.n_valid[0])),
           "device": torch.cuda.get_device_name(0)}
    # -- the trainer launch, all members alive -------------------------------------------------------------------------
    L.TrainerRun(hyper, data, members, 1).launch(1)        # first-launch costs (module load, LDS attribute)
    per_launch = {}
    for k in (1, 2, 4, 8, 16):
        run = L.TrainerRun(hyper, data, members, 1)
        ms = device_ms(lambda: run.launch(k))
        assert int(run.stopped.sum()) == 0
        per_launch[str(k)] = {"launch_ms": ms, "ms_per_epoch": ms / k}
    res["train_launch"] = per_launch
    ms_epoch = per_launch["8"]["ms_per_epoch"]
    fl = flops_per_epoch(hyper, members)
    res["algorithmic_gflop_per_epoch"] = fl / 1e9
    res["achieved_tflops"] = fl / (ms_epoch * 1e-3) / 1e12
    res["fraction_of_fp32_matrix_peak"] = res["achieved_tflops"] / PEAK_FP32_MATRIX_TFLOPS
    res["us_per_step_per_member"] = ms_epoch * 1e3 / (steps_per_epoch / M)
    # -- the public call ----------------------------------------------------------------------------------------------
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lc.train_under_null_hypothesis()
    torch.cuda.synchronize()
    res["train_under_null_hypothesis_wall_s"] = time.perf_counter() - t0
    ep = np.concatenate([c.epochs for clfs in lc.trained_clfs_null.values() for c in clfs])
    res["null_epochs_trained"] = dict(min=int(ep.min()), mean=float(ep.mean()), max=int(ep.max()))
    res["epochs_per_launch"] = lc.epochs_per_launch
    # -- evaluation ---------------------------------------------------------------------------------------------------
    params = torch.cat([c.params for clfs in lc.trained_clfs_null.values() for c in clfs])
    L.lc2st_eval(hyper, params, theta_o, x[0])
    res["eval_ms"] = {"members": int(params.shape[0]), "draws": a.num_eval,
                      "device_ms": device_ms(lambda: L.lc2st_eval(hyper, params, theta_o, x[0]), 5)}
    # -- baselines ----------------------------------------------------------------------------------------------------
    dev_data = data.cuda()
    d_ms, w_ms = eager_sequential_ms_per_step(hyper, dev_data, members)
    res["baseline_eager_sequential"] = {
        "note": "eager torch, one member after the other with torch.optim.Adam; stands in for the reference's skorch "
                "path, which cannot be installed here; 300 steps of one member timed, scaled to an epoch of all members",
        "device_ms_per_step": d_ms, "wall_ms_per_step": w_ms, "ms_per_epoch_all_members": w_ms * steps_per_epoch}
    d_ms, w_ms = eager_bmm_ms_per_step(hyper, dev_data, members)
    res["baseline_eager_bmm"] = {
        "note": "eager torch, all members batched through bmm, hand-written Adam over the stacked parameters",
        "device_ms_per_step": d_ms, "wall_ms_per_step": w_ms,
        "ms_per_epoch_all_members": w_ms * steps_per_epoch / M}
    res["not_measured"] = ["the reference's skorch path itself (not installable)", "validation pass and early stopping "
                           "in the eager baselines (training steps only)"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
