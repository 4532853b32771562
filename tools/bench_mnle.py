"""MNLE measurements: every figure next to the eager-torch restatement (tests/mnle_oracle.py) on the same GPU.

    python tools/bench_mnle.py --out profiles/mnle_bench.json

Shapes: theta-dim 4, one binary choice column, sbi's defaults (widths 50, 2 MADE blocks, 5 transforms, 10 bins),
log-transformed reaction times.
  * `step_B200`, `step_B65536`  -- one FusedMNLEStep.step (re-pack, fused joint loss forward + backward, fixed-order
        weight-gradient reduction, clip + Adam) against the restatement's loss, autograd, clip_grad_norm_ and Adam;
  * `log_prob_paired_65536`     -- 65 536 (x, theta) pairs;
  * `trials_T100_N20`, `trials_T1000_N2000` -- the iid-trials potential sum_t log p(x_t | theta_n): one pass over the
        (trial, theta) grid read in place against the restatement on the expanded (T N) pairs.
Device times are medians over CUDA events after a warm-up of the same leg (the device ramps its clock after idling).
"""
import argparse
import json
import sys
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _median_ms(fn, reps=30, warm=10):
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions (profiling runs)")
    ap.add_argument("--hip-only", action="store_true", help="skip the eager legs (kernel traces of the library alone)")
    a = ap.parse_args()
    import torch

    from sbi_amd.inference.trainers.fused import FusedMNLEStep
    from sbi_amd.neural_nets.estimators.mixed_density_estimator import (mnle_log_prob_call, mnle_trials_call,
                                                                        split_input)
    from sbi_amd.neural_nets.net_builders.mixed_nets import build_mnle
    from tests.mnle_oracle import MixedOracle

    reps = 5 if a.quick else 30

    def eager_ms(fn, **kw):
        return float("nan") if a.hip_only else _median_ms(fn, **kw)

    C = 4
    res = {"device": torch.cuda.get_device_name(0), "C": C, "num_categories": [2], "widths": 50,
           "num_transforms": 5, "num_bins": 10, "log_transform_x": True}
    torch.manual_seed(0)
    N = 65536
    theta = torch.randn(N, C)
    choice = (torch.rand(N) < torch.sigmoid(2 * theta[:, 0])).float()
    rt = torch.exp(0.5 * theta[:, 1] + 0.3 * (2 * choice - 1) + 0.25 * torch.randn(N))
    x = torch.stack([rt, choice], 1)

    def build():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return build_mnle(x, theta, log_transform_x=True).cuda()

    def restatement(est):
        o = MixedOracle([2], [torch.tensor([0.0, 1.0])], C, log_transform=True)
        o.set_zstats(est.net.zstats.cpu())
        o.load_state_dict(est.state_dict(), strict=False)
        return o.cuda()

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    xx, th = x.cuda(), theta.cuda()
    for B in (200, 65536):
        e = build()
        step = FusedMNLEStep(e)
        xb, tb = xx[:B].contiguous(), th[:B].contiguous()
        t_hip = _median_ms(lambda: step.step(xb, tb), reps=reps)
        o = restatement(e)
        opt = torch.optim.Adam(o.parameters(), lr=5e-4)

        def eager():
            opt.zero_grad()
            o.loss(xb, tb).mean().backward()
            torch.nn.utils.clip_grad_norm_(o.parameters(), 5.0)
            opt.step()

        t_eager = eager_ms(eager, reps=reps)
        put(f"step_B{B}", batch=B, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip)

    est = build()
    oracle = restatement(est)
    with torch.no_grad():
        xc, idx, val = split_input(est.net, xx)
        t_hip = _median_ms(lambda: mnle_log_prob_call(est.net, xc, idx, val, th), reps=reps)
        t_eager = eager_ms(lambda: oracle.log_prob(xx, th), reps=reps)
        put("log_prob_paired_65536", rows=N, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip)
        for T, M in ((100, 20), (1000, 2000)):
            x_o, th_m = xx[:T].contiguous(), th[:M].contiguous()
            xc, idx, val = split_input(est.net, x_o)
            t_hip = _median_ms(lambda: mnle_trials_call(est.net, xc, idx, val, th_m), reps=reps)

            def eager_trials():
                xe = x_o[:, None, :].expand(T, M, 2).reshape(T * M, 2)
                te = th_m[None].expand(T, M, C).reshape(T * M, C)
                return oracle.log_prob(xe, te).reshape(T, M).sum(0)

            t_eager = eager_ms(eager_trials, reps=max(3, reps // 3), warm=3)
            put(f"trials_T{T}_N{M}", trials=T, thetas=M, pairs=T * M, hip_ms=t_hip, eager_ms=t_eager,
                speedup=t_eager / t_hip)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
