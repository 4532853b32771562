"""Affine MAF measurements: every figure next to the `maf_rqs` kernels at the same shape and next to the eager-torch
restatement (tests/maf_affine_oracle.py) on the same GPU.

    python tools/bench_maf_affine.py --out profiles/maf_affine_bench.json

Shapes: theta-dim = x-dim = 10, sbi's defaults (hidden 50, 2 blocks, 5 transforms).
  * `step_B200`, `step_B65536` -- one FusedTrainStep.step (re-pack, forward with stash, per-transform backward,
        split-K weight gradients, fixed-order reduction, clip + Adam) of the affine MAF, of maf_rqs, and the
        restatement's loss, autograd, clip_grad_norm_ and Adam;
  * `log_prob_paired_65536`    -- 65 536 (theta, x) pairs;
  * `sample_1e6`               -- 10^6 draws at one x_o (given noise: the inverse direction, D passes per transform).
`affine_over_rqs` < 1 means the affine kernel is the faster one; the floor this tool checks is "not slower than maf_rqs
at both step sizes" (same hidden stack, a 2-tile head instead of D * PT tiles, no spline).
Device times are medians over CUDA events after a warm-up (the device ramps its clock after idling); no idle gap sits
in front of a timed region.  The two kernel legs that are compared are timed ALTERNATELY (affine, maf_rqs, affine,
...), so a drift of the clock falls on both.  The exit status is 1 when the floor is missed.
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


def _paired_median_ms(fa, fb, reps=30, warm=10):
    """Medians of two legs timed alternately, after warming both."""
    import torch

    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return tuple(sorted(t)[len(t) // 2] for t in ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--hip-only", action="store_true", help="skip the eager legs")
    a = ap.parse_args()
    import torch

    from sbi_amd.inference.trainers.fused import FusedTrainStep
    from sbi_amd.neural_nets.net_builders.flow import build_maf, build_maf_rqs
    from tests.maf_affine_oracle import MAFOracle

    reps = 5 if a.quick else 30

    def eager_ms(fn, **kw):
        return float("nan") if a.hip_only else _median_ms(fn, **kw)

    D = 10
    res = {"device": torch.cuda.get_device_name(0), "D": D, "C": D, "hidden_features": 50, "num_transforms": 5,
           "num_blocks": 2}
    torch.manual_seed(0)
    N = 65536
    theta = torch.randn(N, D) * (0.1 ** 0.5)
    x = theta + (0.1 ** 0.5) * torch.randn(N, D)

    def build(fn):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn(theta[:2000], x[:2000]).cuda()

    def restatement(est):
        o = MAFOracle(theta[:2000], x[:2000])
        o.load_state_dict(est.state_dict())
        return o.cuda()

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    th, xx = theta.cuda(), x.cuda()
    ok = True
    for B in (200, 65536):
        tb, xb = th[:B].contiguous(), xx[:B].contiguous()
        e = build(build_maf)
        step = FusedTrainStep(e, lr=5e-4, clip_max_norm=5.0)
        r = build(build_maf_rqs)
        rstep = FusedTrainStep(r, lr=5e-4, clip_max_norm=5.0)
        t_aff, t_rqs = _paired_median_ms(lambda: step.step(tb, xb), lambda: rstep.step(tb, xb), reps=reps)
        o = restatement(e)
        opt = torch.optim.Adam(o.parameters(), lr=5e-4)

        def eager():
            opt.zero_grad()
            o.loss(tb, xb).mean().backward()
            torch.nn.utils.clip_grad_norm_(o.parameters(), 5.0)
            opt.step()

        t_eager = eager_ms(eager, reps=reps)
        ok = ok and t_aff <= t_rqs
        put(f"step_B{B}", batch=B, affine_ms=t_aff, maf_rqs_ms=t_rqs, eager_ms=t_eager,
            affine_over_rqs=t_aff / t_rqs, speedup_vs_eager=t_eager / t_aff)

    e, r = build(build_maf), build(build_maf_rqs)
    o = restatement(e)
    with torch.no_grad():
        t_aff, t_rqs = _paired_median_ms(lambda: e.log_prob(th, xx), lambda: r.log_prob(th, xx), reps=reps)
        t_eager = eager_ms(lambda: o.log_prob(th, xx), reps=reps)
        put("log_prob_paired_65536", rows=N, affine_ms=t_aff, maf_rqs_ms=t_rqs, eager_ms=t_eager,
            affine_over_rqs=t_aff / t_rqs, speedup_vs_eager=t_eager / t_aff)
        M = 10 ** 6
        noise = torch.randn(M, D, device="cuda")
        x_o = xx[:1].contiguous()
        t_aff, t_rqs = _paired_median_ms(lambda: e.sample_from_noise(noise, x_o),
                                         lambda: r.sample_from_noise(noise, x_o), reps=max(3, reps // 3), warm=3)
        x_rep = x_o.expand(M, -1)
        t_eager = eager_ms(lambda: o.sample_from_noise(noise, x_rep), reps=3, warm=1)
        put("sample_1e6", draws=M, affine_ms=t_aff, maf_rqs_ms=t_rqs, eager_ms=t_eager,
            affine_over_rqs=t_aff / t_rqs, speedup_vs_eager=t_eager / t_aff)
    res["floor_not_slower_than_maf_rqs_at_both_step_sizes"] = bool(ok)
    print("floor (affine step not slower than maf_rqs at both batch sizes):", "met" if ok else "MISSED")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
