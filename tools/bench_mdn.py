"""MDN measurements: every figure next to the eager-torch restatement (tests/mdn_oracle.py) on the same GPU.

    python tools/bench_mdn.py --out profiles/mdn_bench.json

Shapes: theta-dim = x-dim = 10, sbi's defaults (hidden 50, 10 components).
  * `step_B200`, `step_B65536` -- one FusedMDNStep.step (re-pack, fused loss forward + backward, fixed-order
        weight-gradient reduction, clip + Adam) against the restatement's loss, autograd, clip_grad_norm_ and Adam;
  * `log_prob_paired_65536`    -- 65 536 (theta, x) pairs;
  * `log_prob_one_x_65536`     -- 65 536 theta at one x_o (the network runs once per workgroup);
  * `sample_one_x_1e6`         -- 10^6 draws at one x_o (uniforms and normals drawn outside the timed region on both
                                  sides: the restatement gets its component indices from the same uniforms);
  * `sample_paired_65536`      -- our own paired sampler at 65 536 rows (the one-x_o figures must beat the paired ones).
Device times are medians over CUDA events after a warm-up of the same leg (the device ramps its clock after idling).
"""
import argparse
import json
import sys
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

    from sbi_amd.inference.trainers.fused import FusedMDNStep
    from sbi_amd.neural_nets.estimators.mdn import mdn_log_prob_call, mdn_sample_call
    from sbi_amd.neural_nets.net_builders.mdn import build_mdn
    from tests.mdn_oracle import MDNOracle

    reps = 5 if a.quick else 30

    def eager_ms(fn, **kw):       # the restatement's legs (skipped by --hip-only)
        return float("nan") if a.hip_only else _median_ms(fn, **kw)

    D = C = 10
    res = {"device": torch.cuda.get_device_name(0), "D": D, "C": C, "hidden_features": 50, "num_components": 10}
    torch.manual_seed(0)
    theta = torch.randn(65536, D)
    x = theta + 0.5 * torch.randn(65536, C)
    est = build_mdn(theta, x).cuda()
    oracle = MDNOracle(D, C)
    oracle.set_zstats(est.net.zstats.cpu())
    oracle.load_state_dict(est.state_dict())
    oracle = oracle.cuda()
    th, xx = theta.cuda(), x.cuda()

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    for B in (200, 65536):
        e = build_mdn(theta, x).cuda()
        step = FusedMDNStep(e)
        tb, xb = th[:B].contiguous(), xx[:B].contiguous()
        t_hip = _median_ms(lambda: step.step(tb, xb), reps=reps)
        o = MDNOracle(D, C)
        o.set_zstats(e.net.zstats.cpu())
        o = o.cuda()
        opt = torch.optim.Adam(o.parameters(), lr=5e-4)

        def eager():
            opt.zero_grad()
            o.loss(tb, xb).mean().backward()
            torch.nn.utils.clip_grad_norm_(o.parameters(), 5.0)
            opt.step()

        t_eager = eager_ms(eager, reps=reps)
        put(f"step_B{B}", batch=B, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip)

    with torch.no_grad():
        N = 65536
        t_hip = _median_ms(lambda: mdn_log_prob_call(est.net, th, xx), reps=reps)
        t_eager = eager_ms(lambda: oracle.log_prob(th, xx), reps=reps)
        put("log_prob_paired_65536", rows=N, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip)
        x1 = xx[:1].contiguous()
        t_one = _median_ms(lambda: mdn_log_prob_call(est.net, th, x1), reps=reps)
        t_eager = eager_ms(lambda: oracle.log_prob(th[:, None], x1), reps=reps)
        put("log_prob_one_x_65536", rows=N, hip_ms=t_one, eager_ms=t_eager, speedup=t_eager / t_one,
            paired_hip_ms=t_hip, speedup_vs_paired=t_hip / t_one)

        u = torch.rand(N, device="cuda")
        zeta = torch.randn(N, D, device="cuda")
        t_pair = _median_ms(lambda: mdn_sample_call(est.net, zeta, xx, u=u), reps=reps)
        t_one = _median_ms(lambda: mdn_sample_call(est.net, zeta, x1, u=u), reps=reps)
        put("sample_paired_65536", rows=N, hip_ms=t_pair, one_x_hip_ms=t_one, speedup_one_x_vs_paired=t_pair / t_one)

        M = 10**6
        u = torch.rand(M, device="cuda")
        zeta = torch.randn(M, D, device="cuda")
        t_hip = _median_ms(lambda: mdn_sample_call(est.net, zeta, x1, u=u), reps=reps)

        def eager_sample():
            comp = torch.searchsorted(oracle.cumulative_weights(x1)[0].contiguous(), u, right=True).clamp(max=9)
            return oracle.sample_given(comp, zeta, x1)

        t_eager = eager_ms(eager_sample, reps=max(3, reps // 3), warm=3)
        put("sample_one_x_1e6", draws=M, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
            draws_per_s=M / (t_hip * 1e-3))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
