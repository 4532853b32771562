"""NPSE measurements: the fused score-matching training step next to the FMPE step of the same run, and the fused
Euler-Maruyama sampler next to the host loop over the score kernel and eager torch.

    python tools/bench_npse.py --out profiles/npse_bench.json

Shapes: theta-dim = x-dim = 10, sbi's default score network (hidden 100, 5 layers, time embedding 32), VE SDE.
  * `step`    -- one FusedNPSEStep.step (draws, DSM forward + stash with the control variate's second column, backward,
                 fixed-order weight-gradient reduction, clip + Adam) at batch 200 and 65 536, alternated with
                 FusedFMPEStep.step on the same tensors: the yardstick for what the second forward and the DSM epilogue
                 cost;
  * `sample`  -- 10^4 and 10^6 posterior draws at 500 Euler-Maruyama steps: `sbi_amd_npse_sample_sde` (one launch),
                 the host loop over `sbi_amd_npse_score` (one launch + the update per step) and eager torch evaluating
                 the restatement tests/npse_oracle.py on the same GPU (what the reference's Python loop does).
Device times are medians over CUDA events after a warm-up of the same leg (the device ramps its clock after idling);
compared legs alternate inside one timed sequence.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _median_ms_alternating(fns, reps, warm):
    """Medians of several legs timed in alternation (A B A B ...), so clock and neighbours hit all of them alike."""
    import torch

    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in ts]


def net_flops(n, D, C, H=100, L=5, E=32):
    """Forward multiply-adds x 2 of the vector-field MLP for n rows."""
    return 2.0 * n * (D * H + C * H + 2 * H * H + E * H + L * H * H + H * D)


def bench_step(res):
    import torch

    from sbi_amd.inference.trainers.fused import FusedFMPEStep, FusedNPSEStep
    from sbi_amd.neural_nets import build_score_matching_estimator
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import build_flow_matching_estimator

    D = C = 10
    for B in (200, 65536):
        torch.manual_seed(0)
        theta = torch.randn(B, D)
        x = theta + 0.5 * torch.randn(B, C)
        sc = build_score_matching_estimator(theta, x, sde_type="ve").to("cuda")
        fm = build_flow_matching_estimator(theta, x).to("cuda")
        th, xx = theta.cuda(), x.cuda()
        s_np, s_fm = FusedNPSEStep(sc), FusedFMPEStep(fm)
        s_nocv = FusedNPSEStep(sc)
        s_nocv.control_variate_threshold = 0.0
        t_np, t_fm, t_nocv = _median_ms_alternating(
            [lambda: s_np.step(th, xx), lambda: s_fm.step(th, xx), lambda: s_nocv.step(th, xx)],
            reps=60 if B == 200 else 20, warm=15 if B == 200 else 5)
        flop = 3 * net_flops(2 * B, D, C)
        res[f"step_B{B}"] = dict(batch=B, npse_ms=t_np, fmpe_ms=t_fm, npse_over_fmpe=t_np / t_fm,
                                 npse_without_control_variate_ms=t_nocv, tflops_npse=flop / (t_np * 1e-3) / 1e12,
                                 fp32_peak_fraction=flop / (t_np * 1e-3) / 157.3e12)
        print(json.dumps(res[f"step_B{B}"]), flush=True)


def bench_sample(res, big):
    import torch

    from sbi_amd.neural_nets import build_score_matching_estimator
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_fused, sample_sde_loop
    from tests.npse_oracle import NPSEOracle

    D = C = 10
    steps = 500
    torch.manual_seed(0)
    theta = torch.randn(2000, D)
    x = theta + 0.5 * torch.randn(2000, C)
    est = build_score_matching_estimator(theta, x, sde_type="ve")
    with torch.no_grad():
        est.net.flat_params.add_(0.05 * torch.randn_like(est.net.flat_params))
    oracle = NPSEOracle(D, C, sde="ve")
    oracle.load_reference_state_dict(est.reference_state_dict())
    est, oracle = est.to("cuda"), oracle.to("cuda")
    xo = x[:1].cuda()
    ts = est.solve_schedule(steps + 1)
    for n in (10**4, 10**6) if big else (10**4,):
        reps, warm = (10, 3) if n == 10**4 else (3, 1)
        with torch.no_grad():
            t_fused, t_loop, t_eager = _median_ms_alternating(
                [lambda: sample_sde_fused(est, n, xo, ts, 1.0, None, seed=1),
                 lambda: sample_sde_loop(est, n, xo, ts, 1.0),
                 lambda: oracle.sample_sde(xo, ts, None, 1.0, n=n)], reps=reps, warm=warm)
        flop = steps * net_flops(n, D, C)
        res[f"sample_{n}"] = dict(draws=n, steps=steps, fused_ms=t_fused, host_loop_ms=t_loop, eager_torch_ms=t_eager,
                                  fused_over_host_loop=t_loop / t_fused, fused_over_eager=t_eager / t_fused,
                                  draws_per_s_fused=n / (t_fused * 1e-3), tflops_fused=flop / (t_fused * 1e-3) / 1e12,
                                  fp32_peak_fraction=flop / (t_fused * 1e-3) / 157.3e12)
        print(json.dumps(res[f"sample_{n}"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["step", "sample"], default=None)
    ap.add_argument("--no-big", action="store_true", help="skip the 10^6-draw leg")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_npse.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only in (None, "step"):
        bench_step(res)
    if a.only in (None, "sample"):
        bench_sample(res, not a.no_big)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
