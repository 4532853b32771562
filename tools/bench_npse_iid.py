"""NPSE with iid observations: the fused compositional-score sampler next to the two ways of doing without it, on one GPU.

    python tools/bench_npse_iid.py --out profiles/npse_iid_bench.json

Three legs draw n posterior samples given N observations with `steps` Euler-Maruyama steps (auto_gauss-style dense
precisions, MultivariateNormal prior, sbi's default score net H = 100, L = 5, VE):
  * fused  -- `sample_sde_iid_fused`: one launch for all steps (plus the condition prologue);
  * loop   -- `sample_sde_iid_loop`: per step one `sbi_amd_npse_score` launch on the n N expanded rows, the per-row
              composition kernel and the update in torch;
  * eager  -- the per-call restatement of sbi's `IIDScoreFunction.__call__` in eager torch on the device
              (tests/npse_iid_oracle.py: N score evaluations, inverses, eigh and a solve per step).
Shapes (n, N, steps, D = C): (10000, 10, 500, 10) and (1000, 100, 500, 10).  Method of tools/bench_sir.py: host clock
around a call that ends in a device synchronise, the legs alternating, median over the repetitions, after a warm-up.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _alternating_median_ms(fns, reps, warm=1):
    import torch

    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) * 1e3)
    return [sorted(t)[len(t) // 2] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--skip-eager", action="store_true")
    a = ap.parse_args()
    import torch

    from sbi_amd.inference.potentials.vector_field_adaptor import AutoGaussCorrectedScoreFn
    from sbi_amd.neural_nets import build_score_matching_estimator
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_iid_fused, sample_sde_iid_loop
    from tests.npse_iid_oracle import make_prior, random_prior_spec, sample_iid
    from tests.npse_oracle import NPSEOracle

    if not torch.cuda.is_available():
        raise SystemExit("bench_npse_iid.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "reps": a.reps}
    D = C = 10
    torch.manual_seed(0)
    theta = torch.randn(512, D)
    x = theta + 0.5 * torch.randn(512, C)
    est = build_score_matching_estimator(theta, x, sde_type="ve")
    with torch.no_grad():
        est.net.flat_params.add_(0.02 * torch.randn_like(est.net.flat_params))
    oracle = NPSEOracle(D, C, sde="ve")
    oracle.load_reference_state_dict(est.reference_state_dict())
    oracle = oracle.cuda()
    oracle._base = tuple(b.cuda() for b in oracle._base)
    est = est.cuda()
    spec = random_prior_spec(D, 1)
    ts = est.solve_schedule(a.steps + 1)
    for n, N in ((10_000, 10), (1_000, 100)):
        B = torch.randn(N, D, D, dtype=torch.float64) * 0.3
        prec = B @ B.transpose(1, 2) + 2.0 * torch.eye(D, dtype=torch.float64)
        fn = AutoGaussCorrectedScoreFn(est, make_prior("mvn", spec), device="cuda")
        fn.posterior_precision_est_fn = lambda conditions: prec
        xs = x[:N].cuda().contiguous()
        t0 = time.perf_counter()
        tb = fn.tables(ts[:-1].cpu(), xs)
        tables_ms = (time.perf_counter() - t0) * 1e3
        lam, mats, vecs = tb.on("cuda")
        noise = torch.randn(a.steps + 1, n, D, device="cuda")

        def fused():
            return sample_sde_iid_fused(est, n, xs, ts, lam, mats, vecs, 1.0, noise)

        def loop():
            return sample_sde_iid_loop(est, n, xs, ts, lam, mats, vecs, 1.0, noise)

        def eager():
            return sample_iid(oracle, "auto_gauss", "mvn", spec, xs, ts, noise, prec=prec)

        legs = [fused, loop] + ([] if a.skip_eager else [eager])
        agree = float((fused() - loop()).abs().max())
        t = _alternating_median_ms(legs, a.reps)
        row = dict(n=n, N=N, D=D, fused_ms=t[0], loop_ms=t[1], loop_over_fused=t[1] / t[0], host_tables_ms=tables_ms,
                   fused_vs_loop_max_abs=agree)
        if not a.skip_eager:
            row.update(eager_ms=t[2], eager_over_fused=t[2] / t[0])
        res[f"n{n}_N{N}"] = row
        print(f"n{n}_N{N}", json.dumps(row), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
