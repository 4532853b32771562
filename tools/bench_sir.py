"""SIR measurements: the selection kernel next to the eager-torch op sequence it replaces, and
`ImportanceSamplingPosterior.sample` next to `MCMCPosterior.sample` on one trained NLE, all on the same GPU.

    python tools/bench_sir.py --out profiles/sir_bench.json

  * `select_B10000_K32_D10`, `select_B100_K10000_D10` -- one `sbi_amd_sir_resample` launch (uniforms drawn in the
        kernel) against the reference's sequence on the same log-weights and candidates: subtract, softmax, cumsum,
        rand, compare, cumsum, compare, boolean-mask gather (sbi/samplers/importance/sir.py:59-63; the gather
        synchronises with the host).  Both legs are timed with a host clock around `calls` back-to-back calls that end in
        a device synchronise, the two legs alternating, median over the repetitions, after a warm-up of both.
  * `posterior_sample_100000` -- `ImportanceSamplingPosterior.sample((100_000,))` (32 candidates per draw, prior as
        proposal) against `MCMCPosterior.sample((100_000,))` with the trainer's default MCMC parameters, on an NLE
        trained for a few epochs on the 2-d linear-Gaussian task.  The two do not return the same thing -- SIR draws are
        independent and approximate (bias O(1 / K)), MCMC draws are correlated and asymptotically exact -- so the ratio
        is the price of a draw, not of an effective sample.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _alternating_median_ms(fns, calls, reps, warm=3):
    """Median wall time per call (ms) of each function: `calls` back-to-back calls then a synchronise, alternating."""
    import torch

    for _ in range(warm):
        for fn in fns:
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) * 1e3 / calls)
    return [sorted(t)[len(t) // 2] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions and a smaller posterior leg")
    ap.add_argument("--skip-posterior", action="store_true")
    a = ap.parse_args()
    import torch

    from sbi_amd.samplers.importance.sir import sir_select

    if not torch.cuda.is_available():
        raise SystemExit("bench_sir.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    reps, calls = (5, 20) if a.quick else (15, 100)
    torch.manual_seed(0)
    for B, K, D in ((10_000, 32, 10), (100, 10_000, 10)):
        log_p = torch.randn(B, K, device="cuda") * 3
        log_q = torch.randn(B, K, device="cuda")
        cand = torch.randn(B, K, D, device="cuda")
        state = {"row": 0}

        def hip():
            state["row"] += B
            return sir_select(log_p, log_q, cand, None, 1234, state["row"])[0]

        def eager():
            weights = (log_p - log_q).softmax(-1).cumsum(-1)
            u = torch.rand(B, 1, device="cuda")
            mask = torch.cumsum(weights >= u, -1) == 1
            return cand[mask]

        t_hip, t_eager = _alternating_median_ms([hip, eager], calls, reps)
        put(f"select_B{B}_K{K}_D{D}", B=B, K=K, D=D, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
            calls_per_window=calls, repetitions=reps)

    if not a.skip_posterior:
        import warnings

        from sbi_amd.inference import NLE, ImportanceSamplingPosterior
        from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential
        from sbi_amd.simulators.linear_gaussian import linear_gaussian
        from sbi_amd.utils import BoxUniform

        dim = 2
        n = 20_000 if a.quick else 100_000
        prior = BoxUniform(-2.0 * torch.ones(dim), 2.0 * torch.ones(dim), device="cuda")
        theta = prior.sample((2000,)).cpu()
        x = linear_gaussian(theta, -0.5 * torch.ones(dim), 0.5 * torch.eye(dim))
        inf = NLE(prior=prior, density_estimator="nsf", device="cuda", show_progress_bars=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = inf.append_simulations(theta, x).train(max_num_epochs=20)
        x_o = torch.zeros(1, dim)
        potential_fn, transform = likelihood_estimator_based_potential(est, prior, None)
        sir = ImportanceSamplingPosterior(potential_fn, prior, theta_transform=transform).set_default_x(x_o)
        mcmc = inf.build_posterior(sample_with="mcmc").set_default_x(x_o)

        def timed(fn, reps):
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return sorted(ts)[len(ts) // 2], out

        sir.sample((1000,))                                                   # warm-up of both routes
        mcmc.sample((1000,), show_progress_bars=False)
        t_sir, s_sir = timed(lambda: sir.sample((n,)), 5)
        t_mcmc, s_mcmc = timed(lambda: mcmc.sample((n,), show_progress_bars=False), 1 if a.quick else 3)
        put(f"posterior_sample_{n}", draws=n, sir_s=t_sir, mcmc_s=t_mcmc, speedup=t_mcmc / t_sir,
            sir_mean=s_sir.mean(0).tolist(), mcmc_mean=s_mcmc.mean(0).tolist(),
            sir_std=s_sir.std(0).tolist(), mcmc_std=s_mcmc.std(0).tolist())
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
