"""NLE measurements: the iid-trials likelihood kernel and the MCMC tick on NLE's potential.

    python tools/bench_nle.py --out profiles/nle_bench.json

Part 1 (default config, x-dim = theta-dim = 10): for (num_theta, num_trials) in {(20, 1), (20, 100), (10 000, 1),
(10 000, 100)}, the median device time of
  * `trials`  -- sbi_amd_nsf_log_prob_trials (per-row kernel + the fixed-order sum), nothing materialised;
  * `generic` -- the reference's path: expand x_o to (num_trials, num_theta, D), batched log_prob, sum over trials;
  * `paired`  -- sbi_amd_nsf_log_prob alone on the same rows, materialised beforehand (the yardstick of the kernel).
Part 2: an NLE trained once on the linear Gaussian (dim 10, 5 trials of x_o), then MCMCPosterior.sample with 20 and
100 chains, the fused tick (trials kernel + tick kernel) against the generic potential: wall time per tick.  The
kernels launched per tick come from `rocprofv3 --kernel-trace --stats` over two child runs that differ only in the
number of samples (the difference of the dispatch counts over the difference of the ticks).
Every GPU step runs in a child process with its own time limit.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = [(20, 1), (20, 100), (10_000, 1), (10_000, 100)]
DIM = 10
NUM_TRIALS_MCMC = 5


def _median_ms(fn, reps=30, warm=5):
    import torch

    for _ in range(warm):
        fn()
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


def kernels():
    import torch

    from sbi_amd.inference.potentials.likelihood_based_potential import log_likelihoods_over_trials_generic
    from sbi_amd.neural_nets.estimators.nsf_flow import _log_prob_call, log_prob_trials_call
    from sbi_amd.neural_nets.net_builders.flow import build_nsf

    torch.manual_seed(0)
    est = build_nsf(torch.randn(1000, DIM), torch.randn(1000, DIM)).to("cuda")
    est.eval()
    out = []
    for num_theta, num_trials in SHAPES:
        x_o = torch.randn(num_trials, DIM, device="cuda")
        theta = torch.randn(num_theta, DIM, device="cuda")
        x_mat = x_o.repeat(num_theta, 1).contiguous()
        th_mat = theta.repeat_interleave(num_trials, dim=0).contiguous()
        with torch.no_grad():
            t_trials = _median_ms(lambda: log_prob_trials_call(est.net, x_o, theta))
            t_generic = _median_ms(lambda: log_likelihoods_over_trials_generic(x_o, theta, est))
            t_paired = _median_ms(lambda: _log_prob_call(est.net, x_mat, th_mat, False))
        row = dict(num_theta=num_theta, num_trials=num_trials, rows=num_theta * num_trials, trials_ms=t_trials,
                   generic_ms=t_generic, paired_ms=t_paired, trials_over_paired=t_trials / t_paired)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def _trained_estimator(path):
    import torch
    from torch.distributions import MultivariateNormal

    from sbi_amd.inference import NLE
    from sbi_amd.neural_nets import likelihood_nn
    from sbi_amd.simulators.linear_gaussian import linear_gaussian

    torch.manual_seed(0)
    prior = MultivariateNormal(torch.zeros(DIM, device="cuda"), torch.eye(DIM, device="cuda"))
    theta = prior.sample((5000,)).cpu()
    x = linear_gaussian(theta, -1.0 * torch.ones(DIM), 0.8 * torch.eye(DIM))
    inf = NLE(prior=prior, density_estimator=likelihood_nn("nsf"), device="cuda", show_progress_bars=False)
    est = inf.append_simulations(theta, x).train(max_num_epochs=40)
    torch.save(est, path)


def _sample(est_path, chains, num_samples, fused):
    """One MCMC run; returns (ticks, seconds of the chain loop)."""
    import torch
    from torch.distributions import MultivariateNormal

    from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
    from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential

    est = torch.load(est_path, weights_only=False)
    prior = MultivariateNormal(torch.zeros(DIM, device="cuda"), torch.eye(DIM, device="cuda"))
    x_o = torch.zeros(NUM_TRIALS_MCMC, DIM, device="cuda")
    pot, tf = likelihood_estimator_based_potential(est, prior, x_o)
    post = MCMCPosterior(pot, prior, tf, num_chains=chains, thin=1, warmup_steps=10, init_strategy="resample",
                         device="cuda")
    if not fused:       # the reference's path: no fused tick, and the potential expands x_o against every theta
        from sbi_amd.inference.potentials.likelihood_based_potential import log_likelihoods_over_trials_generic

        post._fused_potential = lambda: None
        pot.log_likelihood_over_trials = lambda th, tg=False: log_likelihoods_over_trials_generic(pot.x_o, th, est, tg)
    timing = {}
    inner = post._slice_np_mcmc

    def timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*a, **k)
        torch.cuda.synchronize()
        timing["s"] = time.perf_counter() - t0
        return r

    post._slice_np_mcmc = timed
    post.set_default_x(x_o)
    post.sample((40,), show_progress_bars=False)              # warm-up: module loads, weight packing
    ticks = post.posterior_sampler.num_ticks
    post.sample((num_samples,), show_progress_bars=False)
    last = post.posterior_sampler.num_ticks
    return ticks + last, last, timing["s"]


def _child(args):
    total, ticks, secs = _sample(args.est, args.chains, args.num_samples, args.mode == "fused")
    print(json.dumps(dict(total_ticks=total, ticks=ticks, seconds=secs)), flush=True)


def _run(cmd, limit):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError(f"{cmd[0]} ... exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def _kernel_calls(stats_dir):
    total = 0
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"no kernel_stats.csv under {stats_dir}")
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                total += int(row["Calls"])
    return total


def mcmc(est_path, prof_dir):
    out = []
    me = [sys.executable, str(Path(__file__).resolve())]
    for mode in ("fused", "generic"):
        for chains in (20, 100):
            res = json.loads(_run(me + ["--child", "--est", est_path, "--mode", mode, "--chains", str(chains),
                                        "--num-samples", "400"], 600).strip().splitlines()[-1])
            row = dict(mode=mode, chains=chains, ticks=res["ticks"], ms_per_tick=1e3 * res["seconds"] / res["ticks"])
            print(json.dumps(row), flush=True)
            out.append(row)
    counts = {}
    for mode in ("fused", "generic"):
        pts = []
        for ns in (100, 400):
            d = os.path.join(prof_dir, f"{mode}_{ns}")
            so = _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--"] + me +
                      ["--child", "--est", est_path, "--mode", mode, "--chains", "20", "--num-samples", str(ns)], 900)
            res = json.loads([ln for ln in so.splitlines() if ln.startswith("{")][-1])
            pts.append((res["total_ticks"], _kernel_calls(d)))
        (t0, c0), (t1, c1) = pts
        counts[mode] = dict(ticks=[t0, t1], dispatches=[c0, c1], kernels_per_tick=(c1 - c0) / (t1 - t0))
        print(json.dumps({mode: counts[mode]}), flush=True)
    return out, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--est")
    ap.add_argument("--mode", default="fused")
    ap.add_argument("--chains", type=int, default=20)
    ap.add_argument("--num-samples", type=int, default=400)
    ap.add_argument("--skip-mcmc", action="store_true")
    args = ap.parse_args()
    if args.child:
        return _child(args)
    import torch

    result = dict(device=torch.cuda.get_device_name(0), kernels=kernels())
    if not args.skip_mcmc:
        with tempfile.TemporaryDirectory() as tmp:
            est_path = os.path.join(tmp, "nle_estimator.pt")
            _trained_estimator(est_path)
            result["mcmc"], result["mcmc_kernels_per_tick"] = mcmc(est_path, os.path.join(tmp, "prof"))
            if args.out:        # keep one kernel-stats table per mode next to the JSON
                for mode in ("fused", "generic"):
                    f = glob.glob(os.path.join(tmp, "prof", f"{mode}_400", "**", "*kernel_stats.csv"), recursive=True)
                    if f:
                        Path(args.out).with_name(f"nle_tick_{mode}_kernel_stats.csv").write_text(Path(f[0]).read_text())
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
