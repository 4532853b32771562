"""Misspecification-test measurement: `calculate_baseline_mmd` (one `sbi_amd_mmd_rbf_splits` launch for all shuffles)
next to the eager-torch per-shuffle loop it replaces, on the same GPU.

    python tools/bench_mmd.py --out profiles/mmd_bench.json

Defaults are the reference's: 1000 shuffles of 1000 samples, D = 10, 100 observations, from a pool of 5000 rows.  The
eager leg is the loop of sbi/diagnostics/misspecification.py:56-86 restated on device tensors: per shuffle a randperm,
three cdist, a median read back by the host, three exp + mean.  Each leg is timed with a host clock around `calls`
back-to-back calls that end in a device synchronise; the two legs alternate; the figure is the median over the
repetitions, after a warm-up of both.  The two legs draw different shuffles (a keyed permutation against randperm), so
their outputs agree in distribution only; the means of both are recorded next to the times.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _alternating_median_ms(fns, calls, reps, warm=2):
    import torch

    for _ in range(warm):
        for fn, c in zip(fns, calls):
            for _ in range(c):
                fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, (fn, c) in enumerate(zip(fns, calls)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(c):
                fn()
            torch.cuda.synchronize()
            times[i].append((time.perf_counter() - t0) * 1e3 / c)
    return [sorted(t)[len(t) // 2] for t in times], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-shuffle", type=int, default=1000)
    ap.add_argument("--max-samples", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--n-obs", type=int, default=100)
    ap.add_argument("--pool", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch

    from sbi_amd.diagnostics import calculate_baseline_mmd

    if not torch.cuda.is_available():
        raise SystemExit("bench_mmd.py measures on a ROCm device; none is visible")
    torch.manual_seed(0)
    y = 2 * torch.randn(a.pool, a.dim, device="cuda") + 1
    last = {}

    def hip():
        last["hip"] = calculate_baseline_mmd(a.n_obs, y, n_shuffle=a.n_shuffle, max_samples=a.max_samples, seed=7)

    def eager():
        mmds = torch.zeros(a.n_shuffle)
        for i in range(a.n_shuffle):
            idx = torch.randperm(y.shape[0], device="cuda")[:a.max_samples]
            p, q = y[idx[:a.n_obs]], y[idx[a.n_obs:]]
            bw = torch.median(torch.cdist(p, q)).item()
            k = lambda u, v: torch.exp(-(torch.cdist(u, v) ** 2) / (2.0 * bw**2)).mean()
            mmds[i] = k(p, p) + k(q, q) - 2 * k(p, q)
        last["eager"] = mmds

    (t_hip, t_eager), raw = _alternating_median_ms([hip, eager], [10, 1], a.reps)
    res = {
        "device": torch.cuda.get_device_name(0),
        "n_shuffle": a.n_shuffle, "max_samples": a.max_samples, "dim": a.dim, "n_obs": a.n_obs, "pool": a.pool,
        "hip_ms": t_hip, "eager_ms": t_eager, "speedup": t_eager / t_hip,
        "hip_ms_all": raw[0], "eager_ms_all": raw[1],
        "calls_per_window": {"hip": 10, "eager": 1}, "repetitions": a.reps,
        "hip_mean_mmd": last["hip"].mean().item(), "eager_mean_mmd": last["eager"].mean().item(),
        "method": "host clock around back-to-back calls ending in a device synchronise; legs alternate; medians",
    }
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
