"""ABC measurement: the three hot paths on their kernels next to the package's own eager-torch fallback of the same
formulas, on the same GPU.

    python tools/bench_abc.py --out profiles/abc_bench.json

Legs (each: the device route and `force_fallback=True`):
  * smc_weights  -- the SMC-ABC weight update of one population: `SMCABC.kernel_log_mixture` for N new against N old
                    particles (one `sbi_amd_mixture_lse` launch; the reference loops over the particles in Python,
                    which the fallback here already does not);
  * kde_cv       -- `cv_bandwidth` (the zoom search of get_kde(bandwidth="cv"), 20 folds x 10 bandwidths per launch);
  * wasserstein  -- `wasserstein_distance` of B simulated sets against one observed set at the reference's defaults
                    (eps 1e-3, 1000 iterations, tol 1e-9): one persistent `sbi_amd_sinkhorn` launch against up to 1000
                    iterations of eager launches with a host synchronisation each.
Each leg is timed with a host clock around calls that end in a device synchronise; device and fallback alternate; the
figure is the median over the repetitions after a warm-up of both.
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
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=5)
    ap.add_argument("--kde-samples", type=int, default=1000)
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--set-size", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from sbi_amd.inference import SMCABC
    from sbi_amd.utils import kde
    from sbi_amd.utils.metrics import _sinkhorn
    from sbi_amd.utils.torchutils import BoxUniform

    if not torch.cuda.is_available():
        raise SystemExit("bench_abc.py measures on a ROCm device; none is visible")
    torch.manual_seed(0)
    dev = "cuda"
    result = {"config": {k: v for k, v in vars(a).items() if k != "out"}}

    prior = BoxUniform(-5 * torch.ones(a.dim), 5 * torch.ones(a.dim), device=dev)
    smc = SMCABC(lambda t: t, prior, show_progress_bars=False)
    old, new = torch.randn(a.particles, a.dim, device=dev), torch.randn(a.particles, a.dim, device=dev)
    log_w = torch.log_softmax(torch.randn(a.particles, device=dev), 0)
    smc.kernel_variance = 2.0 * torch.eye(a.dim, device=dev)
    k, f = _alternating_median_ms([lambda: smc.kernel_log_mixture(new, old, log_w),
                                   lambda: smc.kernel_log_mixture(new, old, log_w, force_fallback=True)], a.reps)
    result["smc_weights"] = {"kernel_ms": k, "fallback_ms": f}

    samples = torch.randn(a.kde_samples, a.dim, device=dev)
    k, f = _alternating_median_ms([lambda: kde.cv_bandwidth(samples),
                                   lambda: kde.cv_bandwidth(samples, force_fallback=True)], a.reps)
    result["kde_cv"] = {"kernel_ms": k, "fallback_ms": f}

    x_o = torch.randn(a.set_size, 2, device=dev)
    x = torch.randn(a.sets, a.set_size, 2, device=dev) + 0.5
    k, f = _alternating_median_ms(
        [lambda: _sinkhorn(x_o, x, None, None, None, a.sets, 1e-3, 1000, 1e-9),
         lambda: _sinkhorn(x_o, x, None, None, None, a.sets, 1e-3, 1000, 1e-9, force_fallback=True)], a.reps)
    result["wasserstein"] = {"kernel_ms": k, "fallback_ms": f}

    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
