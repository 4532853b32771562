"""Conditional-correlation measurement: `conditional_corrcoeff` on its device route (fill + one `log_prob` call + one
moments launch per chunk of whole grids) next to the package's own loop route (one grid per `log_prob` call, the same
fp64 formula as torch ops) on the same GPU.

    python tools/bench_conditional.py --out profiles/conditional_bench.json

An untrained NSF posterior at theta-dim 10 (sbi's default hyper-parameters), resolution 50, all 45 pairs, with 1 and
with 100 conditions.  Each leg is timed with a host clock around a call that ends in a device synchronise; the two legs
alternate; the figure is the median over the repetitions, after a warm-up of both.  Both routes evaluate the same theta
rows with the same kernel, so their matrices agree within the reduction's rounding; the largest difference is recorded
next to the times.
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
    return [sorted(t)[len(t) // 2] for t in times], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=50)
    ap.add_argument("--conditions", type=int, nargs="+", default=[1, 100])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from sbi_amd.analysis import conditional_corrcoeff
    from sbi_amd.analysis import conditional_density as cd
    from sbi_amd.inference.posteriors.direct_posterior import DirectPosterior
    from sbi_amd.neural_nets.net_builders.flow import build_nsf
    from sbi_amd.utils.torchutils import BoxUniform

    if not torch.cuda.is_available():
        raise SystemExit("bench_conditional.py measures on a ROCm device; none is visible")
    torch.manual_seed(0)
    D, R = a.dim, a.resolution
    est = build_nsf(torch.randn(1000, D), torch.randn(1000, D)).to("cuda")
    prior = BoxUniform(-3 * torch.ones(D, device="cuda"), 3 * torch.ones(D, device="cuda"))
    post = DirectPosterior(est, prior, device="cuda")
    post.set_default_x(torch.randn(1, D, device="cuda"))
    limits = torch.tensor([[-2.0, 2.0]] * D)
    shapes = []
    for C in a.conditions:
        condition = torch.rand(C, D) * 2 - 1
        last = {}

        def device_route():
            last["device"] = conditional_corrcoeff(post, limits, condition, resolution=R)

        def loop_route():
            cd.force_loop = True
            try:
                last["loop"] = conditional_corrcoeff(post, limits, condition, resolution=R)
            finally:
                cd.force_loop = False

        (t_dev, t_loop), raw = _alternating_median_ms([device_route, loop_route], a.reps)
        shapes.append({
            "conditions": C, "grids": C * D * (D - 1) // 2, "rows": C * D * (D - 1) // 2 * R * R,
            "device_ms": t_dev, "loop_ms": t_loop, "speedup": t_loop / t_dev,
            "device_ms_all": raw[0], "loop_ms_all": raw[1],
            "max_abs_difference": float((last["device"] - last["loop"]).abs().max()),
        })
        print(json.dumps(shapes[-1]), flush=True)
    res = {
        "device": torch.cuda.get_device_name(0), "dim": D, "resolution": R, "repetitions": a.reps, "shapes": shapes,
        "method": "host clock around one call ending in a device synchronise; legs alternate; medians; one warm-up each",
    }
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
