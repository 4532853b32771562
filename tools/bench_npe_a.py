"""NPE-A measurements: the three mixture kernels next to the package's own eager-torch route (the same formulas,
sbi_amd/neural_nets/estimators/mog_ops.py `*_eager`) on the same GPU.

    python tools/bench_npe_a.py --out profiles/npe_a_bench.json

  * `correct_B1_K10_L100_D10`, `correct_B1000_K10_L10_D10` -- one `sbi_amd_mog_correct` call (three launches) against
        `correct_eager`: one observation against a 100-component proposal (round 3 at the default K), and 1000
        observations against one 10-component proposal (`sample_batched` / SBC in round 2).
  * `log_prob_n1000000_M100`, `log_prob_n1000000_M1000` -- `sbi_amd_mog_log_prob` of 10^6 theta under one mixture
        (the MFMA kernel) against `log_prob_eager`, which walks the rows in chunks of 2^24 / (M D).
  * `sample_n1000000_M1000` -- `sbi_amd_mog_sample` (cumulative table + binary search + back-substitution) against
        `sample_eager` (fp64 softmax / cumsum / searchsorted, gather, `solve_triangular`), uniforms and normals given.

Both legs are timed with a host clock around `calls` back-to-back calls that end in a device synchronise, the two legs
alternating, median over the repetitions, after a warm-up of both (as tools/bench_sir.py).
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets.estimators import mog_ops

    if not torch.cuda.is_available():
        raise SystemExit("bench_npe_a.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    def mixture(g, B, K, D, lo, hi, mean_scale):
        A = torch.triu(torch.randn(B, K, D, D, generator=g), 1) * (0.5 * lo / D)
        i = torch.arange(D)
        A[..., i, i] = torch.rand(B, K, D, generator=g) * (hi - lo) + lo
        return [t.cuda().contiguous() for t in (torch.randn(B, K, generator=g),
                                                mean_scale * torch.randn(B, K, D, generator=g),
                                                A.transpose(-1, -2) @ A, A)]

    g = torch.Generator().manual_seed(0)
    reps = 5 if a.quick else 11
    for B, K, L, D, calls in ((1, 10, 100, 10, 20), (1000, 10, 10, 10, 5)):
        d, p = mixture(g, B, K, D, 2.0, 4.0, 0.5), mixture(g, 1, L, D, 0.5, 1.0, 0.5)
        _, m0, P0, _ = mixture(g, 1, 1, D, 0.2, 0.3, 0.1)
        args = (d[0], d[1], d[2], p[0], p[1], p[2], m0[0, 0].contiguous(), P0[0, 0].contiguous())
        t_hip, t_eager = _alternating_median_ms([lambda: mog_ops.correct_kernel(*args),
                                                 lambda: mog_ops.correct_eager(*args)], calls, reps)
        put(f"correct_B{B}_K{K}_L{L}_D{D}", B=B, K=K, L=L, D=D, hip_ms=t_hip, eager_ms=t_eager,
            speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps)

    n, D = 1_000_000, 10
    theta = (0.6 * torch.randn(n, D, generator=g)).cuda()
    zeta = torch.randn(n, D, generator=g).cuda()
    u = torch.rand(n, generator=g).cuda()
    shift, scale = (0.3 * torch.randn(D, generator=g)).cuda(), (0.5 + torch.rand(D, generator=g)).cuda()
    for M in (100, 1000):
        d, p = mixture(g, 1, 10, D, 2.0, 4.0, 0.5), mixture(g, 1, M // 10, D, 0.5, 1.0, 0.5)
        mix = mog_ops.correct_kernel(d[0], d[1], d[2], p[0], p[1], p[2])[:4]
        t_hip, t_eager = _alternating_median_ms(
            [lambda: mog_ops.log_prob_kernel(*mix, theta, shift, scale),
             lambda: mog_ops.log_prob_eager(*mix, theta, shift, scale)], 1, reps, warm=1)
        put(f"log_prob_n{n}_M{M}", n=n, M=M, D=D, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
            calls_per_window=1, repetitions=reps)
    t_hip, t_eager = _alternating_median_ms(
        [lambda: mog_ops.sample_kernel(mix[0], mix[1], mix[3], zeta, u, None, shift, scale),
         lambda: mog_ops.sample_eager(mix[0], mix[1], mix[3], zeta, u, None, shift, scale)], 1, reps, warm=1)
    put(f"sample_n{n}_M1000", n=n, M=1000, D=D, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
        calls_per_window=1, repetitions=reps)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
