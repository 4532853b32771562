"""VIPosterior measurements: time per training iteration on the kernel route next to the eager route of the same
class, on the same GPU, plus `sample` and `log_prob` of 10^6 rows.

    python tools/bench_vi.py --out profiles/vi_bench.json

  * `iter_<potential>_<method>_n<particles>` -- D = 10, 256 and 4 096 particles, rKL and IW (K = 8).  One window is
        `iters` optimiser iterations then a device synchronise (the kernel route's read-back every 25 iterations
        included: it is part of the route), timed with a host clock; the two legs alternate, median over the
        repetitions, after a warm-up of both.  `analytic`: a Gaussian log-density potential, which isolates VI's own
        overhead; `nle`: the potential of an NLE (NSF) trained for a few epochs on the 10-d linear-Gaussian task.
  * `sample_1e6`, `log_prob_1e6` -- `LearnableGaussian.sample((10**6,))` / `.log_prob` of 10^6 rows, the kernels
        against the torch formulas (`force_eager`).
"""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

D = 10


def _alternating_median_ms(fns, reps, warm=2):
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


class GaussianPotential:
    def __init__(self, prior, device):
        import torch

        self.prior, self.device = prior, device
        g = torch.Generator().manual_seed(0)
        self.m = (0.5 * torch.randn(D, generator=g)).to(device)
        self.A = (0.4 * torch.eye(D) + 0.1 * torch.randn(D, D, generator=g).tril(-1)).to(device)

    def set_x(self, x_o, x_is_iid=True):
        self.x_o = x_o

    def to(self, device):
        return self

    def __call__(self, theta, track_gradients=True):
        import torch
        from torch.distributions import MultivariateNormal

        with torch.set_grad_enabled(track_gradients):
            return MultivariateNormal(self.m, scale_tril=self.A).log_prob(theta) + self.prior.log_prob(theta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip-nle", action="store_true")
    a = ap.parse_args()
    import torch

    from sbi_amd.inference import NLE, VIPosterior
    from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential
    from sbi_amd.simulators.linear_gaussian import linear_gaussian
    from sbi_amd.utils import BoxUniform

    if not torch.cuda.is_available():
        raise SystemExit("bench_vi.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0), "D": D}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    prior = BoxUniform(-3.0 * torch.ones(D), 3.0 * torch.ones(D), device="cuda")
    potentials = {"analytic": (GaussianPotential(prior, "cuda"), None)}
    if not a.skip_nle:
        torch.manual_seed(1)
        theta = prior.sample((2000,)).cpu()
        x = linear_gaussian(theta, -0.5 * torch.ones(D), 0.5 * torch.eye(D))
        inf = NLE(prior=prior, density_estimator="nsf", device="cuda", show_progress_bars=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = inf.append_simulations(theta, x).train(max_num_epochs=5)
        potentials["nle"] = likelihood_estimator_based_potential(est, prior, None)
    x_o = torch.zeros(1, D, device="cuda")
    iters, reps = (50, 5) if a.quick else (100, 9)
    for pname, (potential_fn, transform) in potentials.items():
        for method, kw in (("rKL", {}), ("IW", {"K": 8})):
            for n in (256, 4096):
                legs = []
                for eager in (False, True):
                    torch.manual_seed(2)
                    post = VIPosterior(potential_fn, prior, q="gaussian", vi_method=method, theta_transform=transform,
                                       device="cuda").set_default_x(x_o)
                    post.force_eager = eager
                    post.train(max_num_iters=25, n_particles=n, quality_control=False, show_progress_bar=False,
                               check_for_convergence=False, warm_up_rounds=5, **kw)
                    assert post._optimizer.kernel_route()[0] == (not eager)
                    legs.append(post)

                def window(post):
                    return lambda: post.train(max_num_iters=iters, n_particles=n, quality_control=False,
                                              show_progress_bar=False, check_for_convergence=False, **kw)

                t_hip, t_eager = _alternating_median_ms([window(legs[0]), window(legs[1])], reps)
                put(f"iter_{pname}_{method}_n{n}", particles=n, rows_per_step=n * kw.get("K", 1),
                    hip_ms_per_iter=t_hip / iters, eager_ms_per_iter=t_eager / iters, speedup=t_eager / t_hip,
                    iters_per_window=iters, repetitions=reps)

    post = VIPosterior(potentials["analytic"][0], prior, q="gaussian", device="cuda").set_default_x(x_o)
    q = post.q
    N = 10**6
    theta = q.sample((N,))

    def leg(fn, eager):
        def run():
            q.force_eager = eager
            with torch.no_grad():
                return fn()
        return run

    t_hip, t_eager = _alternating_median_ms([leg(lambda: q.sample((N,)), False), leg(lambda: q.sample((N,)), True)], 9)
    put("sample_1e6", hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip)
    t_hip, t_eager = _alternating_median_ms([leg(lambda: q.log_prob(theta), False), leg(lambda: q.log_prob(theta), True)],
                                            9)
    put("log_prob_1e6", hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip)
    q.force_eager = False
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
