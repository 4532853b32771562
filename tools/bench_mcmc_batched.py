"""Batched MCMC and calibration diagnostics, measured on one MI355X.

    python tools/bench_mcmc_batched.py --out profiles/mcmc_batched_bench.json

  * `ticks`  -- batched slice sampling on the NRE potential (theta-dim = x-dim = 3, sbi's default classifier: hidden 50,
                2 blocks; box prior) at (observations, chains per observation) = (1, 20), (100, 20), (1 000, 20), one
                sampler run of the SAME chains (same seed, same init) per route: `generic` (the potential through torch,
                uniforms from torch), `two_launch` (sbi_amd_nre_log_ratio + prior + sbi_amd_mcmc_slice_tick) and
                `persistent_wgN` (sbi_amd_nre_mcmc_slice_run with N lanes per workgroup).  The legs alternate inside
                one timed sequence -- the device ramps its clock after idling, so a leg measured alone after a pause is
                not comparable -- after a warm-up round; medians over device events.  `ms_per_tick` divides by the
                ticks of the two-launch run: the fused routes walk identical chains, the persistent one only rounds
                its last launch up to `poll_every`.
  * `run_sbc` -- wall time of run_sbc (N = 1 000 observations, L = 1 000 draws each, "marginals") through the four
                posterior kinds (NPE direct, NLE MCMC, NRE MCMC, FMPE ODE) on briefly trained nets, split into sampling
                and ranking, next to the per-observation, per-parameter rank loop of sbi's `_run_sbc` restated on the
                host for the same samples.
  * `calibration` -- SBC / TARP (N = 200, L = 100) of a trained NRE_B through batched MCMC and of a trained NPE through
                the direct posterior with the expected-coverage reduce, each next to the same posterior asked about
                permuted observations.
"""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _box(dim):
    import torch

    from sbi_amd.utils.torchutils import BoxUniform

    return BoxUniform(-2.0 * torch.ones(dim), 2.0 * torch.ones(dim), device="cuda")


def _task(dim, n, seed=0):
    import torch

    from sbi_amd.simulators.linear_gaussian import linear_gaussian

    torch.manual_seed(seed)
    prior = _box(dim)
    theta = prior.sample((n,)).cpu()
    return prior, theta, linear_gaussian(theta, -1.0 * torch.ones(dim), 0.8 * torch.eye(dim))


def bench_ticks(res, sizes, reps, wgs):
    import torch

    from sbi_amd.inference import NRE_B
    from sbi_amd.inference.posteriors.mcmc_posterior import unconstrained_potential
    from sbi_amd.samplers.mcmc import SliceSamplerVectorized

    dim = 3
    prior, theta, x = _task(dim, 2000)
    inf = NRE_B(prior=prior, device="cuda", show_progress_bars=False)
    inf.append_simulations(theta, x).train(max_num_epochs=10)
    post = inf.build_posterior()
    out = {}
    for B, K in sizes:
        torch.manual_seed(1)
        xs = x[:B].cuda()
        post.potential_fn.set_x(xs.repeat_interleave(K, dim=0), x_is_iid=False)
        fused = post._fused_potential_batched(xs, K)
        generic = unconstrained_potential(post.potential_fn, post.theta_transform, "cuda")
        init = torch.randn(B * K, dim, device="cuda") * 0.3
        legs = {"generic": (generic, None, 0), "two_launch": (fused, False, 0)}
        legs.update({f"persistent_wg{wg}": (fused, True, wg) for wg in wgs})
        times = {name: [] for name in legs}
        ticks, routes = {}, {}
        for rep in range(reps + 1):                      # round 0 warms every leg up
            for name, (fn, persistent, wg) in legs.items():
                torch.manual_seed(5)
                s = SliceSamplerVectorized(fn, init.clone(), num_chains=B * K, thin=1, tuning=10, poll_every=64,
                                           persistent=persistent, nre_wg_size=wg)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                s.run(10)
                b.record()
                b.synchronize()
                if rep:
                    times[name].append(a.elapsed_time(b))
                ticks[name], routes[name] = s.num_ticks, s.route
        base = ticks["two_launch"]
        entry = {}
        for name, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            entry[name] = dict(route=routes[name], run_ms=med, ticks=ticks[name],
                               ms_per_tick=med / (ticks[name] if name == "generic" else base))
        two = entry["two_launch"]["run_ms"]
        for name in entry:
            entry[name]["vs_two_launch"] = two / entry[name]["run_ms"]
        out[f"B{B}_K{K}"] = entry
        print(f"B{B}_K{K}", json.dumps(entry), flush=True)
    res["ticks"] = out


def _host_rank_loop(thetas, samples):
    """The rank loop of sbi's `_run_sbc` for "marginals", restated: one comparison, sum and host read per observation
    and parameter, on host tensors."""
    import torch

    N, D = thetas.shape
    ranks = torch.zeros(N, D)
    for i in range(N):
        for d in range(D):
            ranks[i, d] = (samples[:, i, d] < thetas[i, d]).sum().item()
    return ranks


def bench_run_sbc(res, N, L):
    import torch

    from sbi_amd.diagnostics.sbc import _run_sbc
    from sbi_amd.inference import FMPE, NLE, NPE, NRE_B
    from sbi_amd.neural_nets import NSFConfig
    from sbi_amd.utils.diagnostics_utils import get_posterior_samples_on_batch

    dim = 3
    prior, theta, x = _task(dim, 3000)
    _, thetas, xs = _task(dim, N, seed=9)
    mcmc = dict(num_chains=20, thin=1, warmup_steps=50, init_strategy="resample",
                init_strategy_parameters=dict(num_candidate_samples=1000))
    makers = {
        "npe_direct": lambda: (NPE(prior=prior, density_estimator=NSFConfig(), device="cuda", show_progress_bars=False), {}),
        "nle_mcmc": lambda: (NLE(prior=prior, density_estimator="nsf", device="cuda", show_progress_bars=False),
                             dict(mcmc_parameters=mcmc)),
        "nre_mcmc": lambda: (NRE_B(prior=prior, device="cuda", show_progress_bars=False), dict(mcmc_parameters=mcmc)),
        "fmpe_ode": lambda: (FMPE(prior=prior, device="cuda", show_progress_bars=False), {}),
    }
    out = {}
    for name, make in makers.items():
        inf, kw = make()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            inf.append_simulations(theta, x).train(max_num_epochs=10)
            post = inf.build_posterior(**kw)
            get_posterior_samples_on_batch(xs[:50], post, (100,))          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samples = get_posterior_samples_on_batch(xs, post, (L,))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ranks = _run_sbc(thetas, xs, samples, "marginals")
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        host = samples.cpu()
        t3 = time.perf_counter()
        loop = _host_rank_loop(thetas, host)
        t4 = time.perf_counter()
        assert torch.equal(loop, ranks)
        out[name] = dict(N=N, L=L, sampling_s=t1 - t0, ranking_s=t2 - t1, run_sbc_s=t2 - t0, host_rank_loop_s=t4 - t3,
                         route=getattr(getattr(post, "posterior_sampler", None), "route", None))
        print(name, json.dumps(out[name]), flush=True)
    res["run_sbc"] = out


def bench_calibration(res):
    import torch

    from sbi_amd.diagnostics import check_tarp, run_sbc, run_tarp
    from sbi_amd.diagnostics.sbc import check_uniformity_frequentist
    from sbi_amd.inference import NPE, NRE_B
    from sbi_amd.neural_nets import NSFConfig

    dim, N, L = 2, 200, 100
    prior, theta, x = _task(dim, 3000)
    _, thetas, xs = _task(dim, N, seed=7)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nre = NRE_B(prior=prior, device="cuda", show_progress_bars=False)
        nre.append_simulations(theta, x).train(max_num_epochs=60)
        npe = NPE(prior=prior, density_estimator=NSFConfig(), device="cuda", show_progress_bars=False)
        npe.append_simulations(theta, x).train(training_batch_size=100, max_num_epochs=40)
        posts = {
            "nre_b_batched_mcmc": (nre.build_posterior(mcmc_parameters=dict(
                num_chains=20, thin=2, warmup_steps=50, init_strategy="resample",
                init_strategy_parameters=dict(num_candidate_samples=1000))), "marginals"),
            "npe_direct_expected_coverage": (npe.build_posterior(), None),
        }
        perm = torch.randperm(N)
        for name, (post, fns) in posts.items():
            fns = post.log_prob if fns is None else fns
            entry = {}
            for tag, obs in (("trained", xs), ("permuted_observations", xs[perm])):
                torch.manual_seed(3)
                t0 = time.perf_counter()
                ranks, _ = run_sbc(thetas, obs, post, num_posterior_samples=L, reduce_fns=fns, show_progress_bar=False)
                ecp, alpha = run_tarp(thetas, obs, post, num_posterior_samples=L, show_progress_bar=False)
                torch.cuda.synchronize()
                entry[tag] = dict(min_ks_p=check_uniformity_frequentist(ranks, L).min().item(),
                                  atc=check_tarp(ecp, alpha)[0], wall_s=time.perf_counter() - t0)
            out[name] = entry
            print(name, json.dumps(entry), flush=True)
    res["calibration"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mcmc_batched_bench.json"))
    ap.add_argument("--only", choices=["ticks", "run_sbc", "calibration"], default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1x20,100x20,1000x20")
    ap.add_argument("--wg", default="64,128,256")
    ap.add_argument("--sbc-n", type=int, default=1000)
    ap.add_argument("--sbc-l", type=int, default=1000)
    a = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0)}
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    if a.only in (None, "ticks"):
        bench_ticks(res, sizes, a.reps, [int(w) for w in a.wg.split(",")])
    if a.only in (None, "run_sbc"):
        bench_run_sbc(res, a.sbc_n, a.sbc_l)
    if a.only in (None, "calibration"):
        bench_calibration(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
