"""NRE measurements: the fused NRE_B training step against eager torch, the log-ratio kernel, the iid-trials kernel and
the MCMC tick on the ratio potential.

    python tools/bench_nre.py --out profiles/nre_bench.json

Shapes: theta-dim = x-dim = 10, sbi's default classifier (hidden 50, 2 blocks), 10 atoms.
  * `step`   -- one FusedNREStep.step (atoms, forward + stash, loss weights, backward + fixed-order weight-gradient
                reduction, clip + Adam, re-pack) at batch 200 and 65 536;
  * `eager`  -- the same step as eager torch on the same device: the oracle's ResidualNet in fp32 on the
                atoms-major pairs, the NRE_B loss, autograd, clip_grad_norm_ and torch.optim.Adam;
  * `log_ratio` -- sbi_amd_nre_log_ratio for one x_o at 10^6 theta (evals / s);
  * `trials` -- sbi_amd_nre_log_ratio_trials at 20 theta x 100 trials and 10 000 x 100;
  * `mcmc_tick` -- MCMCPosterior.sample wall time for 2 000 draws at 20 chains x 100 trials, fused tick against the
                generic potential.
Device times are medians over CUDA events after a warm-up of the same leg (the device ramps its clock after idling).
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _median_ms(fn, reps=30, warm=10):
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
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


def bench_step(res):
    import torch

    from oracle.nsf_oracle import ResidualNet
    from sbi_amd.inference.trainers.nre.nre import MODE_B, FusedNREStep, draw_atoms, row_losses_torch
    from sbi_amd.neural_nets import classifier_nn

    D = C = 10
    A = 10
    for B in (200, 65536):
        torch.manual_seed(0)
        theta = torch.randn(B, D)
        x = theta + 0.5 * torch.randn(B, C)
        est = classifier_nn("resnet")(theta, x).to("cuda")
        th, xx = theta.cuda(), x.cuda()
        step = FusedNREStep(est, MODE_B, A)
        t_hip = _median_ms(lambda: step.step(th, xx), reps=50 if B == 200 else 20)
        # eager torch on the same device
        net = ResidualNet(D + C, 1, 50, None, 2).cuda()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4)
        zs = est.net.zstats

        def eager():
            atoms = draw_atoms(th, A, 1)
            zt = (atoms.reshape(-1, D) - zs[:D]) / zs[D : 2 * D]
            zx = ((xx - zs[2 * D : 2 * D + C]) / zs[2 * D + C :]).repeat(A, 1)
            opt.zero_grad()
            logits = net(torch.cat([zt, zx], 1)).squeeze(-1)
            row_losses_torch(MODE_B, logits, B, A).mean().backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
            opt.step()

        t_eager = _median_ms(eager, reps=50 if B == 200 else 20)
        flop = 3 * 2.0 * (A * B) * (D * 50 + 2 * 2 * 50 * 50 + 50) + 2.0 * B * C * 50
        res[f"step_B{B}"] = dict(batch=B, atoms=A, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
                                 tflops_hip=flop / (t_hip * 1e-3) / 1e12, fp32_peak_fraction=flop / (t_hip * 1e-3)
                                 / 157.3e12)
        print(json.dumps(res[f"step_B{B}"]), flush=True)


def bench_log_ratio(res):
    import torch

    from sbi_amd.neural_nets import classifier_nn

    torch.manual_seed(0)
    est = classifier_nn("resnet")(torch.randn(500, 10), torch.randn(500, 10)).to("cuda")
    th = torch.randn(10**6, 10, device="cuda")
    x_o = torch.randn(1, 10, device="cuda")
    t = _median_ms(lambda: est.log_ratio_one_x(th, x_o))
    flop = 2.0 * 1e6 * (10 * 50 + 4 * 50 * 50 + 50)
    res["log_ratio_1e6"] = dict(ms=t, evals_per_s=1e6 / (t * 1e-3), fp32_peak_fraction=flop / (t * 1e-3) / 157.3e12)
    print(json.dumps(res["log_ratio_1e6"]), flush=True)
    for N, T in ((20, 100), (10_000, 100)):
        xt = torch.randn(T, 10, device="cuda")
        thn = th[:N]
        t_tr = _median_ms(lambda: est.log_ratio_iid_trials(xt, thn))
        pairs_th = thn.repeat_interleave(T, 0)
        with torch.no_grad():
            t_pairs = _median_ms(lambda: est._log_ratio_rows(pairs_th, xt, T).reshape(N, T).sum(1))
        res[f"trials_{N}x{T}"] = dict(trials_ms=t_tr, materialised_pairs_ms=t_pairs)
        print(json.dumps(res[f"trials_{N}x{T}"]), flush=True)


def bench_mcmc(res):
    import torch
    from torch.distributions import MultivariateNormal

    from sbi_amd.inference import NRE_B
    from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
    from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential
    from sbi_amd.simulators.linear_gaussian import linear_gaussian

    torch.manual_seed(0)
    dim = 10
    prior = MultivariateNormal(torch.zeros(dim, device="cuda"), torch.eye(dim, device="cuda"))
    theta = prior.sample((2000,)).cpu()
    x = linear_gaussian(theta, -torch.ones(dim), 0.8 * torch.eye(dim))
    inf = NRE_B(prior=prior, device="cuda", show_progress_bars=False)
    est = inf.append_simulations(theta, x).train(max_num_epochs=5)
    x_o = torch.zeros(100, dim, device="cuda")
    pot, tf = ratio_estimator_based_potential(est, prior, x_o)
    out = {}
    for name in ("fused", "generic"):
        post = MCMCPosterior(pot, prior, tf, num_chains=20, thin=1, warmup_steps=10, init_strategy="proposal",
                             device="cuda")
        if name == "generic":
            post._fused_potential = lambda: None       # the potential through the generic tick
        post.sample((200,), x=x_o, show_progress_bars=False)            # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        post.sample((2000,), x=x_o, show_progress_bars=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[name] = dict(wall_s=dt, fused=getattr(post.potential_, "fused_spec", None) is not None)
    res["mcmc_20_chains_100_trials"] = out
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-mcmc", action="store_true")
    a = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0)}
    bench_step(res)
    bench_log_ratio(res)
    if not a.skip_mcmc:
        bench_mcmc(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
