"""SpectralConvEmbedding measurements: the sc_embed HIP kernels next to the module's own eager route on the same GPU.

    python tools/bench_sc_embed.py --out profiles/sc_embed_bench.json

  * `module_*` -- forward + backward of the whole module on x (B, in_channels, n_points), or (B, 2, in_channels,
        n_points) with a sorted random grid as positions; the kernel route's time includes the `torch.cat` that rebuilds
        the flat weight image on every call.
  * `npe_epoch` -- one `NPE.train()` epoch on 2000 simulations of (1, 64), batch 200: the mean of epochs 2.. of a
        6-epoch run; four runs per route, alternating, the first of each dropped as warm-up, the median of the rest.

The eager leg is the same module with `force_eager`: the dense (B, modes, n_points) operator, complex `matmul`s and
`einsum`s of the installed torch.  The other leg is the module's default route, recorded as `default_route` ("kernel",
or the reason it ran eager).

Both legs are timed with a host clock around `calls` back-to-back calls that end in a device synchronise, the two legs
alternating, median over the repetitions, after a warm-up of both, as tools/bench_sir.py does.  The first shape is
measured again at the end.
"""
import argparse
import copy
import json
import sys
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

DOC = dict(modes=15, num_layers=4)
# (B, in_channels, n_points, positions, module kwargs, tag)
SHAPES = ((200, 1, 100, False, {}, ""), (200, 3, 500, False, {}, ""), (200, 3, 500, True, {}, ""),
          (200, 3, 500, False, DOC, "_m15_l4"), (1024, 3, 500, False, {}, ""), (4096, 1, 500, False, {}, ""),
          (16, 1, 4000, False, {}, ""), (200, 1, 100, False, {}, "_again"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--no-npe", action="store_true", help="skip the NPE.train() epoch")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import NSFConfig, SpectralConvEmbedding

    if not torch.cuda.is_available():
        raise SystemExit("bench_sc_embed.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    def step(net, x, wts):
        def run():
            net.zero_grad(set_to_none=True)
            (net(x) * wts).sum().backward()
        return run

    g = torch.Generator().manual_seed(0)
    for B, cin, n, positions, kw, tag in SHAPES:
        torch.manual_seed(0)
        net = SpectralConvEmbedding(cin, **kw).cuda()
        twin = copy.deepcopy(net)
        twin.force_eager = True
        x = torch.randn(B, cin, n, generator=g)
        if positions:
            grid = torch.sort(torch.rand(n, generator=g))[0]
            x = torch.stack([x, grid.expand_as(x)], dim=1)
        x = x.cuda()
        routed = net.kernel_route(x)
        assert not twin.kernel_route(x)[0]
        wts = torch.randn(B, 2 * net.modes * net.out_channels, generator=g).cuda()
        calls, reps, warm = (2, 3 if a.quick else 7, 1) if B * n >= 500_000 else (5, 5 if a.quick else 9, 2)
        t_hip, t_eager = _alternating_median_ms([step(net, x, wts), step(twin, x, wts)], calls, reps, warm=warm)
        put(f"module_B{B}_C{cin}_N{n}{'_positions' if positions else ''}{tag}", B=B, in_channels=cin, n_points=n,
            positions=positions, default_route=routed[1], hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
            calls_per_window=calls, repetitions=reps, **kw)
        del net, twin, x
        torch.cuda.empty_cache()

    if not a.no_npe:
        from torch.distributions import MultivariateNormal

        from sbi_amd.inference import NPE

        theta = torch.randn(2000, 2, generator=g)
        grid = torch.arange(64) / 64 * 6.2831853
        x = theta[:, :1] * torch.sin(grid) + theta[:, 1:] * torch.cos(grid) + 0.5 * torch.randn(2000, 64, generator=g)
        x = x[:, None]
        runs = {"hip": [], "eager": []}
        for rep in range(4):            # run 0 of each leg is warm-up and is dropped; the legs alternate
            for name, force in (("hip", False), ("eager", True)):
                torch.manual_seed(0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    emb = SpectralConvEmbedding(1)
                    emb.force_eager = force
                    prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
                    inf = NPE(prior=prior, density_estimator=NSFConfig(embedding_net=emb), device="cuda",
                              show_progress_bars=False)
                    inf.append_simulations(theta, x).train(training_batch_size=200, max_num_epochs=6)
                d = inf.summary["epoch_durations_sec"][1:]
                if rep > 0:
                    runs[name].append(1e3 * sum(d) / len(d))
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        put("npe_epoch", hip_ms=med["hip"], eager_ms=med["eager"], speedup=med["eager"] / med["hip"], all_runs_ms=runs,
            simulations=2000, shape=[1, 64], batch=200)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
