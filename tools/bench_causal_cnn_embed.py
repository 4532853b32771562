"""CausalCNNEmbedding measurements: the causal_cnn HIP kernels next to the module's own eager route on the same GPU.

    python tools/bench_causal_cnn_embed.py --out profiles/causal_cnn_embed_bench.json

  * `features_*` -- forward + backward of `CausalCNNEmbedding.features` (five causal layers of 16 channels, kernel 2,
        dilations 1 .. 16, average pool 160: sbi's defaults) on x (B, T); the kernel route's time includes the
        `torch.cat` that rebuilds the flat weight image on every call.
  * `module_*` -- forward + backward of the whole module, the default aggregator included.
  * `sample_*` -- the forward alone under `no_grad` at B = 1: what every `posterior.sample(x=x_o)` pays.
  * `npe_epoch` -- one `NPE.train()` epoch on 2000 simulations of T = 400, batch 200: the mean of epochs 2.. of a
        6-epoch run; four runs per route, alternating, the first of each dropped as warm-up, the median of the rest.

The eager leg is the same module with `force_eager`: `ZeroPad1d` + `Conv1d` + `LeakyReLU` per layer and `AvgPool1d`
of the installed torch.  The other leg is the module's default route, recorded as `default_route` ("kernel", or the
reason it ran eager).

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

# (B, T, forward only, tag)
SHAPES = ((200, 400, False, ""), (200, 4000, False, ""), (200, 20_000, False, ""), (1024, 4000, False, ""),
          (4096, 1000, False, ""), (1, 100_000, True, ""), (200, 400, False, "_again"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--no-npe", action="store_true", help="skip the NPE.train() epoch")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import CausalCNNEmbedding, NSFConfig

    if not torch.cuda.is_available():
        raise SystemExit("bench_causal_cnn_embed.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    def step(fn, net, x, wts):
        def run():
            net.zero_grad(set_to_none=True)
            (fn(x) * wts).sum().backward()
        return run

    def forward_only(fn, x):
        def run():
            with torch.no_grad():
                fn(x)
        return run

    g = torch.Generator().manual_seed(0)
    for B, T, fwd_only, tag in SHAPES:
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = CausalCNNEmbedding((T,)).cuda()
        twin = copy.deepcopy(net)
        twin.force_eager = True
        x = torch.randn(B, T, generator=g).cuda()
        routed = net.kernel_route(x[:, None])
        assert not twin.kernel_route(x[:, None])[0]
        name = f"B{B}_T{T}{tag}"
        calls, reps, warm = (1, 3 if a.quick else 7, 1) if B * T >= 2_000_000 else (5, 5 if a.quick else 9, 2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if fwd_only:
                t_hip, t_eager = _alternating_median_ms([forward_only(net, x), forward_only(twin, x)], calls, reps,
                                                        warm=warm)
                put(f"sample_{name}", B=B, T=T, default_route=routed[1], hip_ms=t_hip, eager_ms=t_eager,
                    speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps)
                continue
            for what, shape, pick in (("features", (B, 16, T // 160), lambda m: m.features),
                                      ("module", (B, 20), lambda m: m)):
                wts = torch.randn(*shape, generator=g).cuda()
                t_hip, t_eager = _alternating_median_ms([step(pick(net), net, x, wts), step(pick(twin), twin, x, wts)],
                                                        calls, reps, warm=warm)
                put(f"{what}_{name}", B=B, T=T, default_route=routed[1], hip_ms=t_hip, eager_ms=t_eager,
                    speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps)
        del net, twin, x
        torch.cuda.empty_cache()

    if not a.no_npe:
        from torch.distributions import MultivariateNormal

        from sbi_amd.inference import NPE

        theta = torch.randn(2000, 2, generator=g)
        grid = torch.linspace(0, 6.28, 400)
        x = theta[:, :1] * torch.sin(grid) + theta[:, 1:] * torch.cos(grid) + 0.5 * torch.randn(2000, 400, generator=g)
        runs = {"hip": [], "eager": []}
        for rep in range(4):            # run 0 of each leg is warm-up and is dropped; the legs alternate
            for name, force in (("hip", False), ("eager", True)):
                torch.manual_seed(0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    emb = CausalCNNEmbedding((400,))
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
            simulations=2000, T=400, batch=200)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
