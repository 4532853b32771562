"""LRUEmbedding measurements: the lru_embed HIP kernels next to the module's own eager route on the same GPU.

    python tools/bench_lru_embed.py --out profiles/lru_embed_bench.json

  * `features_*` -- forward + backward of `LRUEmbedding.features` (input layer, two bidirectional blocks of 20 + 20
        states, width 40, mean over time: sbi's defaults) on x (B, T, input_dim); the kernel route's time includes
        the `torch.cat` that rebuilds the flat weight image on every call.
  * `module_*` -- forward + backward of the whole module, `output_layer` included.
  * `sample_*` -- the forward alone under `no_grad` at B = 1: what every `posterior.sample(x=x_o)` pays.
  * `npe_epoch` -- one `NPE.train()` epoch on 2000 simulations of T = 100, batch 200: the mean of epochs 2.. of a
        6-epoch run; four runs per route, alternating, the first of each dropped as warm-up, the median of the rest.

The eager leg is the same module with `force_eager`: a Python loop over time in complex arithmetic.  The other leg is
the module's default route, recorded as `default_route` ("kernel", or the reason it ran eager).

Both legs are timed with a host clock around `calls` back-to-back calls that end in a device synchronise, the two legs
alternating, median over the repetitions, after a warm-up of both, as tools/bench_sir.py does.  The first shape is
measured again at the end.  The eager route's time grows with T (thousands of launches per call at T = 1000), so long
sequences are timed one call per window.
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

# (B, T, input_dim, forward only, tag)
SHAPES = ((200, 100, 1, False, ""), (200, 1000, 1, False, ""), (200, 1000, 3, False, ""), (1, 1000, 3, True, ""),
          (1024, 100, 3, False, ""), (4096, 100, 3, False, ""), (200, 100, 1, False, "_again"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--no-npe", action="store_true", help="skip the NPE.train() epoch")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import LRUEmbedding, NSFConfig

    if not torch.cuda.is_available():
        raise SystemExit("bench_lru_embed.py measures on a ROCm device; none is visible")
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
    for B, T, input_dim, fwd_only, tag in SHAPES:
        torch.manual_seed(0)
        net = LRUEmbedding(input_dim, 20).cuda()
        twin = copy.deepcopy(net)
        twin.force_eager = True
        x = torch.randn(B, T, input_dim, generator=g).cuda()
        routed = net.kernel_route(x)
        assert not twin.kernel_route(x)[0]
        name = f"B{B}_T{T}_i{input_dim}{tag}"
        calls, reps, warm = (1, 3 if a.quick else 5, 1) if T >= 1000 else (3, 5 if a.quick else 9, 2)
        if fwd_only:
            t_hip, t_eager = _alternating_median_ms([forward_only(net, x), forward_only(twin, x)], calls, reps, warm=warm)
            put(f"sample_{name}", B=B, T=T, input_dim=input_dim, default_route=routed[1], hip_ms=t_hip,
                eager_ms=t_eager, speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps)
            continue
        for what, width, pick in (("features", 40, lambda m: m.features), ("module", 20, lambda m: m)):
            wts = torch.randn(B, width, generator=g).cuda()
            t_hip, t_eager = _alternating_median_ms([step(pick(net), net, x, wts), step(pick(twin), twin, x, wts)],
                                                    calls, reps, warm=warm)
            put(f"{what}_{name}", B=B, T=T, input_dim=input_dim, default_route=routed[1], hip_ms=t_hip,
                eager_ms=t_eager, speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps)

    if not a.no_npe:
        from torch.distributions import MultivariateNormal

        from sbi_amd.inference import NPE

        theta = torch.randn(2000, 2, generator=g)
        grid = torch.linspace(0, 6.28, 100)
        x = (theta[:, :1] * torch.sin(grid) + theta[:, 1:] * torch.cos(grid)
             + 0.5 * torch.randn(2000, 100, generator=g))[..., None]
        runs = {"hip": [], "eager": []}
        for rep in range(4):            # run 0 of each leg is warm-up and is dropped; the legs alternate
            for name, force in (("hip", False), ("eager", True)):
                torch.manual_seed(0)
                emb = LRUEmbedding(1, 20)
                emb.force_eager = force
                prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
                inf = NPE(prior=prior, density_estimator=NSFConfig(embedding_net=emb), device="cuda",
                          show_progress_bars=False)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    inf.append_simulations(theta, x).train(training_batch_size=200, max_num_epochs=6)
                d = inf.summary["epoch_durations_sec"][1:]
                if rep > 0:
                    runs[name].append(1e3 * sum(d) / len(d))
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        put("npe_epoch", hip_ms=med["hip"], eager_ms=med["eager"], speedup=med["eager"] / med["hip"], all_runs_ms=runs,
            simulations=2000, T=100, batch=200)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
