"""CNNEmbedding measurements: the cnn_embed HIP kernels next to the module's own eager route on the same GPU.

    python tools/bench_cnn_embed.py --out profiles/cnn_embed_bench.json

  * `stack_*`  -- forward + backward of the convolution stack alone (`CNNEmbedding.features`: conv -> ReLU -> max-pool
        x 2 at sbi's defaults, 6 / 12 channels, 5-wide kernels, pool 2) on x (B, in_channels, shape); the kernel
        route's time includes the `torch.cat` that rebuilds the flat weight image on every call.
  * `module_*` -- forward + backward of the whole module, `FCEmbedding` head included (the head takes its own route:
        the embed kernels for F <= 64, eager beyond).
  * `npe_epoch` -- one `NPE.train()` epoch on 2000 simulations of shape (28, 28), batch 200: the mean of epochs 2.. of
        a 6-epoch run; four runs per route, alternating, the first of each dropped as warm-up, the median of the rest.

The eager leg is the same module with `force_eager`: eager torch all the way down, no cnn or embed kernel.  The other
leg is the module's default route, recorded as `default_route` ("kernel", or the reason it ran eager: batches above
1024 are routed to eager because the kernels measured slower there).

Both legs are timed with a host clock around `calls` back-to-back calls that end in a device synchronise, the two legs
alternating, median over the repetitions, after a warm-up of both (the eager convolution's first calls include the
library's kernel selection), as tools/bench_sir.py does.  The first shape is measured again at the end.
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

# (4096, (28, 28)) is above the kernels' batch limit: `module.kernel_route` answers False and the "hip" leg is the
# module's default route, whatever it is.  1024 is the limit itself.
SHAPES = ((200, (100,), 1, ""), (200, (1000,), 1, ""), (200, (28, 28), 1, ""), (1024, (28, 28), 1, ""),
          (4096, (28, 28), 1, ""), (200, (32, 32), 3, ""), (200, (100,), 1, "_again"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--no-npe", action="store_true", help="skip the NPE.train() epoch")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import CNNEmbedding, NSFConfig

    if not torch.cuda.is_available():
        raise SystemExit("bench_cnn_embed.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    def step(fn, net, x, wts):
        def run():
            net.zero_grad(set_to_none=True)
            (fn(x) * wts).sum().backward()
        return run

    g = torch.Generator().manual_seed(0)
    reps = 5 if a.quick else 15
    for B, shape, cin, tag in SHAPES:
        net = CNNEmbedding(shape, in_channels=cin).cuda()
        twin = copy.deepcopy(net)
        twin.force_eager = True
        x = torch.randn(B, cin, *shape, generator=g).cuda()
        routed = net.kernel_route(x)
        assert not twin.kernel_route(x)[0]
        F = net.linear_subnet.dims[0]
        name = f"B{B}_{'x'.join(map(str, shape))}_c{cin}{tag}"
        calls = 20 if B < 1000 else 5
        for what, width, pick in (("stack", F, lambda m: m.features), ("module", 20, lambda m: m)):
            wts = torch.randn(B, width, generator=g).cuda()
            t_hip, t_eager = _alternating_median_ms([step(pick(net), net, x, wts), step(pick(twin), twin, x, wts)],
                                                    calls, reps, warm=10)
            put(f"{what}_{name}", B=B, shape=list(shape), in_channels=cin, features=F, default_route=routed[1],
                hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps)

    if not a.no_npe:
        from torch.distributions import MultivariateNormal

        from sbi_amd.inference import NPE

        theta = torch.randn(2000, 2, generator=g)
        x = theta[:, :1, None] + theta[:, 1:, None] * torch.linspace(-1, 1, 28)[None, None, :] \
            + 0.5 * torch.randn(2000, 28, 28, generator=g)
        runs = {"hip": [], "eager": []}
        for rep in range(4):            # run 0 of each leg is warm-up and is dropped; the legs alternate
            for name, force in (("hip", False), ("eager", True)):
                torch.manual_seed(0)
                emb = CNNEmbedding((28, 28))
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
            simulations=2000, shape=[28, 28], batch=200)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
