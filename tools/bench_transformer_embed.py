"""TransformerEmbedding measurements: the tr_embed HIP kernels next to the module's own eager route on the same GPU.

    python tools/bench_transformer_embed.py --out profiles/transformer_embed_bench.json

  * `module_*` -- forward + backward of the whole module in training mode (attention_dropout 0.5 unless the tag says
        otherwise) on a scalar series x (B, T) at feature_space_dim=96 and otherwise the defaults; `_forward` shapes are
        a forward under `torch.no_grad()` in eval mode.  The kernel route's time includes the `torch.cat` that rebuilds
        the flat weight image and the allocation of the workspace on every call.
    A shape that the measured rule (`MAX_TRAINING_WORK`) routes to eager is measured a second time with the rule
        lifted (`kernels_forced_ms`), so that the losing figures stay in the file.
  * `npe_epoch` -- one `NPE.train()` epoch on 2000 simulations of T = 100, batch 200, with final_emb_dimension=24
        (the NSF's training kernels refuse the 48 context features of the default): the mean of epochs 2.. of a
        6-epoch run; four runs per route, alternating, the first of each dropped as warm-up, the median of the rest.

The eager leg is the same module with `force_eager`: the (B, H, T, T) scores, mask and dropout tensors of the installed
torch.  The other leg is the module's default route, recorded as `default_route` ("kernel", or the reason it ran eager).

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

# (B, T, forward only, module kwargs, tag)
SMALL = dict(feature_space_dim=48, num_hidden_layers=2, intermediate_size=64)
SHAPES = ((200, 100, False, {}, ""), (200, 1000, False, {}, ""), (1024, 100, False, {}, ""),
          (4096, 100, False, {}, ""), (1, 1000, True, {}, "_forward"),
          (200, 100, False, dict(attention_dropout=0.0), "_p0"),
          # the crossover of the training route: smaller batches at the same sizes, and a small module
          (4, 100, False, {}, ""), (16, 100, False, {}, ""), (32, 100, False, {}, ""), (64, 100, False, {}, ""),
          (128, 100, False, {}, ""), (200, 32, False, SMALL, "_F48_L2"),
          (200, 100, False, {}, "_again"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--no-npe", action="store_true", help="skip the NPE.train() epoch")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import NSFConfig, TransformerEmbedding
    from sbi_amd.neural_nets.embedding_nets import transformer as TR

    if not torch.cuda.is_available():
        raise SystemExit("bench_transformer_embed.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    def step(net, x, wts, forward_only):
        def train():
            net.zero_grad(set_to_none=True)
            (net(x) * wts).sum().backward()

        def infer():
            with torch.no_grad():
                net(x)
        return infer if forward_only else train

    g = torch.Generator().manual_seed(0)
    for B, T, forward_only, kw, tag in SHAPES:
        torch.manual_seed(0)
        net = TransformerEmbedding(**dict(dict(feature_space_dim=96), **kw)).cuda().train(not forward_only)
        twin = copy.deepcopy(net)
        twin.force_eager = True
        x = torch.randn(B, T, generator=g).cuda()
        with torch.set_grad_enabled(not forward_only):
            routed = net.kernel_route(x)
        assert not twin.kernel_route(x)[0]
        wts = torch.randn(B, net.aggregator.out_features, generator=g).cuda()
        calls, reps, warm = (2, 3 if a.quick else 5, 1) if B * T >= 100_000 else (5, 5 if a.quick else 9, 2)
        t_hip, t_eager = _alternating_median_ms([step(net, x, wts, forward_only), step(twin, x, wts, forward_only)],
                                                calls, reps, warm=warm)
        extra = {}
        if "measured faster" in routed[1]:
            # the shape the measured rule routes to eager: the kernels' own (losing) figure, with the rule lifted
            rule, TR.MAX_TRAINING_WORK = TR.MAX_TRAINING_WORK, float("inf")
            assert net.kernel_route(x)[0], net.kernel_route(x)
            t_forced, t_eager2 = _alternating_median_ms([step(net, x, wts, forward_only),
                                                         step(twin, x, wts, forward_only)], calls, reps, warm=warm)
            TR.MAX_TRAINING_WORK = rule
            extra = dict(kernels_forced_ms=t_forced, eager_next_to_forced_ms=t_eager2,
                         kernels_forced_speedup=t_eager2 / t_forced)
        put(f"module_B{B}_T{T}{tag}", B=B, T=T, forward_only=forward_only, default_route=routed[1], hip_ms=t_hip,
            eager_ms=t_eager, speedup=t_eager / t_hip, calls_per_window=calls, repetitions=reps,
            attention_dropout=net.config["attention_dropout"], **extra)
        del net, twin, x
        torch.cuda.empty_cache()

    if not a.no_npe:
        from torch.distributions import MultivariateNormal

        from sbi_amd.inference import NPE

        theta = torch.randn(2000, 2, generator=g)
        grid = torch.arange(100) / 100 * 6.2831853
        x = theta[:, :1] * torch.sin(grid) + theta[:, 1:] * torch.cos(grid) + 0.5 * torch.randn(2000, 100, generator=g)
        runs = {"hip": [], "eager": []}
        for rep in range(4):            # run 0 of each leg is warm-up and is dropped; the legs alternate
            for name, force in (("hip", False), ("eager", True)):
                torch.manual_seed(0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    emb = TransformerEmbedding(feature_space_dim=96, final_emb_dimension=24)
                    emb.force_eager = force
                    prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
                    inf = NPE(prior=prior, density_estimator=NSFConfig(embedding_net=emb), device="cuda",
                              show_progress_bars=False)
                    inf.append_simulations(theta, x).train(training_batch_size=200, max_num_epochs=6)
                d = inf.summary["epoch_durations_sec"][1:]
                if rep > 0:
                    runs[name].append(1e3 * sum(d) / len(d))
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        route = TransformerEmbedding(feature_space_dim=96, final_emb_dimension=24).cuda().kernel_route(
            torch.zeros(200, 100, device="cuda"))[1]
        put("npe_epoch", hip_ms=med["hip"], eager_ms=med["eager"], speedup=med["eager"] / med["hip"], all_runs_ms=runs,
            simulations=2000, shape=[100], batch=200, final_emb_dimension=24, default_route=route)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
