"""Embedding-net measurements: the embed HIP kernels next to the modules' own eager route on the same GPU.

    python tools/bench_embed.py --out profiles/embed_bench.json

  * `perminv_B*_T*_D*` -- forward + backward of `PermutationInvariantEmbedding(FCEmbedding(D, 20, 2, 50), 20)` (sbi's
        defaults: head 100 hidden units, 20 outputs) on x (B, T, D) with a trial count uniform in 1..T, NaN-padded;
        the kernel route's time includes the `torch.cat` that rebuilds the flat weight image on every call.
  * `fc_B*` -- forward + backward (with d/dx) of `FCEmbedding(10)` on B rows.
  * `npe_epoch` -- one `NPE.train()` epoch of the iid-trials task of tests/test_npe_iid_embedding_e2e_gpu.py (2000
        simulations, T = 8, batch 200): the mean of epochs 2.. of a 6-epoch run; four runs per route, alternating, the
        first of each dropped as warm-up, the median of the other three.

The eager leg is the same module with `force_eager`: eager torch all the way down, no embed kernel.

Both legs are timed with a host clock around `calls` back-to-back calls that end in a device synchronise, the two legs
alternating, median over the repetitions, after a warm-up of both (as tools/bench_sir.py).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import FCEmbedding, NSFConfig, PermutationInvariantEmbedding

    if not torch.cuda.is_available():
        raise SystemExit("bench_embed.py measures on a ROCm device; none is visible")
    res = {"device": torch.cuda.get_device_name(0)}

    def put(name, **kw):
        res[name] = kw
        print(name, json.dumps(kw), flush=True)

    def legs(net):
        net = net.cuda()
        twin = copy.deepcopy(net)
        twin.force_eager = True
        return net, twin

    def step(net, x, wts):
        def run():
            net.zero_grad(set_to_none=True)
            if x.requires_grad:
                x.grad = None
            (net(x) * wts).sum().backward()
        return run

    g = torch.Generator().manual_seed(0)
    reps = 5 if a.quick else 15
    # the first shape is measured again at the end under another name: a first window that differs from the repeat
    # is warm-up (clock ramp, first-call costs), not the shape
    for B, T, D, tag in ((200, 10, 2, ""), (200, 100, 2, ""), (4096, 10, 5, ""), (4096, 100, 5, ""),
                         (200, 10, 2, "_again")):
        x = torch.randn(B, T, D, generator=g)
        counts = torch.randint(1, T + 1, (B,), generator=g)
        x[torch.arange(T)[None, :] >= counts[:, None]] = float("nan")
        x, wts = x.cuda(), torch.randn(B, 20, generator=g).cuda()
        net, twin = legs(PermutationInvariantEmbedding(FCEmbedding(D, 20, 2, 50), 20))
        assert net.kernel_route(x)[0] and not twin.kernel_route(x)[0]
        calls = 20 if B * T < 100_000 else 5
        t_hip, t_eager = _alternating_median_ms([step(net, x, wts), step(twin, x, wts)], calls, reps, warm=10)
        put(f"perminv_B{B}_T{T}_D{D}{tag}", B=B, T=T, D=D, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
            calls_per_window=calls, repetitions=reps)
    for B in (200, 65536):
        x = torch.randn(B, 10, generator=g).cuda().requires_grad_(True)
        wts = torch.randn(B, 20, generator=g).cuda()
        net, twin = legs(FCEmbedding(10))
        assert net.kernel_route(x)[0] and not twin.kernel_route(x)[0]
        calls = 20 if B < 10_000 else 5
        t_hip, t_eager = _alternating_median_ms([step(net, x, wts), step(twin, x, wts)], calls, reps, warm=10)
        put(f"fc_B{B}", B=B, in_dim=10, hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip, calls_per_window=calls,
            repetitions=reps)

    # one NPE.train() epoch of the e2e task
    from torch.distributions import MultivariateNormal

    from sbi_amd.inference import NPE

    theta = torch.randn(2000, 2, generator=g)
    x = theta[:, None, :] + 0.5 * torch.randn(2000, 8, 2, generator=g)
    counts = torch.randint(1, 9, (2000,), generator=g)
    x[torch.arange(8)[None, :] >= counts[:, None]] = float("nan")
    runs = {"hip": [], "eager": []}
    for rep in range(4):            # run 0 of each leg is warm-up and is dropped; the legs alternate
        for name, force in (("hip", False), ("eager", True)):
            torch.manual_seed(0)
            emb = PermutationInvariantEmbedding(FCEmbedding(2, 20, 2, 40), 20, num_hiddens=40, output_dim=10)
            emb.force_eager = force
            prior = MultivariateNormal(torch.zeros(2, device="cuda"), torch.eye(2, device="cuda"))
            inf = NPE(prior=prior, density_estimator=NSFConfig(embedding_net=emb), device="cuda",
                      show_progress_bars=False)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                inf.append_simulations(theta, x, exclude_invalid_x=False).train(training_batch_size=200,
                                                                                 max_num_epochs=6)
            d = inf.summary["epoch_durations_sec"][1:]
            if rep > 0:
                runs[name].append(1e3 * sum(d) / len(d))
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    put("npe_epoch", hip_ms=med["hip"], eager_ms=med["eager"], speedup=med["eager"] / med["hip"], all_runs_ms=runs,
        simulations=2000, T=8, batch=200)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
