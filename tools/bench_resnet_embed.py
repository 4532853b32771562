"""ResNetEmbedding1D measurements: the resnet_embed HIP kernels next to the module's own eager route on the same GPU.

    python tools/bench_resnet_embed.py --out profiles/resnet_embed_bench.json

  * `default_B*` -- the default net (c_in 10, c_out 8, 20 blocks, c_internal 128, c_hidden 128, head 1000) at batch 1,
        16, 64, 200, 1024, 8192 and 65 536: forward + backward of the whole module (head included, which is torch in
        both legs), and (`_forward`) a forward under `torch.no_grad()`.
  * `narrow_B200*` -- c_internal 32, c_hidden 32, 3 blocks, head 32.
    The kernel route's time includes everything it pays per call: the `torch.cat` that rebuilds the flat parameters,
        the pack launch that writes the staged weight image, the allocation of the workspace.
    A shape that the measured rule (`MAX_ROWS_TRAINING` / `MAX_ROWS_FORWARD`) routes to eager is measured a second
        time with the rule lifted (`kernels_forced_ms`), so that the losing figures stay in the file.

The eager leg is the same module with `force_eager`.  The other leg is the module's default route, recorded as
`default_route` ("kernel", or the reason it ran eager).  Both legs are timed with a host clock around `calls`
back-to-back calls that end in a device synchronise, the two legs alternating, median over the repetitions, after a
warm-up of both, as tools/bench_sir.py does.  The first shape is measured again at the end.  One process, no child
processes: run it under a time limit of its own (`timeout -k 10 600 python tools/bench_resnet_embed.py ...`).
"""
import argparse
import copy
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

DEFAULT = dict(c_in=10, c_out=8)
NARROW = dict(c_in=10, c_out=8, n_blocks=3, c_internal=32, c_hidden_final=32, construct_mapping_kwargs={"c_hidden": 32})
# (name, rows, module kwargs)
SHAPES = [(f"default_B{b}", b, DEFAULT) for b in (1, 16, 64, 200, 1024, 8192, 65536)] + \
    [("narrow_B200", 200, NARROW), ("default_B1_again", 1, DEFAULT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    a = ap.parse_args()
    import torch

    from bench_sir import _alternating_median_ms
    from sbi_amd.neural_nets import ResNetEmbedding1D
    from sbi_amd.neural_nets.embedding_nets import resnet as RN

    if not torch.cuda.is_available():
        raise SystemExit("bench_resnet_embed.py measures on a ROCm device; none is visible")
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
    for name, rows, kw in SHAPES:
        for forward_only in (False, True):
            torch.manual_seed(0)
            net = ResNetEmbedding1D(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in kw.items()}).cuda()
            twin = copy.deepcopy(net)
            twin.force_eager = True
            x = torch.randn(rows, kw["c_in"], generator=g).cuda()
            wts = torch.randn(rows, kw["c_out"], generator=g).cuda()
            with torch.set_grad_enabled(not forward_only):
                routed = net.kernel_route(x)
            assert not twin.kernel_route(x)[0]
            calls, reps, warm = (2, 3 if a.quick else 5, 1) if rows >= 8192 else (10, 5 if a.quick else 9, 2)
            legs = [step(net, x, wts, forward_only), step(twin, x, wts, forward_only)]
            t_hip, t_eager = _alternating_median_ms(legs, calls, reps, warm=warm)
            extra = {}
            if "measured faster" in routed[1]:
                rule = RN.MAX_ROWS_TRAINING, RN.MAX_ROWS_FORWARD
                RN.MAX_ROWS_TRAINING = RN.MAX_ROWS_FORWARD = float("inf")
                with torch.set_grad_enabled(not forward_only):
                    assert net.kernel_route(x)[0], net.kernel_route(x)
                t_forced, t_eager2 = _alternating_median_ms(legs, calls, reps, warm=warm)
                RN.MAX_ROWS_TRAINING, RN.MAX_ROWS_FORWARD = rule
                extra = dict(kernels_forced_ms=t_forced, eager_next_to_forced_ms=t_eager2,
                             kernels_forced_speedup=t_eager2 / t_forced)
            put(name + ("_forward" if forward_only else ""), rows=rows, forward_only=forward_only,
                default_route=routed[1], hip_ms=t_hip, eager_ms=t_eager, speedup=t_eager / t_hip,
                calls_per_window=calls, repetitions=reps, **extra)
            del net, twin, x, legs
            torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
