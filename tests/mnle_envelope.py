"""Configurations and helpers of the MNLE parity tests (tests/test_mnle_gpu.py, test_mnle_envelope_gpu.py,
test_mnle_envelope_cpu.py): the shapes at which csrc/mnle_kernel.h and the host side in csrc/mnle.hip take another
path, the two row pools, and the reference-only criteria by which rows are left out of a comparison.  Importable
without a GPU; no test functions here.

Bounds are the project's (docstring of tests/test_mnle_gpu.py): "no further from fp64 than the fp32 restatement is
(x2) + 1e-5" for log_prob, its parts, the finite logits and the sampled continuous column; for the training pass
1e-5 + 1e-5 max|ref| on the losses, 2e-4 of the gradient's max norm, 3e-4 per parameter block and for d loss / d theta.
"""
import copy
import functools
import warnings

import torch

from tests.mnle_oracle import MixedOracle

# name: (categories, C, discrete width, discrete blocks, embedding, hidden, K, T, context layers)
BASE_CONFIGS = {
    "defaults": ([2], 4, 50, 2, 50, 50, 10, 5, 1),
    "multi": ([2, 5, 3], 3, 32, 1, 32, 32, 8, 2, 0),
    "corner": ([16, 2, 7, 16], 64, 64, 4, 64, 64, 16, 8, 2),
    "tiny": ([3], 1, 8, 1, 8, 8, 4, 1, 1),
}
NEW_CONFIGS = {
    # three distinct widths, K = 5 (mnle_k5.hip, PT = 1 with 14 parameters), a 1-category variable whose Kmax comes
    # from another one, L = 3 (virtual gradient blocks with l - 1 > 0), embedding input width 40 (three 16-tiles)
    "uneven": ([3, 1, 4], 5, 24, 1, 40, 56, 5, 3, 3),
    # T = 16, L = 4: 111 weight-gradient linears in three batches; every width one past a 16-tile; C = 17
    "deep": ([2, 16], 17, 33, 3, 17, 49, 16, 16, 4),
    # no residual block, no context layer, one transform, near-minimal widths, C = 1
    "floor2": ([1, 2], 1, 2, 0, 3, 2, 4, 1, 0),
    # every minimum of the envelope.  Forward paths only: with width-1 ReLU nets d loss / d theta of the restatement is
    # identically zero on all 1000 rows of the pool, so there is no reference gradient to compare with.
    "floor": ([1], 1, 1, 0, 1, 1, 4, 1, 0),
}
CONFIGS = {**BASE_CONFIGS, **NEW_CONFIGS}
TRAINABLE_NEW = ["uneven", "deep", "floor2"]
POOL_ROWS = 1000
LARGE_ROWS = 16321          # first row count at which mnle_waves() picks 4 waves (2 waves from 8161)
LARGE_CONFIGS = ["tiny", "uneven"]
SAMPLE_SEED = 11


def category_values(cats):
    """Raw values that are not the indices: {-1, 1}, {0, 2, 5, ...}, ..."""
    out = []
    for v, c in enumerate(cats):
        if c == 2:
            out.append(torch.tensor([-1.0, 1.0]))
        else:
            out.append(torch.cumsum(torch.arange(c, dtype=torch.float32) % 3 + 2, 0) - 2 + v)
    return out


def toy_data(cats, C, n, log_x, seed=0):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(n, C, generator=g) * 1.3 + 0.2
    vals = category_values(cats)
    idx = torch.stack([torch.randint(0, c, (n,), generator=g) for c in cats], 1)
    idx[: max(cats)] = torch.stack([torch.arange(max(cats)) % c for c in cats], 1)      # every category is present
    d = torch.stack([vals[v][idx[:, v]] for v in range(len(cats))], 1)
    base = 0.5 * theta[:, 0] + 0.2 * idx[:, 0].float() + 0.4 * torch.randn(n, generator=g)
    xc = torch.exp(0.5 * base) if log_x else base
    return theta, torch.cat([xc[:, None], d], 1)


def hyper_of(name, log_x=False):
    from sbi_amd.neural_nets.estimators.mixed_density_estimator import MNLEHyper

    cats, C, Hd, NB, E, Hc, K, T, L = CONFIGS[name]
    return MNLEHyper(num_categories=tuple(cats), C=C, discrete_hidden=Hd, discrete_blocks=NB, embedding=E, hidden=Hc,
                     num_bins=K, num_transforms=T, context_layers=L, log_transform=log_x)


@functools.lru_cache(maxsize=None)
def mnle_pair_cpu(name, log_x=False, perturb=0.05, seed=1):
    """(fp32 restatement, fp64 restatement, HIP estimator on the CPU, theta, x): identical perturbed weights and
    z-scoring; theta and x are the 1000-row pool the estimator was built from."""
    from sbi_amd.neural_nets.net_builders.mixed_nets import build_mnle

    cats, C, Hd, NB, E, Hc, K, T, L = CONFIGS[name]
    theta, x = toy_data(cats, C, POOL_ROWS, log_x)
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = build_mnle(x, theta, log_transform_x=log_x, hidden_features=Hc, discrete_hidden_features=Hd,
                         discrete_hidden_layers=NB, combined_embedding_features=E, num_bins=K, num_transforms=T,
                         hidden_layers_spline_context=L, num_categories_per_variable=torch.tensor(cats))
    oracle = MixedOracle(cats, category_values(cats), C, Hd, NB, E, Hc, K, T, L, 10.0, log_x)
    oracle.set_zstats(est.net.zstats)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in oracle.parameters():
            p.add_(perturb * torch.randn(p.shape, generator=g))
    est.load_state_dict(oracle.state_dict())
    assert torch.equal(est.net.flat_params.detach().cpu(), oracle.flat_params())
    return oracle, copy.deepcopy(oracle).double(), est, theta, x


@functools.lru_cache(maxsize=None)
def pool(name, log_x, large=False):
    """(theta, x) of the 1000-row pool the estimator was built from, or of the 16321-row pool for the wave counts and
    the multi-chunk training passes (the category values are a function of the categories alone: same lookup)."""
    cats, C = CONFIGS[name][:2]
    return toy_data(cats, C, LARGE_ROWS, log_x, seed=2) if large else toy_data(cats, C, POOL_ROWS, log_x)


@functools.lru_cache(maxsize=None)
def row_gradients(name, large=False):
    """d loss / d theta per row of a pool (log x) in the fp32 and in the fp64 restatement, both as fp64."""
    o32, o64 = mnle_pair_cpu(name, True)[:2]
    theta, x = pool(name, True, large)

    def row_grads(o, dt):
        th = theta.to(dt).clone().requires_grad_(True)
        o.loss(x.to(dt), th).sum().backward()
        o.zero_grad()
        return th.grad.double()

    return row_grads(o32, torch.float32), row_grads(o64, torch.float64)


@functools.lru_cache(maxsize=None)
def smooth_rows(name, large=False):
    """Rows of a pool on which the fp32 and the fp64 restatement take the same branch of every ReLU: (kept row
    numbers, number left out).

    The networks are piecewise linear in their activations: a pre-activation within fp32 rounding of zero is positive
    in one precision and negative in the other, and the fp64 gradient is then the derivative of a DIFFERENT piece than
    the one any fp32 evaluation is on (the corner configuration has 2 240 ReLU inputs per row: at 1e-6 absolute
    rounding error that is about one such row in 500).  Such a row shows in the references alone, as a jump in its
    d loss / d theta between the two restatements (fp32 rounding moves that gradient by ~1e-5 of its size, a flipped
    unit by far more); these rows are left out, their number is capped by the caller, and the kernels' output plays
    no part in the choice."""
    g32, g64 = row_gradients(name, large)
    rel = (g32 - g64).abs().max(1).values / g64.abs().max(1).values
    keep = rel <= 1e-3
    return torch.nonzero(keep)[:, 0], int((~keep).sum())


def sample_draws(n, V):
    """The sampling tests' draws: uniforms (n, V) and normal noise (n,)."""
    g = torch.Generator().manual_seed(SAMPLE_SEED)
    return torch.rand(n, V, generator=g), torch.randn(n, generator=g)


@functools.lru_cache(maxsize=None)
def sample_reference(name, log_x, large=False):
    """Both restatements' draws for `sample_draws` on a whole pool:
    (u, noise, idx64, x64, idx32, x32, keep), keep = u further than 1e-6 from every cumulative boundary in fp64."""
    o32, o64 = mnle_pair_cpu(name, log_x)[:2]
    theta, _ = pool(name, log_x, large)
    u, noise = sample_draws(theta.shape[0], len(CONFIGS[name][0]))
    with torch.no_grad():
        idx64, x64, gap = o64.sample_given(u.double(), noise.double(), theta.double())
        idx32, x32, _ = o32.sample_given(u, noise, theta)
    return u, noise, idx64, x64, idx32, x32, gap > 1e-6


@functools.lru_cache(maxsize=None)
def joint_reference(name, log_x, large=False):
    """log p of a whole pool in the fp32 and the fp64 restatement."""
    o32, o64 = mnle_pair_cpu(name, log_x)[:2]
    theta, x = pool(name, log_x, large)
    with torch.no_grad():
        return o32.log_prob(x, theta), o64.log_prob(x.double(), theta.double())


def training_reference(o, x, theta, w):
    """(per-row losses, flat parameter gradient, d / d theta) of sum_i w_i loss_i by autograd in the restatement's own
    precision, returned as fp64."""
    dt = next(o.parameters()).dtype
    o.zero_grad()
    th = theta.to(dt).clone().requires_grad_(True)
    loss = o.loss(x.to(dt), th)
    (loss * w.to(dt)).sum().backward()
    out = loss.detach().double(), o.flat_grads().double().clone(), th.grad.double().clone()
    o.zero_grad()
    return out


def training_distances(net, got, gth, gref, gth_ref):
    """(whole-gradient distance / max norm, worst block distance / max(|block|, 1e-3 scale) with its key, d / d theta
    distance / max norm) of a flat gradient and a condition gradient against fp64 references."""
    got, gth = got.double().cpu(), gth.double().cpu()
    scale = gref.abs().max().item()
    rel = (got - gref).abs().max().item() / scale
    worst, worst_key = 0.0, None
    for key, off, cnt, _ in net._slices():
        a, b = got[off: off + cnt], gref[off: off + cnt]
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale)
        if worst_key is None or e > worst:
            worst, worst_key = e, key
    e_th = (gth - gth_ref).abs().max().item() / gth_ref.abs().max().item()
    return rel, worst, worst_key, e_th
