"""Acceptance metric of the hot path: the classifier two-sample test.

Same estimator and defaults as sbi/utils/metrics.py:56-175 (random forest with 100
trees, 5-fold CV, z-scored inputs, seed 1); 0.5 = indistinguishable samples.

The MMD estimators (sbi/utils/metrics.py:178-290) follow at the end: on a ROCm device one launch of
`sbi_amd_mmd_rbf_splits` (include/sbi_amd_mmd.h), elsewhere the eager-torch evaluation of sbi_amd/utils/mmd_splits.py.

The distances of the ABC samplers (`Distance`, `l1`, `mse_distance`, `mmd_distance`, `wasserstein_distance`,
`wasserstein_2_squared`, `regularized_ot_dual`; sbi/utils/metrics.py:293-707) close the file.
"""

from __future__ import annotations

import warnings
from functools import partial
from typing import Optional

import numpy as np
import torch
from torch import Tensor


def c2st(X: Tensor, Y: Tensor, seed: int = 1, n_folds: int = 5, metric: str = "accuracy",
         classifier: str = "rf", z_score: bool = True, noise_scale=None, verbosity: int = 0) -> Tensor:
    """Cross-validated accuracy of a classifier telling X from Y."""
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import KFold, cross_val_score
    from sklearn.neural_network import MLPClassifier

    X, Y = X.detach().cpu(), Y.detach().cpu()
    if z_score:
        X_mean, X_std = torch.mean(X, dim=0), torch.std(X, dim=0)
        X_std[X_std == 0] = 1.0   # constant dims stay constant instead of turning into NaN
        X = (X - X_mean) / X_std
        Y = (Y - X_mean) / X_std
    if noise_scale is not None:
        X = X + noise_scale * torch.randn(X.shape)
        Y = Y + noise_scale * torch.randn(Y.shape)
    ndim = X.shape[-1]
    if classifier == "rf":
        clf = RandomForestClassifier(random_state=seed)
    elif classifier == "mlp":
        clf = MLPClassifier(activation="relu", hidden_layer_sizes=(10 * ndim, 10 * ndim), max_iter=1000,
                            solver="adam", early_stopping=True, n_iter_no_change=50, random_state=seed)
    else:
        raise ValueError(f"Invalid classifier: {classifier}. Use 'rf' or 'mlp'.")
    data = np.concatenate((X.numpy(), Y.numpy()))
    target = np.concatenate((np.zeros(X.shape[0]), np.ones(Y.shape[0])))
    shuffle = KFold(n_splits=n_folds, shuffle=True, random_state=seed)
    scores = cross_val_score(clf, data, target, cv=shuffle, scoring=metric, verbose=verbosity)
    return torch.from_numpy(np.atleast_1d(np.mean(scores).astype(np.float32)))


def check_c2st(x: Tensor, y: Tensor, alg: str, tol: float = 0.1) -> None:
    """Raise if the C2ST accuracy is further than ``tol`` from chance (0.5)."""
    score = c2st(x, y).item()
    print(f"c2st for {alg} is {score:.2f}.")
    assert (0.5 - tol) <= score <= (0.5 + tol), (
        f"{alg}'s c2st={score:.2f} is too far from the desired near-chance performance."
    )


def l2(x: Tensor, y: Tensor, axis: int = -1) -> Tensor:
    """Euclidean distance along `axis` (sbi/utils/metrics.py `l2`; the default distance of TARP)."""
    return torch.sqrt(torch.sum((x - y) ** 2, dim=axis))



def _mmd_sums(x: Tensor, y: Tensor, pair_set: int, scale, bw_floor: float) -> Tensor:
    """[bw, S_xx, S_yy, S_xy] with the bandwidth `scale`, or the median over the cross pairs and the within-set pairs
    of `pair_set` (0: all ordered pairs with the diagonal, 1: the strict lower triangle)."""
    from sbi_amd.utils.mmd_splits import rbf_splits

    nx, ny = x.shape[0], y.shape[0]
    pool = torch.cat((x.reshape(nx, -1), y.reshape(ny, -1).to(x.device)))
    idx = torch.arange(nx + ny, device=pool.device).reshape(1, -1)
    bw = None
    if scale is not None:
        bw = torch.as_tensor(scale, dtype=torch.float32, device=pool.device).reshape(1).clamp(min=bw_floor)
    return rbf_splits(pool, 1, nx + ny, nx, pair_set, 1, idx=idx, bandwidth=bw, bw_floor=bw_floor)[0].double()


def unbiased_mmd_squared(x: Tensor, y: Tensor, scale: Optional[float] = None):
    """Unbiased estimate of the squared maximum-mean discrepancy with a Gaussian kernel of lengthscale `scale`
    (Gretton et al. 2012, "A kernel two-sample test").  x: (m, d), y: (n, d).  Without `scale` the lengthscale is the
    median of the distances over the cross pairs and the strict lower triangles of x and of y; either is kept above
    1e-8.  The reference's normalisation as written: 2 (kxx + kyy - kxy), kxx = (sum over the strict lower triangle) /
    (m (m - 1)).  A 0-dim fp32 tensor."""
    nx, ny = x.shape[0], y.shape[0]
    assert nx != 1 and ny != 1, "The unbiased MMD estimator is not defined for empirical distributions of size 1."
    s = _mmd_sums(x, y, 1, scale, 1e-8)
    kxx = s[1] / (nx * (nx - 1))
    kxy = s[3] / (nx * ny)
    kyy = s[2] / (ny * (ny - 1))
    return (2 * (kxx + kyy - kxy)).to(torch.float32)


def biased_mmd(x: Tensor, y: Tensor, scale: Optional[float] = None):
    """Biased estimate of the maximum-mean discrepancy (the square root of kxx - 2 kxy + kyy, every mean over all
    ordered pairs) with a Gaussian kernel of lengthscale `scale`; without `scale`, the median of all m^2 + m n + n^2
    distances.  A 0-dim fp32 tensor."""
    nx, ny = x.shape[0], y.shape[0]
    s = _mmd_sums(x, y, 0, scale, 0.0)
    kxx = s[1] / nx**2
    kxy = s[3] / (nx * ny)
    kyy = s[2] / ny**2
    return torch.sqrt(kxx - 2 * kxy + kyy).to(torch.float32)


def biased_mmd_hypothesis_test(x: Tensor, y: Tensor, alpha=0.05):
    """(biased MMD, its acceptance threshold at level alpha) for two samples of one size (Gretton et al. 2012)."""
    assert x.shape[0] == y.shape[0]
    mmd_biased = biased_mmd(x, y).item()
    threshold = np.sqrt(2 / x.shape[0]) * (1 + np.sqrt(-2 * np.log(alpha)))
    return mmd_biased, threshold


def unbiased_mmd_squared_hypothesis_test(x: Tensor, y: Tensor, alpha=0.05):
    """(unbiased squared MMD, its acceptance threshold at level alpha) for two samples of one size."""
    assert x.shape[0] == y.shape[0]
    mmd_square_unbiased = unbiased_mmd_squared(x, y).item()
    threshold = (4 / np.sqrt(x.shape[0])) * np.sqrt(-np.log(alpha))
    return mmd_square_unbiased, threshold


# ---- ABC distances (sbi/utils/metrics.py `Distance` and what it wraps) ------------------------------------------------
# Entropic optimal transport: on a ROCm device one launch of `sbi_amd_sinkhorn` (include/sbi_amd_abc.h: one workgroup
# per problem, all iterations on the device); for host tensors and problems outside its LDS budget the eager
# composition `sinkhorn_torch` of the same iteration.

SINKHORN_LDS_FLOATS = 40_000     # SBI_AMD_SINKHORN_LDS_FLOATS of include/sbi_amd_abc.h


def sinkhorn_fits(m: int, n: int) -> bool:
    """Whether an (m, n) problem fits the Sinkhorn kernel's LDS budget."""
    return m * (n | 1) + 5 * (m + n) + 16 <= SINKHORN_LDS_FLOATS


def squared_distances(x: Tensor, y: Tensor) -> Tensor:
    """(..., m, n) squared Euclidean distances from differences (never |a|^2 + |b|^2 - 2 a.b)."""
    return ((x.unsqueeze(-2) - y.unsqueeze(-3)) ** 2).sum(-1)


def sinkhorn_torch(cost: Tensor, a: Tensor, b: Tensor, epsilon: float, max_iter: int, tol: float):
    """The fallback: (f, g, iters) of the log-domain dual iteration on (B, m, n) costs.  f is updated from the old g, g
    from the new f; a problem is frozen after the first iteration with err = max(sum |df|, sum |dg|) < tol (that
    update is kept); iters counts the iterations a problem executed."""
    f, g = torch.zeros_like(a), torch.zeros_like(b)
    log_a, log_b = torch.log(a), torch.log(b)
    done = torch.zeros(a.shape[0], dtype=torch.bool, device=a.device)
    iters = torch.zeros(a.shape[0], dtype=torch.int32, device=a.device)
    for _ in range(max_iter):
        f_new = f + epsilon * (log_a - torch.logsumexp(((f[:, :, None] - cost) + g[:, None, :]) / epsilon, dim=2))
        g_new = g + epsilon * (log_b - torch.logsumexp(((f_new[:, :, None] - cost) + g[:, None, :]) / epsilon, dim=1))
        f_new, g_new = torch.where(done[:, None], f, f_new), torch.where(done[:, None], g, g_new)
        err = torch.maximum((f - f_new).abs().sum(1), (g - g_new).abs().sum(1))
        iters = iters + (~done).to(torch.int32)
        f, g = f_new, g_new
        done = done | (err < tol)
        if bool(done.all()):
            break
    return f, g, iters


def _sinkhorn(x: Optional[Tensor], y: Optional[Tensor], cost: Optional[Tensor], a: Optional[Tensor],
              b: Optional[Tensor], B: int, epsilon: float, max_iter: int, tol: float, force_fallback: bool = False):
    """(f, g, w, iters) for B problems.  x (m, D) shared or (B, m, D), y (B, n, D) -- or cost (B, m, n); a, b (B, m),
    (B, n) or None (uniform).  The kernel when everything is on a ROCm device and the problem fits, else eager torch."""
    ref = cost if cost is not None else y
    dev = ref.device

    def f32(t):
        return None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()

    x, y, cost, a, b = f32(x), f32(y), f32(cost), f32(a), f32(b)
    m, n = (cost.shape[1], cost.shape[2]) if cost is not None else (x.shape[-2], y.shape[-2])
    if ref.is_cuda and not force_fallback and sinkhorn_fits(m, n):
        from sbi_amd import _lib

        lib = _lib.load()
        _lib.require_device(ref, x, y, a, b)
        D = 0 if cost is not None else x.shape[-1]
        stride = 0 if (x is None or x.dim() == 2) else m * D
        f = torch.empty((B, m), dtype=torch.float32, device=dev)
        g = torch.empty((B, n), dtype=torch.float32, device=dev)
        w = torch.empty((B,), dtype=torch.float32, device=dev)
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.sbi_amd_sinkhorn(_lib.ptr(x), stride, m, _lib.ptr(y), n, D, _lib.ptr(cost), _lib.ptr(a),
                                      _lib.ptr(b), B, float(epsilon), int(max_iter), float(tol), _lib.ptr(f),
                                      _lib.ptr(g), _lib.ptr(w), _lib.ptr(iters), _lib.current_stream(dev))
        if rc != _lib.E_UNSUPPORTED:
            _lib.check(rc, "sinkhorn")
            return f, g, w, iters
    if cost is None:
        cost = squared_distances(x if x.dim() == 3 else x.unsqueeze(0).expand(B, m, x.shape[-1]), y)
    if a is None:
        a = torch.full((B, m), 1.0 / m, dtype=torch.float32, device=dev)
    if b is None:
        b = torch.full((B, n), 1.0 / n, dtype=torch.float32, device=dev)
    f, g, iters = sinkhorn_torch(cost, a, b, epsilon, max_iter, tol)
    w = (torch.exp(((f[:, :, None] - cost) + g[:, None, :]) / epsilon) * cost).sum(dim=(1, 2))
    return f, g, w, iters


def regularized_ot_dual(a: Tensor, b: Tensor, cost: Tensor, epsilon: float = 1e-3, max_iter: int = 1000, tol=1e-9):
    """The entropic optimal-transport coupling, (B, m, n) or (m, n), from the dual (Sinkhorn) iteration (Peyre &
    Cuturi 2019).  a: (B, m) or (m,), b: (B, n) or (n,), cost: (B, m, n) or (m, n).  No warning is given when
    max_iter is reached (the reference's never fires: its counter is compared before it is incremented)."""
    assert a.ndim == b.ndim, "Please make sure that 'a' and 'b' are both either batched or not."
    batched = a.ndim != 1
    if not batched:
        a, b, cost = a.unsqueeze(0), b.unsqueeze(0), cost.unsqueeze(0)
    a, b = a.to(cost.device), b.to(cost.device)
    f, g, _, _ = _sinkhorn(None, None, cost, a, b, cost.shape[0], epsilon, max_iter, tol)
    coupling = torch.exp(((f[:, :, None] - cost.to(torch.float32)) + g[:, None, :]) / epsilon)
    return coupling if batched else coupling.squeeze(0)


def wasserstein_2_squared(x: Tensor, y: Tensor, epsilon: float = 1e-3, max_iter: int = 1000, tol: float = 1e-9):
    """The squared 2-Wasserstein distance approximated by entropic regularised optimal transport between the uniform
    empirical distributions on x ((B, m, d) or (m, d)) and y ((B, n, d) or (n, d)): shape (B,) or ()."""
    assert x.ndim == y.ndim, "Please make sure that 'x' and 'y' are both either batched or not."
    if x.ndim not in (2, 3):
        raise ValueError("This implementation of Wasserstein is only implemented, if x.ndim=2 or x.ndim=3.")
    batched = x.ndim == 3
    if not batched:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    w = _sinkhorn(x.to(y.device), y, None, None, None, y.shape[0], epsilon, max_iter, tol)[2]
    return w if batched else w[0]


def l1(x: Tensor, y: Tensor, axis: int = -1) -> Tensor:
    """Mean absolute difference along `axis`."""
    return torch.mean(torch.abs(x - y), dim=axis)


def mse_distance(x_o: Tensor, x: Tensor) -> Tensor:
    """Mean squared difference along the last axis."""
    return torch.mean((x_o - x) ** 2, dim=-1)


def mmd_distance(x_o: Tensor, x: Tensor, scale: Optional[float] = None) -> Tensor:
    """`unbiased_mmd_squared(x_o, x[b])` for every simulated set b: x_o (n_o, d), x (B, m, d) -> (B,).  One launch of
    the split kernel: the pool is x_o followed by the B sets, split b = rows of x_o, then rows of set b."""
    n_o, B, m = x_o.shape[0], x.shape[0], x.shape[1]
    assert n_o != 1 and m != 1, "The unbiased MMD estimator is not defined for empirical distributions of size 1."
    from sbi_amd.utils.mmd_splits import rbf_splits

    pool = torch.cat((x_o.reshape(n_o, -1).to(x.device), x.reshape(B * m, -1)))
    idx = torch.cat((torch.arange(n_o, device=x.device).expand(B, n_o),
                     n_o + torch.arange(B * m, device=x.device).reshape(B, m)), dim=1)
    bw = None
    if scale is not None:
        bw = torch.as_tensor(scale, dtype=torch.float32, device=x.device).reshape(1).clamp(min=1e-8).expand(B)
    s = rbf_splits(pool, B, n_o + m, n_o, 1, 1, idx=idx, bandwidth=bw, bw_floor=1e-8).double()
    return (2 * (s[:, 1] / (n_o * (n_o - 1)) + s[:, 2] / (m * (m - 1)) - s[:, 3] / (n_o * m))).to(torch.float32)


def wasserstein_distance(x_o: Tensor, x: Tensor, epsilon: float = 1e-3, max_iter: int = 1000,
                         tol: float = 1e-9) -> Tensor:
    """`wasserstein_2_squared(x_o, x[b])` for every simulated set b: x_o (n_o, d), x (B, m, d) -> (B,).  x_o is never
    repeated: every problem reads the one copy."""
    return _sinkhorn(x_o.to(x.device), x, None, None, None, x.shape[0], epsilon, max_iter, tol)[2]


class Distance:
    """The distance between the observation and simulated data of the ABC samplers: a name ('l1', 'l2', 'mse' compare
    single data points; 'mmd', 'wasserstein' compare sets of iid data points) or a callable (x_o, x) -> (batch,)."""

    def __init__(self, distance, requires_iid_data: Optional[bool] = None, distance_kwargs: Optional[dict] = None,
                 batch_size: int = -1):
        self.distance_kwargs = distance_kwargs or {}
        self.batch_size = batch_size
        if callable(distance):
            if requires_iid_data is None:
                warnings.warn("Please specify if your the custom distance requires iid data or is evaluated between "
                              "single datapoints. By default, we assume that `requires_iid_data=False`", stacklevel=2)
                requires_iid_data = False
            self.distance_fn = distance
            self._requires_iid_data = requires_iid_data
            return
        pairwise, statistical = ["l1", "l2", "mse"], ["mmd", "wasserstein"]
        assert distance in pairwise + statistical, f"{distance} must be one of {pairwise + statistical}."
        self._requires_iid_data = distance in statistical
        self.distance_fn = {"mse": mse_distance, "l2": l2, "l1": l1,
                            "mmd": partial(mmd_distance, **self.distance_kwargs),
                            "wasserstein": partial(wasserstein_distance, **self.distance_kwargs)}[distance]

    def __call__(self, x_o: Tensor, x: Tensor) -> Tensor:
        if self.requires_iid_data:
            assert x.ndim >= 3, "simulated data needs batch dimension"
            assert x_o.ndim + 1 == x.ndim
        else:
            assert x.ndim >= 2, "simulated data needs batch dimension"
        if self.batch_size == -1:
            return self.distance_fn(x_o, x)
        return self._batched_distance(x_o, x)

    def _batched_distance(self, x_o: Tensor, x: Tensor) -> Tensor:
        """The distance in chunks of `batch_size` simulations (statistical distances over two large sets can exhaust
        memory).  Every simulation is covered: the chunks tile the batch, the last one may be shorter."""
        distances = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        for s in range(0, x.shape[0], self.batch_size):
            distances[s:s + self.batch_size] = self.distance_fn(x_o, x[s:s + self.batch_size])
        return distances

    @property
    def requires_iid_data(self):
        return self._requires_iid_data
