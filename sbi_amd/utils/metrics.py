"""Acceptance metric of the hot path: the classifier two-sample test.

Same estimator and defaults as sbi/utils/metrics.py:56-175 (random forest with 100
trees, 5-fold CV, z-scored inputs, seed 1); 0.5 = indistinguishable samples.

The MMD estimators (sbi/utils/metrics.py:178-290) follow at the end: on a ROCm device one launch of
`sbi_amd_mmd_rbf_splits` (include/sbi_amd_mmd.h), elsewhere the eager-torch evaluation of sbi_amd/utils/mmd_splits.py.
"""

from __future__ import annotations

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
