"""fp64 restatement of include/sbi_amd_cond.h's grid moments: the yardstick for what the reference cannot give in fp64.

Per grid (R x R cells, cell i R + j at x = axes[d1][j], y = axes[d2][i]): m = max logp, w = exp(logp - m) in fp32,
coordinates centred in fp64 on the axis midpoint (a[0] + a[R-1]) / 2, six fp64 sums, rho from them.  A grid with a NaN,
with m = +-inf or with vx vy <= 0 has rho = NaN; its probs are NaN for a NaN or +inf, 0 when everything is -inf.
numpy only (no torch reductions), one grid at a time: slow and plain on purpose."""

import numpy as np
import torch


def grid_moments(logp: torch.Tensor, axes: torch.Tensor, pairs, g0: int = 0):
    """logp (G, R*R) fp32, axes (D, R) fp32, pairs list of (d1, d2): rho (G) fp64, probs (G, R, R) fp32, moments (G, 6)
    fp64 = S, Sx, Sy, Sxx, Syy, Sxy (NaN rows for grids with a NaN or an infinite maximum)."""
    lp = logp.detach().cpu().to(torch.float32)
    ax = axes.detach().cpu().to(torch.float32).numpy().astype(np.float64)
    G, R = lp.shape[0], axes.shape[1]
    P = len(pairs)
    rho = np.full(G, np.nan)
    probs = np.zeros((G, R, R), dtype=np.float32)
    moments = np.full((G, 6), np.nan)
    for g in range(G):
        d1, d2 = pairs[(g0 + g) % P]
        row = lp[g]
        if bool(torch.isnan(row).any()):
            probs[g] = np.nan
            continue
        m = row.max()
        if m == float("inf"):
            probs[g] = np.nan
            continue
        if m == float("-inf"):
            continue
        w32 = torch.exp(row - m)                       # fp32 subtraction and fp32 exp, like the kernel
        probs[g] = w32.numpy().reshape(R, R)
        w = probs[g].astype(np.float64)
        xc = ax[d1] - (ax[d1][0] + ax[d1][R - 1]) / 2
        yc = ax[d2] - (ax[d2][0] + ax[d2][R - 1]) / 2
        X, Y = np.meshgrid(xc, yc)                     # X[i, j] = xc[j], Y[i, j] = yc[i]
        S = w.sum()
        Sx, Sy = (w * X).sum(), (w * Y).sum()
        Sxx, Syy, Sxy = (w * X * X).sum(), (w * Y * Y).sum(), (w * X * Y).sum()
        moments[g] = (S, Sx, Sy, Sxx, Syy, Sxy)
        vx = Sxx / S - (Sx / S) ** 2
        vy = Syy / S - (Sy / S) ** 2
        if vx * vy > 0:
            rho[g] = (Sxy / S - Sx * Sy / S ** 2) / np.sqrt(vx * vy)
    return torch.from_numpy(rho), torch.from_numpy(probs), torch.from_numpy(moments)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in units of the last place between two fp32 tensors of equal sign pattern (NaN == NaN counts as 0)."""
    a, b = a.detach().cpu().to(torch.float32).contiguous(), b.detach().cpu().to(torch.float32).contiguous()
    both_nan = torch.isnan(a) & torch.isnan(b)
    ia, ib = a.view(torch.int32).to(torch.int64), b.view(torch.int32).to(torch.int64)
    d = (ia - ib).abs()
    return torch.where(both_nan, torch.zeros_like(d), d)
