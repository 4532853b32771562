"""Conditional posterior analysis: ``eval_conditional_density``, ``conditional_corrcoeff``, ``conditional_potential``,
``ConditionedMDN`` with sbi's names, signatures and defaults (sbi/analysis/conditional_density.py), and
``conditional_density_grids`` beyond sbi.

Routes of ``conditional_corrcoeff``:

* device route -- the density answers on a ROCm device and the grid kernels' envelope holds (resolution <= 1024,
  theta-dim <= 64): whole grids g = c P + p (condition c, pair p) are filled a chunk at a time
  (``sbi_amd_cond_grid_fill``), a chunk is ONE ``density.log_prob(rows)`` call, and one
  ``sbi_amd_cond_grid_moments`` launch reduces it to its correlation coefficients.  The mean over the conditions is
  taken in fp64 by torch.  Nothing is read back to the host before the result.  ``max_grid_rows`` (default 2^22) bounds
  the rows of one chunk; a grid's result does not depend on the chunking.
* loop route -- sbi's loop, one pair of one condition at a time, reduced by the same formula as torch ops.  It serves
  host tensors and everything outside the envelope; ``force_loop = True`` (module flag) pins it.

Deliberate departures from sbi (see sbi_amd/utils/conditional_density_utils.py): the correlation coefficient is
evaluated in fp64 on centred coordinates, and a degenerate grid gives NaN where sbi gives +-inf or an arbitrary
number.  Otherwise ``probs``, the raw log-probs and the shapes are sbi's.
"""

from __future__ import annotations

from typing import Any, Callable, List, Optional, Tuple, Union

import torch
from torch import Tensor

from sbi_amd.utils import conditional_density_utils as cdu
from sbi_amd.utils.conditional_density_utils import (ConditionedPotential, RestrictedPriorForConditional,
                                                     RestrictedTransformForConditional, compute_corrcoeff,
                                                     condition_mog, extract_and_transform_mog)
from sbi_amd.utils.torchutils import ensure_theta_batched

force_loop = False                 # True: `conditional_corrcoeff` / `eval_conditional_density` never take the kernels
DEFAULT_MAX_GRID_ROWS = 1 << 22


def _device_of(density: Any) -> torch.device:
    return torch.device(density._device if hasattr(density, "_device") else "cpu")


def _axis(limits: Tensor, dim: int, eps: Union[Tensor, float], resolution: int, device) -> Tensor:
    return torch.linspace(float(limits[dim, 0] + eps), float(limits[dim, 1] - eps), resolution, device=device)


def _axes(limits: Tensor, resolution: int, device) -> Tensor:
    """(D, R): the grid points of every dimension, the values `eval_conditional_density` evaluates at."""
    return torch.stack([_axis(limits, d, 1e-32, resolution, device) for d in range(limits.shape[0])]).contiguous()


def _on_kernels(device: torch.device, dim: int, resolution: int) -> bool:
    return (not force_loop) and device.type == "cuda" and cdu.in_envelope(dim, resolution)


def _eager_rows(condition: Tensor, axis1: Tensor, axis2: Tensor, dim1: int, dim2: int) -> Tensor:
    """The theta rows of one grid by torch ops: dim1 runs fastest (row i R + j holds axis1[j] and axis2[i])."""
    R = axis1.shape[0]
    if dim1 == dim2:
        rows = condition.repeat(R, 1)
        rows[:, dim1] = axis1
        return rows
    rows = condition.repeat(R * R, 1)
    rows[:, dim1] = axis1.repeat(R)
    rows[:, dim2] = axis2.repeat_interleave(R)
    return rows


def eval_conditional_density(density: Any, condition: Tensor, limits: Tensor, dim1: int, dim2: int,
                             resolution: int = 50, eps_margins1: Union[Tensor, float] = 1e-32,
                             eps_margins2: Union[Tensor, float] = 1e-32, return_raw_log_prob: bool = False) -> Tensor:
    r"""Return the unnormalized conditional along `dim1, dim2` given `condition`.

    The joint density is evaluated on an evenly spaced grid inside `limits` with every other dimension fixed to
    `condition` (shape (1, dim_theta)): $p(x_1 | x_2) \propto p(x_1, x_2)$.

    Args:
        density: Probability density function with `.log_prob()` method.
        condition: Parameter set that all dimensions other than dim1 and dim2 are fixed to.
        limits: Bounds within which to evaluate the density. Shape (dim_theta, 2).
        dim1, dim2: The dimensions along which to evaluate the conditional.
        resolution: Resolution of the grid.
        eps_margins1, eps_margins2: Margin kept from the limits along `dim1` / `dim2`.
        return_raw_log_prob: If `True`, return the log-probability on the grid; otherwise the probability scaled by
            its maximum on the grid (exp(log_prob - max_log_prob)).

    Returns: Conditional probabilities, shape (resolution) if `dim1 == dim2`, else (resolution, resolution).
    """
    condition = ensure_theta_batched(torch.as_tensor(condition))
    dev = condition.device
    axis1 = _axis(limits, dim1, eps_margins1, resolution, dev)
    axis2 = _axis(limits, dim2, eps_margins2, resolution, dev)
    D = condition.shape[1]
    if _on_kernels(dev, D, resolution) and condition.dtype == torch.float32 and condition.shape[0] == 1:
        # fill + moments with one grid: only the two axes in use are gathered, so the other rows of `axes` stay zero
        axes = torch.zeros(D, resolution, dtype=torch.float32, device=dev)
        axes[dim1] = axis1
        axes[dim2] = axis2
        pairs_host = [(dim1, dim2)]
        pairs = cdu.pairs_tensor(pairs_host, dev)
        mode = 1 if dim1 == dim2 else 2
        rows = cdu.grid_fill(condition.contiguous(), axes, pairs_host, pairs, mode, 0, 1)
        log_probs = density.log_prob(rows)
        if mode == 1:
            return log_probs if return_raw_log_prob else torch.exp(log_probs - torch.max(log_probs))
        if return_raw_log_prob:
            return log_probs.reshape(resolution, resolution)
        lp = log_probs.reshape(1, resolution * resolution).to(torch.float32).contiguous()
        return cdu.grid_moments(lp, axes, pairs_host, pairs, want_probs=True)[1][0]
    log_probs = density.log_prob(_eager_rows(condition, axis1, axis2, dim1, dim2))
    if dim1 != dim2:
        log_probs = log_probs.reshape(resolution, resolution)
    if return_raw_log_prob:
        return log_probs
    return torch.exp(log_probs - torch.max(log_probs))


def _subset_pairs(subset_: List[int]) -> List[Tuple[int, int]]:
    """sbi's order: every (dim1, dim2) of the subset with dim1 < dim2, dim1 outermost."""
    return [(d1, d2) for d1 in subset_ for d2 in subset_ if d1 < d2]


def _pair_matrix_positions(subset_: List[int], pairs: List[Tuple[int, int]]) -> Tuple[List[int], List[int]]:
    """Where the coefficient of each pair goes.  sbi writes its list into the upper triangle in order, which matches the
    pairs only for a sorted subset; here entry (a, b) of the matrix always belongs to (subset[a], subset[b])."""
    pos = {d: a for a, d in enumerate(subset_)}
    return [pos[d1] for d1, _ in pairs], [pos[d2] for _, d2 in pairs]


def _assemble(avg: Tensor, subset_: List[int], pairs: List[Tuple[int, int]], device) -> Tensor:
    n = len(subset_)
    out = torch.zeros(n, n, device=device, dtype=torch.float32)
    if pairs:
        ra, rb = _pair_matrix_positions(subset_, pairs)
        ia, ib = torch.tensor(ra, device=device), torch.tensor(rb, device=device)
        vals = avg.to(torch.float32)
        out[ia, ib] = vals
        out[ib, ia] = vals
    out.fill_diagonal_(1.0)
    return out


def _corrcoeff_device(density: Any, limits: Tensor, condition: Tensor, pairs_host: List[Tuple[int, int]],
                      resolution: int, max_grid_rows: int, device: torch.device) -> Tensor:
    """rho (C, P) in fp32 on the device: fill, one log_prob call and one moments launch per chunk of whole grids."""
    C, D = condition.shape
    P, cells = len(pairs_host), resolution * resolution
    axes = _axes(limits, resolution, device)
    pairs = cdu.pairs_tensor(pairs_host, device)
    G = C * P
    per_chunk = max(1, int(max_grid_rows) // cells)
    rho = torch.empty(G, dtype=torch.float32, device=device)
    for g0 in range(0, G, per_chunk):
        g1 = min(G, g0 + per_chunk)
        rows = cdu.grid_fill(condition, axes, pairs_host, pairs, 2, g0, g1)
        lp = density.log_prob(rows).reshape(g1 - g0, cells).to(torch.float32).contiguous()
        rho[g0:g1] = cdu.grid_moments(lp, axes, pairs_host, pairs, g0=g0)[0]
    return rho.reshape(C, P)


def _corrcoeff_loop(density: Any, limits: Tensor, condition: Tensor, pairs_host: List[Tuple[int, int]],
                    resolution: int, device: torch.device) -> Tensor:
    """rho (C, P) in fp64: one grid per `log_prob` call, the centred fp64 formula as torch ops."""
    limits = limits.to(device)
    rows = []
    for cond in condition:
        rows.append(torch.stack([
            cdu.corrcoeff_of_weights(
                eval_conditional_density(density, cond, limits, dim1=d1, dim2=d2, resolution=resolution),
                _axis(limits, d1, 0.0, resolution, device), _axis(limits, d2, 0.0, resolution, device))
            for d1, d2 in pairs_host]))
    return torch.stack(rows)


def conditional_corrcoeff(density: Any, limits: Tensor, condition: Tensor, subset: Optional[List[int]] = None,
                          resolution: int = 50, max_grid_rows: int = DEFAULT_MAX_GRID_ROWS) -> Tensor:
    r"""Returns the conditional correlation matrix of a distribution.

    All but two parameters are fixed to the values of `condition`, and the Pearson correlation coefficient $\rho$ of
    the remaining two under `density` is computed on a grid; this is done for every pair of parameters in `subset`.
    For a batch of conditions the matrices are averaged.

    Args:
        density: Probability density function with `.log_prob()` function.
        limits: Limits within which to evaluate the `density`.
        condition: Values to condition the `density` on, (num_conditions, dim_theta).
        subset: Evaluate the conditional distribution only on a subset of dimensions (all if `None`).
        resolution: Number of grid points per dimension.
        max_grid_rows: (beyond sbi) the most theta rows handed to one `density.log_prob` call on the device route;
            whole grids only, at least one.

    Returns: Average conditional correlation matrix of shape either `(num_dim, num_dim)` or
    `(len(subset), len(subset))` if `subset` was specified.
    """
    device = _device_of(density)
    condition = ensure_theta_batched(torch.as_tensor(condition, dtype=torch.float32)).to(device).contiguous()
    limits = torch.as_tensor(limits)
    subset_ = list(subset) if subset is not None else list(range(condition.shape[1]))
    pairs_host = _subset_pairs(subset_)
    if not pairs_host:
        return _assemble(torch.empty(0), subset_, pairs_host, device)
    D = condition.shape[1]
    if _on_kernels(device, D, resolution) and limits.shape[0] == D:
        rho = _corrcoeff_device(density, limits, condition, pairs_host, resolution, max_grid_rows, device)
    else:
        rho = _corrcoeff_loop(density, limits, condition, pairs_host, resolution, device)
    return _assemble(rho.to(torch.float64).mean(dim=0), subset_, pairs_host, device)


def conditional_density_grids(density: Any, condition: Tensor, limits: Tensor, subset: Optional[List[int]] = None,
                              resolution: int = 50) -> Tuple[Tensor, Tensor, List[Tuple[int, int]]]:
    """(beyond sbi) Every 1-D and 2-D conditional of ONE condition, what a conditional pair plot shows.

    Returns `(diag, offdiag, pairs)`: diag (len(subset), R) with row a the conditional along subset[a]; offdiag
    (len(pairs), R, R) with entry [i, j] at (dim1 = axis[j], dim2 = axis[i]) like `eval_conditional_density`; `pairs`
    the (dim1, dim2) of each 2-D grid (dim1 < dim2).  Each grid is scaled by its own maximum.  On the device this is one
    mode-1 and one mode-2 fill, two `log_prob` calls and one moments launch; elsewhere a loop over
    `eval_conditional_density`."""
    device = _device_of(density)
    condition = ensure_theta_batched(torch.as_tensor(condition, dtype=torch.float32)).to(device).contiguous()
    if condition.shape[0] > 1:
        raise ValueError("Condition with batch size > 1 not supported.")
    limits = torch.as_tensor(limits)
    D = condition.shape[1]
    subset_ = list(subset) if subset is not None else list(range(D))
    pairs_host = _subset_pairs(subset_)
    R = resolution
    if _on_kernels(device, D, R) and limits.shape[0] == D:
        axes = _axes(limits, R, device)
        ones_host = [(d, d) for d in subset_]
        lp1 = density.log_prob(cdu.grid_fill(condition, axes, ones_host, cdu.pairs_tensor(ones_host, device), 1, 0,
                                             len(ones_host))).reshape(len(ones_host), R)
        diag = torch.exp(lp1 - lp1.max(dim=1, keepdim=True).values)
        if not pairs_host:
            return diag, torch.empty(0, R, R, device=device), pairs_host
        pairs = cdu.pairs_tensor(pairs_host, device)
        rows = cdu.grid_fill(condition, axes, pairs_host, pairs, 2, 0, len(pairs_host))
        lp2 = density.log_prob(rows).reshape(len(pairs_host), R * R).to(torch.float32).contiguous()
        return diag, cdu.grid_moments(lp2, axes, pairs_host, pairs, want_probs=True)[1], pairs_host
    lim = limits.to(device)
    diag = torch.stack([eval_conditional_density(density, condition, lim, d, d, resolution=R) for d in subset_])
    off = [eval_conditional_density(density, condition, lim, d1, d2, resolution=R) for d1, d2 in pairs_host]
    return diag, (torch.stack(off) if off else torch.empty(0, R, R, device=device)), pairs_host


class ConditionedMDN:
    def __init__(self, mdn: Any, x_o: Tensor, condition: Tensor, dims_to_sample: List[int]) -> None:
        r"""Class that can sample and evaluate a conditional mixture-of-gaussians.

        The mixture of `mdn` at `x_o` is conditioned in closed form by the module-level `condition_mog` (host, fp64);
        the result is an ordinary `MoG`, whose `log_prob` / `sample` run on the `sbi_amd_mog_*` kernels on a device.

        Args:
            mdn: MixtureDensityEstimator that models $p(\theta|x)$.
            x_o: The datapoint at which the `net` is evaluated.
            condition: Parameter set that all dimensions not specified in `dims_to_sample` will be fixed to
                (dim_theta elements; the entries at `dims_to_sample` are ignored).
            dims_to_sample: Which dimensions to sample from.
        """
        from sbi_amd.neural_nets.estimators.mdn import MoG

        condition = torch.atleast_2d(torch.as_tensor(condition, dtype=torch.float32))
        logits, means, precfs, _ = extract_and_transform_mog(estimator=mdn, context=x_o)
        cond_logits, cond_means, cond_precfs, _ = condition_mog(condition, dims_to_sample, logits, means, precfs)
        self._mog = MoG(logits=cond_logits, means=cond_means,
                        precisions=cond_precfs.transpose(3, 2) @ cond_precfs, precision_factors=cond_precfs)

    def sample(self, sample_shape=torch.Size()) -> Tensor:
        """Samples (*sample_shape, len(dims_to_sample)) from the conditioned MoG."""
        return self._mog.sample(torch.Size(sample_shape)).squeeze(-2).detach()

    def log_prob(self, theta: Tensor) -> Tensor:
        """Log probability of theta (dim,) or (batch_size, dim) under the conditioned MoG: shape (1,) or (batch_size,)."""
        if theta.dim() == 1:
            theta = theta.unsqueeze(0)
        return self._mog.log_prob(theta.to(self._mog.device))


def conditional_potential(potential_fn: Any, theta_transform: Any, prior: Any, condition: Tensor,
                          dims_to_sample: List[int]) -> Tuple[Callable, Any, Any]:
    r"""Returns potential function that can be used to sample the conditional potential, with the transform and the
    prior restricted to `dims_to_sample`.

    The conditional potential is $p(\theta_i | \theta_j, x_o) \propto p(\theta | x_o)$ as a function of $\theta_i$
    only.  The three objects go to ``MCMCPosterior(potential, proposal=restricted_prior,
    theta_transform=restricted_tf)``.

    Returns:
        A conditioned potential function, conditioned parameter transformation, and a marginalised prior.
    """
    restricted_tf = RestrictedTransformForConditional(theta_transform, condition, dims_to_sample)
    condition = torch.atleast_2d(torch.as_tensor(condition, dtype=torch.float32))
    conditioned_potential_fn = ConditionedPotential(potential_fn, condition, dims_to_sample)
    restricted_prior = RestrictedPriorForConditional(prior, dims_to_sample)
    return conditioned_potential_fn, restricted_tf, restricted_prior
