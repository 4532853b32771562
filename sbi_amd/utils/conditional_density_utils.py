"""Conditional densities: correlation coefficient on a grid, conditioned potentials, conditioned mixtures.

sbi's names and signatures (sbi/utils/conditional_density_utils.py): ``compute_corrcoeff``, ``ConditionedPotential``,
``RestrictedPriorForConditional``, ``RestrictedTransformForConditional``, ``condition_mog``,
``extract_and_transform_mog``.  The grid kernels of include/sbi_amd_cond.h are bound here as well
(``grid_fill``, ``grid_moments``, ``expand_condition``); ``sbi_amd.analysis`` builds its routes from them.

Deliberate departures from sbi:

* the correlation coefficient is evaluated in fp64 on coordinates centred at the axis midpoint.  sbi takes
  ``E[XY] - E[X] E[Y]`` in fp32 on the raw coordinates, which loses 2.5e-2 with limits [98, 102] and returns inf with
  limits around 1000; the centred fp64 sums stay within 2e-8 there;
* on a degenerate grid -- a NaN, an infinite maximum, or no spread along an axis (variance product <= 0) -- the result
  is NaN where sbi returns +-inf or an arbitrary number.  On every other grid ``probs``, the raw log-probs and all
  shapes are sbi's.

``RestrictedTransformForConditional`` is a complete ``torch.distributions`` transform (``_call`` / ``_inverse``), so
``.inv`` is torch's inverse transform and ``tf.inv(theta)`` reads as in sbi.
"""

from __future__ import annotations

import math
from typing import Any, List, Optional, Sequence, Tuple

import torch
import torch.distributions.transforms as torch_tf
from torch import Tensor
from torch.distributions import constraints

from sbi_amd import _lib
from sbi_amd.utils.sbiutils import process_x
from sbi_amd.utils.torchutils import ensure_theta_batched

MAX_RESOLUTION, MAX_DIM, EXPAND_MAX_DIM = 1024, 64, 1024
ENVELOPE = "conditional grid kernels: 1 <= resolution <= 1024, 1 <= theta-dim <= 64"


def in_envelope(dim: int, resolution: int) -> bool:
    return 1 <= dim <= MAX_DIM and 1 <= resolution <= MAX_RESOLUTION


# ------------------------------------------------------------------------------------------------ host formula
def corrcoeff_of_weights(weights: Tensor, axis_x: Tensor, axis_y: Tensor) -> Tensor:
    """rho (...,) in fp64 of the weights (..., R, R): cell [i, j] sits at x = axis_x[j], y = axis_y[i].  The formula of
    include/sbi_amd_cond.h as torch ops: fp64 sums on coordinates centred at the axis midpoints; NaN for a grid that
    holds a NaN or an inf, has no mass, or has no spread along an axis."""
    w = weights.to(torch.float64)
    ax, ay = axis_x.to(torch.float64), axis_y.to(torch.float64)
    xc = ax - (ax[0] + ax[-1]) / 2
    yc = ay - (ay[0] + ay[-1]) / 2
    col, row = w.sum(-2), w.sum(-1)                   # mass over x (index j) and over y (index i)
    S = col.sum(-1)
    wx, wy = col * xc, row * yc
    mx, my = wx.sum(-1) / S, wy.sum(-1) / S
    vx = (wx * xc).sum(-1) / S - mx * mx
    vy = (wy * yc).sum(-1) / S - my * my
    cov = ((w * xc).sum(-1) * yc).sum(-1) / S - mx * my
    vv = vx * vy
    ok = torch.isfinite(S) & (S > 0) & (vv > 0)
    rho = cov / torch.sqrt(torch.where(ok, vv, torch.ones_like(vv)))
    return torch.where(ok, rho, torch.full_like(rho, float("nan")))


def compute_corrcoeff(probs: Tensor, limits: Tensor) -> Tensor:
    """
    Given a matrix of probabilities `probs`, return the correlation coefficient.

    Args:
        probs: Matrix of (unnormalized) evaluations of a 2D density.
        limits: Limits within which the entries of the matrix are evenly spaced.

    Returns: Pearson correlation coefficient.
    """
    limits = ensure_theta_batched(torch.as_tensor(limits))
    R_y, R_x = probs.shape[-2:]
    axis_x = torch.linspace(float(limits[0, 0]), float(limits[0, 1]), R_x, device=probs.device)
    axis_y = torch.linspace(float(limits[1, 0]), float(limits[1, 1]), R_y, device=probs.device)
    return corrcoeff_of_weights(probs, axis_x, axis_y).to(probs.dtype)


# ------------------------------------------------------------------------------------------------ kernel bindings
def _check_pairs(pairs_host: Sequence[Tuple[int, int]], D: int, mode: int) -> None:
    for d1, d2 in pairs_host:
        if not (0 <= d1 < D and 0 <= d2 < D) or (d1 == d2) != (mode == 1):
            _lib.check(_lib.E_BADARG, f"cond_grid: pair ({d1}, {d2}) with theta-dim {D} in mode {mode} (mode 2 takes "
                                      "two different dimensions, mode 1 one dimension twice)")


def pairs_tensor(pairs_host: Sequence[Tuple[int, int]], device) -> Tensor:
    return torch.tensor([list(p) for p in pairs_host], dtype=torch.int32, device=device).reshape(-1, 2)


def grid_fill(cond: Tensor, axes: Tensor, pairs_host: Sequence[Tuple[int, int]], pairs: Tensor, mode: int, g0: int,
              g1: int) -> Tensor:
    """theta rows ((g1 - g0) * cells, D) of grids g0 ... g1-1 (``sbi_amd_cond_grid_fill``).  `pairs_host` is the host
    copy of `pairs`: the pairs are validated on it, without reading device memory."""
    dev = _lib.require_device(cond, axes)
    C, D = cond.shape
    R, P = axes.shape[1], len(pairs_host)
    _check_pairs(pairs_host, D, mode)
    if not (0 <= g0 <= g1 <= C * P) or axes.shape[0] != D or pairs.shape != (P, 2) or pairs.dtype != torch.int32:
        _lib.check(_lib.E_BADARG, "cond_grid_fill")
    cells = R * R if mode == 2 else R
    out = torch.empty((g1 - g0) * cells, D, dtype=torch.float32, device=dev)
    if g1 == g0:
        return out                                   # (an empty tensor has no pointer to hand over)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_cond_grid_fill(_lib.ptr(cond), _lib.ptr(axes), pairs.data_ptr(), D, R, P, mode, g0, g1,
                                                _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, f"cond_grid_fill ({ENVELOPE})")
    return out


def grid_moments(logp: Tensor, axes: Tensor, pairs_host: Sequence[Tuple[int, int]], pairs: Tensor, g0: int = 0,
                 want_probs: bool = False, want_moments: bool = False):
    """(rho (G,), probs (G, R, R) or None, moments (G, 6) fp64 or None) of logp (G, R^2) on grids g0 ... g0+G-1
    (``sbi_amd_cond_grid_moments``)."""
    dev = _lib.require_device(logp, axes)
    D, R = axes.shape
    P = len(pairs_host)
    _check_pairs(pairs_host, D, 2)
    G = logp.shape[0]
    if logp.dim() != 2 or logp.shape[1] != R * R or pairs.shape != (P, 2) or pairs.dtype != torch.int32 or g0 < 0:
        _lib.check(_lib.E_BADARG, "cond_grid_moments")
    rho = torch.empty(G, dtype=torch.float32, device=dev)
    probs = torch.empty(G, R, R, dtype=torch.float32, device=dev) if want_probs else None
    moments = torch.empty(G, 6, dtype=torch.float64, device=dev) if want_moments else None
    if G == 0:
        return rho, probs, moments
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_cond_grid_moments(_lib.ptr(logp), _lib.ptr(axes), pairs.data_ptr(), D, R, P, g0, G,
                                                   _lib.ptr(rho), _lib.ptr(probs), _lib.ptr(moments),
                                                   _lib.current_stream(dev))
    _lib.check(rc, f"cond_grid_moments ({ENVELOPE})")
    return rho, probs, moments


def expand_condition(cond: Tensor, dims: Tensor, theta: Tensor) -> Tensor:
    """out (N, D): every row is `cond` (1, D) with the columns `dims` (k, int32, on the device) replaced by theta (N, k)
    (``sbi_amd_cond_expand``)."""
    dev = _lib.require_device(cond, theta)
    N, k = theta.shape
    D = cond.shape[-1]
    out = torch.empty(N, D, dtype=torch.float32, device=dev)
    if N == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_cond_expand(_lib.ptr(cond), dims.data_ptr(), _lib.ptr(theta), N, D, k, _lib.ptr(out),
                                             _lib.current_stream(dev))
    _lib.check(rc, "cond_expand (theta-dim <= 1024)")
    return out


def _fill_free_dims(condition: Tensor, dims_to_sample: List[int], theta: Tensor) -> Tensor:
    """The eager construction: `condition` (1, D) repeated to theta's batch, the free columns overwritten."""
    full = condition.to(theta.device).repeat(theta.shape[0], 1)
    full[:, dims_to_sample] = theta.to(full.dtype)
    return full


# ------------------------------------------------------------------------------------------------ mixtures
def extract_and_transform_mog(estimator: Any, context: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Extracts the Mixture of Gaussians (MoG) parameters from an MDN at the context `x`, transformed back to the
    original (un-z-scored) parameter space when the estimator z-scores theta.

    Adapted to this package's ``MixtureDensityEstimator``: the mixture comes from ``get_uncorrected_mog`` (the
    components kernel), the z-scoring from the net's ``zstats`` buffer (sbi's ``_transform_shift`` /
    ``_transform_scale``).  An estimator that publishes sbi's attributes is read through those instead.

    Returns:
        norm_logits: Normalised log weights of the underlying MoG. (batch_size, n_mixtures)
        means_transformed: Recentred and rescaled means. (batch_size, n_mixtures, n_dims)
        precfs_transformed: Rescaled precision factors. (batch_size, n_mixtures, n_dims, n_dims)
        sumlogdiag: Sum of the log of the diagonal of the precision factors. (batch_size, n_mixtures)
    """
    if context is None:
        raise ValueError("context must be provided for extract_and_transform_mog")
    mog = estimator.get_uncorrected_mog(context)
    norm_logits, means, precfs = mog.log_weights, mog.means, mog.precision_factors
    if getattr(estimator, "_prior_transform", None) is not None:
        raise NotImplementedError("Conditional density extraction is not supported for "
                                  "z_score='transform_to_unconstrained' (it assumes an affine z-score).")
    shift = scale = None
    net = getattr(estimator, "net", None)
    if getattr(net, "z_score_theta", False) and hasattr(net, "zstats"):
        D = means.shape[-1]
        shift, scale = net.zstats[:D].to(means), net.zstats[D : 2 * D].to(means)
    elif getattr(estimator, "has_input_transform", False):
        shift, scale = estimator._transform_shift.to(means), estimator._transform_scale.to(means)
    if shift is not None:
        # z = (theta - shift) / scale: the means move back affinely, and with precision = U^T U the factor of the
        # theta-space precision is U diag(1 / scale) -- its columns divided by the scales
        means = means * scale + shift
        precfs = precfs / scale
    sumlogdiag = torch.log(torch.diagonal(precfs, dim1=-2, dim2=-1)).sum(-1)
    return norm_logits, means, precfs, sumlogdiag


def condition_mog(condition: Tensor, dims: List[int], logits: Tensor, means: Tensor,
                  precfs: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Finds the conditional distribution p(X|Y) for a MoG (batch size 1, evaluated on the host in fp64).

    Args:
        condition: Parameter set (1, n_dims); the entries at `dims` are ignored.
        dims: Which dimensions remain free (X); the others (Y) are fixed to `condition`.
        logits: Log weights of the MoG. (1, n_mixtures)
        means: Means of the MoG. (1, n_mixtures, n_dims)
        precfs: Upper precision factors of the MoG (precision = U^T U). (1, n_mixtures, n_dims, n_dims)

    Returns:
        logits, means, precision factors and their summed log-diagonals of the conditioned MoG, in the dtype and on
        the device of `means`.
    """
    if means.shape[0] != 1 or torch.atleast_2d(condition).shape[0] != 1:
        raise ValueError("Condition with batch size > 1 not supported.")
    K, D = means.shape[1:]
    out_device, out_dtype = means.device, means.dtype
    free = torch.zeros(D, dtype=torch.bool)
    free[list(dims)] = True
    cond64 = torch.atleast_2d(condition).detach().to("cpu", torch.float64)
    lg = logits.detach().to("cpu", torch.float64)[0]
    mu = means.detach().to("cpu", torch.float64)[0]                         # (K, D)
    U = precfs.detach().to("cpu", torch.float64)[0]                         # (K, D, D)

    y = cond64[0, ~free]                                                    # (Dy,)
    mu_x, mu_y = mu[:, free], mu[:, ~free]
    U_xx = U[:, free][:, :, free]                                           # upper triangular: a factor of P_xx | rest
    U_yy = U[:, ~free][:, :, ~free]
    prec = U.transpose(-1, -2) @ U
    P_xx = U_xx.transpose(-1, -2) @ U_xx
    P_yy = U_yy.transpose(-1, -2) @ U_yy
    P_xy = prec[:, free][:, :, ~free]
    dy = (y - mu_y).unsqueeze(-1)                                           # (K, Dy, 1)
    # mean of x | y in precision form: mu_x - P_xx^-1 P_xy (y - mu_y)
    cond_means = mu_x - torch.linalg.solve(P_xx, P_xy @ dy).squeeze(-1)
    # weight of component k given y: its log weight plus log N(y; mu_y, P_yy^-1) in sbi's sub-factor form
    Dy = int((~free).sum())
    quad = (dy.transpose(-1, -2) @ P_yy @ dy).reshape(K)
    log_py = -0.5 * Dy * math.log(2 * math.pi) + torch.log(torch.diagonal(U_yy, dim1=-2, dim2=-1)).sum(-1) - 0.5 * quad
    cond_logits = torch.log_softmax(lg + log_py, dim=-1)
    sumlogdiag = torch.log(torch.diagonal(U_xx, dim1=-2, dim2=-1)).sum(-1)

    def back(t: Tensor) -> Tensor:
        return t.unsqueeze(0).to(out_device, out_dtype)

    return back(cond_logits), back(cond_means), back(U_xx.contiguous()), back(sumlogdiag)


# ------------------------------------------------------------------------------------------------ potentials
class ConditionedPotential:
    def __init__(self, potential_fn: Any, condition: Tensor, dims_to_sample: List[int]):
        r"""
        Return conditional posterior log-probability or $-\infty$ if outside prior.

        Args:
            potential_fn: Potential function to condition on.
            condition: Fixed parameters $\theta_j$, batch size 1.
            dims_to_sample: Which dimensions to sample from. The dimensions not specified in `dims_to_sample` will be
                fixed to values given in `condition`.
        """
        condition = torch.atleast_2d(torch.as_tensor(condition, dtype=torch.float32))
        if condition.shape[0] > 1:
            raise ValueError("Condition with batch size > 1 not supported.")
        self.potential_fn = potential_fn
        self.device = getattr(potential_fn, "device", str(condition.device))
        self.condition = condition.to(self.device).contiguous()
        self.dims_to_sample = list(dims_to_sample)
        self._x_is_iid: Optional[bool] = None
        self._dims_dev: Optional[Tensor] = None          # dims_to_sample on the device, for the expand kernel

    def _on_kernel(self, theta: Tensor, track_gradients: bool) -> bool:
        D, k = self.condition.shape[1], len(self.dims_to_sample)
        return (theta.is_cuda and self.condition.device == theta.device and theta.dtype == torch.float32
                and 1 <= k <= D <= EXPAND_MAX_DIM and theta.shape[1] == k
                and len(set(self.dims_to_sample)) == k and all(0 <= d < D for d in self.dims_to_sample)
                and not (track_gradients and theta.requires_grad))

    def __call__(self, theta: Tensor, track_gradients: bool = True) -> Tensor:
        r"""
        Returns the conditional potential $\log(p(\theta_i|\theta_j, x))$ of the free parameters `theta`
        (batch, len(dims_to_sample)), masked outside of the prior.  On a ROCm device the full parameter rows are built
        by one launch (``sbi_amd_cond_expand``).
        """
        theta_ = ensure_theta_batched(torch.as_tensor(theta, dtype=torch.float32))
        if theta_.device != self.condition.device:
            theta_ = theta_.to(self.condition.device)
        if self._on_kernel(theta_, track_gradients):
            if self._dims_dev is None or self._dims_dev.device != theta_.device:
                self._dims_dev = torch.tensor(self.dims_to_sample, dtype=torch.int32, device=theta_.device)
            full = expand_condition(self.condition, self._dims_dev, theta_.detach().contiguous())
        else:
            full = _fill_free_dims(self.condition, self.dims_to_sample, theta_)
        return self.potential_fn(full, track_gradients=track_gradients)

    @property
    def x_is_iid(self) -> bool:
        """If x has batch dimension greater than 1, whether to intepret the batch as iid samples or batch of data
        points."""
        if self._x_is_iid is not None:
            return self._x_is_iid
        raise ValueError("No observed data is available. Use `potential_fn.set_x(x_o)`.")

    def set_x(self, x_o: Optional[Tensor], x_is_iid: Optional[bool] = True):
        """Check the shape of the observed data and, if valid, set it."""
        if x_o is not None:
            x_o = process_x(x_o).to(self.device)
        self._x_is_iid = x_is_iid
        self.potential_fn.set_x(x_o, x_is_iid=x_is_iid)

    @property
    def x_o(self) -> Tensor:
        """Return the observed data at which the potential is evaluated."""
        if self.potential_fn._x_o is not None:
            return self.potential_fn._x_o
        raise ValueError("No observed data is available.")

    @x_o.setter
    def x_o(self, x_o: Optional[Tensor]) -> None:
        self.set_x(x_o)

    def return_x_o(self) -> Optional[Tensor]:
        """The observed data, or None (unlike the `x_o` property this never raises)."""
        return self.potential_fn._x_o


class RestrictedPriorForConditional:
    """
    Class to restrict a prior to fewer dimensions as needed for conditional sampling.

    `sample` draws the full parameter vector and keeps the free dimensions (what the MCMC init strategies feed to the
    conditioned potential); `log_prob` is the full prior's, because a theta is scored under the full joint once the
    condition has been filled in.
    """

    def __init__(self, full_prior: Any, dims_to_sample: List[int]):
        self.full_prior = full_prior
        self.dims_to_sample = list(dims_to_sample)

    def sample(self, *args, **kwargs):
        return self.full_prior.sample(*args, **kwargs)[:, self.dims_to_sample]

    def log_prob(self, *args, **kwargs):
        return self.full_prior.log_prob(*args, **kwargs)


class RestrictedTransformForConditional(torch_tf.Transform):
    """
    Class to restrict the transform to fewer dimensions for conditional sampling.

    Every method fills the free dimensions of `condition` with `theta`, applies the full transform and keeps the free
    dimensions.  `log_abs_det_jacobian` is taken over ALL dimensions: the share of the fixed ones is a constant, which
    drops out during MCMC.
    """

    domain = constraints.real_vector
    codomain = constraints.real_vector
    bijective = True

    def __init__(self, transform: torch_tf.Transform, condition: Tensor, dims_to_sample: List[int]) -> None:
        super().__init__()
        self.transform = transform
        self.condition = ensure_theta_batched(torch.as_tensor(condition, dtype=torch.float32))
        if self.condition.shape[0] > 1:
            raise ValueError("Condition with batch size > 1 not supported.")
        self.dims_to_sample = list(dims_to_sample)

    def __eq__(self, other):
        return (isinstance(other, RestrictedTransformForConditional) and self.transform == other.transform
                and self.dims_to_sample == other.dims_to_sample and torch.equal(self.condition, other.condition))

    def _full(self, theta: Tensor) -> Tensor:
        return _fill_free_dims(self.condition, self.dims_to_sample, ensure_theta_batched(theta))

    def _call(self, theta: Tensor) -> Tensor:
        return self.transform(self._full(theta))[:, self.dims_to_sample]

    def _inverse(self, theta: Tensor) -> Tensor:
        return self.transform.inv(self._full(theta))[:, self.dims_to_sample]

    def log_abs_det_jacobian(self, theta1: Tensor, theta2: Tensor) -> Tensor:
        return self.transform.log_abs_det_jacobian(self._full(theta1), self._full(theta2))
