"""Score estimators (NPSE) running on the HIP kernels of csrc/npse.hip.

Host-side mirror of sbi's score estimators (same class and method names, argument meaning and shapes):
  ConditionalScoreEstimator, VPScoreEstimator, SubVPScoreEstimator, VEScoreEstimator
                             sbi/neural_nets/estimators/score_estimator.py:18-1098
  VectorFieldMLP             sbi/neural_nets/net_builders/vector_field_nets.py:610-719 (the FMPE network:
                             ``VectorFieldMLPParams`` of flowmatching_estimator.py, same flat layout and key names)

The network, its packed image and the trunk GEMMs are those of the flow-matching path; the SDE-dependent input scaling,
the score pre-conditioning, the denoising-score-matching loss with its control variate and the Euler-Maruyama sampler
are kernel modes around it (include/sbi_amd_npse.h).  The schedules (``train_schedule`` / ``solve_schedule``) and the
scalar SDE functions are host / torch code: times reach the kernels as arrays.

Supported: ``net="mlp"``, flat theta and flat x, the three named weight functions.  Anything else raises; there is no
PyTorch fallback for the network.
"""

from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional, Union

import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.base import ConditionalEstimator
from sbi_amd.neural_nets.estimators.flowmatching_estimator import FMPEHyper, VectorFieldMLPParams, packed_weights

_SDE_CODE = {"ve": 0, "vp": 1, "subvp": 2}
_WEIGHT_CODE = {"identity": 0, "max_likelihood": 1, "variance": 2}


# --------------------------------------------------------------------- kernel calls
def _cfg(est: "ConditionalScoreEstimator", cv_threshold: float = 0.0) -> _lib.NPSEConfigC:
    return _lib.NPSEConfigC(est.net.hyper.c_config(), _SDE_CODE[est.sde_type], _WEIGHT_CODE[est.weight_fn_name],
                            float(getattr(est, "beta_min", 0.0)), float(getattr(est, "beta_max", 0.0)),
                            float(getattr(est, "sigma_min", 0.0)), float(getattr(est, "sigma_max", 0.0)),
                            float(cv_threshold), float(est.t_min), float(est.t_max))


def score_call(est: "ConditionalScoreEstimator", theta_t: Tensor, x: Tensor, times: Tensor, ode: bool = False,
               out: Optional[Tensor] = None) -> Tensor:
    """theta_t (n, D), x (n, C) or (1, C), times (n,) or (1,) -> score (n, D), or ``ode_fn`` with ``ode=True``."""
    net = est.net
    dev = _lib.require_device(theta_t, x, times, net.flat_params)
    n = theta_t.shape[0]
    out = torch.empty_like(theta_t) if out is None else out
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_score(
            _cfg(est), _lib.ptr(packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(theta_t), _lib.ptr(x), x.shape[0],
            _lib.ptr(times), times.numel(), n, int(ode), _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "npse_score")
    return out


def dsm_loss(est: "ConditionalScoreEstimator", theta: Tensor, x: Tensor, times: Tensor, eps: Tensor,
             cv_threshold: float) -> Tensor:
    net = est.net
    dev = _lib.require_device(theta, x, times, eps, net.flat_params)
    n = theta.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_loss(
            _cfg(est, cv_threshold), _lib.ptr(packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(theta), _lib.ptr(x),
            x.shape[0], _lib.ptr(times), _lib.ptr(eps), n, _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "npse_loss")
    return out


def train_workspace(est: "ConditionalScoreEstimator", n: int, device, cv_threshold: float,
                    workspace: Optional[Tensor] = None) -> Tensor:
    need = _lib.load().sbi_amd_npse_train_workspace_floats(_cfg(est, cv_threshold), n)
    if need < 0:
        _lib.check(int(need), "npse_train_workspace_floats")
    if workspace is not None and workspace.numel() >= need and workspace.device == torch.device(device):
        return workspace
    return torch.empty(int(need), dtype=torch.float32, device=device)


def loss_fwd_bwd(est: "ConditionalScoreEstimator", theta: Tensor, x: Tensor, times: Tensor, eps: Tensor,
                 row_weight: Optional[Tensor], uniform_weight: float, grad_out: Tensor, cv_threshold: float,
                 workspace: Optional[Tensor] = None) -> Tensor:
    """Per-row score-matching losses; ``grad_out`` <- d/dparams sum_i w_i loss_i."""
    net = est.net
    dev = _lib.require_device(theta, x, times, eps, net.flat_params, grad_out, row_weight)
    n = theta.shape[0]
    ws = train_workspace(est, n, dev, cv_threshold, workspace)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_loss_fwd_bwd(
            _cfg(est, cv_threshold), _lib.ptr(net.flat_params), _lib.ptr(packed_weights(net)), _lib.ptr(net.zstats),
            _lib.ptr(theta), _lib.ptr(x), x.shape[0], _lib.ptr(times), _lib.ptr(eps), n, _lib.ptr(row_weight),
            float(uniform_weight), _lib.ptr(out), _lib.ptr(grad_out), _lib.ptr(ws), _lib.current_stream(dev))
    _lib.check(rc, "npse_loss_fwd_bwd")
    return out


def sample_sde_fused(est: "ConditionalScoreEstimator", n: int, x: Tensor, ts: Tensor, eta: float = 1.0,
                     noise: Optional[Tensor] = None, seed: int = 0, row_offset: int = 0) -> Tensor:
    """``Diffuser.run`` with the Euler-Maruyama predictor in one launch: x (1, C) or (n, C), ts (steps + 1,) decreasing;
    ``noise`` (steps + 1, n, D) makes the result a pure function of the arguments, otherwise the kernel draws from
    Philox keyed by ``seed`` (a row's draws depend on (seed, row + row_offset, step, dim) only)."""
    net = est.net
    base = torch.cat([est.mean_base.reshape(-1), est.std_base.reshape(-1)]).to(torch.float32).contiguous()
    dev = _lib.require_device(x, ts, net.flat_params, base, noise)
    D = est.input_shape[0]
    steps = ts.numel() - 1
    if noise is not None and tuple(noise.shape) != (steps + 1, n, D):
        raise ValueError(f"noise must have shape {(steps + 1, n, D)}, got {tuple(noise.shape)}")
    out = torch.empty(n, D, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_sample_sde(
            _cfg(est), _lib.ptr(packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(base), _lib.ptr(x), x.shape[0],
            _lib.ptr(ts), steps, float(eta), _lib.ptr(noise), int(seed) & (2**64 - 1), int(row_offset), n,
            _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "npse_sample_sde")
    return out


@torch.no_grad()
def sample_sde_loop(est: "ConditionalScoreEstimator", n: int, x: Tensor, ts: Tensor, eta: float = 1.0,
                    noise: Optional[Tensor] = None) -> Tensor:
    """The plain path (diffuser.py:124-172, predictors.py:112-120): one score launch per step from a host loop.
    The baseline the fused sampler is measured against, and the route for time grids the fused kernel refuses."""
    D = est.input_shape[0]
    dev = x.device

    def draw(k):
        return noise[k] if noise is not None else torch.randn(n, D, device=dev)

    theta = (est.mean_base + est.std_base * draw(0)).contiguous()
    for k in range(1, ts.numel()):
        t1, t0 = ts[k - 1], ts[k]
        dt = t1 - t0
        g = est.diffusion_fn(theta, t1.reshape(1))
        f = est.drift_fn(theta, t1.reshape(1))
        sc = score_call(est, theta, x, t1.reshape(1).contiguous())
        theta = (theta - (f - (1 + eta**2) / 2 * g**2 * sc) * dt + eta * g * draw(k) * torch.sqrt(dt)).contiguous()
    return theta


# --------------------------------------------------------------------- iid observations (include/sbi_amd_npse_iid.h)
IID_FUSED_MAX_D, IID_FUSED_MAX_N = 16, 1024
# which leg `sample_sde_iid` / `score_iid` take inside the fused envelope: the fused sampler measured slower than the
# host loop at both benchmark shapes (profiles/npse_iid_bench.json; README, "NPSE with iid observations")
IID_DEFAULT_FUSED = False


def iid_fused_supported(est: "ConditionalScoreEstimator", N: int, steps: int = 0) -> bool:
    """The envelope of the fused kernels: D <= 16 (one MFMA tile per table), N <= 1024, steps <= 65535."""
    return est.input_shape[0] <= IID_FUSED_MAX_D and 1 <= N <= IID_FUSED_MAX_N and steps <= 65535


def _iid_workspace(est, N: int, dev) -> Tensor:
    need = _lib.load().sbi_amd_npse_iid_workspace_floats(_cfg(est), N)
    if need < 0:
        _lib.check(int(need), "npse_iid_workspace_floats")
    return torch.empty(int(need), dtype=torch.float32, device=dev)


def compose_iid(s: Tensor, theta: Tensor, lam: Optional[Tensor], mats: Tensor, vec: Tensor) -> Tensor:
    """Linv (C sum_i s_i + sum_i Lam_i s_i) + A theta + b: s (n, N, D), theta (n, D), lam (N, D, D) or None,
    mats (3, D, D), vec (D,).  One block per row with sequential sums (``sbi_amd_npse_compose_iid``), not BLAS
    products: rocBLAS picks its kernel by the batch shape, which would make a row's low bits depend on how the rows are
    split into calls."""
    s, theta, mats, vec = s.contiguous(), theta.contiguous(), mats.contiguous(), vec.contiguous()
    lam = None if lam is None else lam.contiguous()
    dev = _lib.require_device(s, theta, lam, mats, vec)
    n, N, D = s.shape
    out = torch.empty_like(theta)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_compose_iid(_lib.ptr(s), _lib.ptr(theta), _lib.ptr(lam), _lib.ptr(mats),
                                                  _lib.ptr(vec), n, N, D, _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "npse_compose_iid")
    return out


def score_iid_fused(est: "ConditionalScoreEstimator", theta_t: Tensor, xs: Tensor, time: Tensor, lam: Optional[Tensor],
                    mats: Tensor, vec: Tensor) -> Tensor:
    """Composed score of the N observations xs (N, C) at theta_t (n, D) and one time, in one launch."""
    net = est.net
    dev = _lib.require_device(theta_t, xs, time, net.flat_params, lam, mats, vec)
    n, N = theta_t.shape[0], xs.shape[0]
    out = torch.empty_like(theta_t)
    if n == 0:
        return out
    ws = _iid_workspace(est, N, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_score_iid(
            _cfg(est), _lib.ptr(packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(theta_t), _lib.ptr(xs), N,
            _lib.ptr(time), _lib.ptr(lam), _lib.ptr(mats), _lib.ptr(vec), n, _lib.ptr(ws), _lib.ptr(out),
            _lib.current_stream(dev))
    _lib.check(rc, "npse_score_iid")
    return out


@torch.no_grad()
def score_iid_loop(est: "ConditionalScoreEstimator", theta_t: Tensor, xs: Tensor, time: Tensor, lam: Optional[Tensor],
                   mats: Tensor, vec: Tensor) -> Tensor:
    """The same score from one `sbi_amd_npse_score` launch on the n N expanded rows and the per-row composition kernel."""
    n, N, D = theta_t.shape[0], xs.shape[0], theta_t.shape[1]
    s = score_call(est, theta_t.repeat_interleave(N, dim=0).contiguous(), xs.repeat(n, 1).contiguous(),
                   time.reshape(1).contiguous())
    return compose_iid(s.reshape(n, N, D), theta_t, lam, mats, vec)


def score_iid(est, theta_t, xs, time, lam, mats, vec) -> Tensor:
    if IID_DEFAULT_FUSED and iid_fused_supported(est, xs.shape[0]):
        return score_iid_fused(est, theta_t, xs, time, lam, mats, vec)
    return score_iid_loop(est, theta_t, xs, time, lam, mats, vec)


def _iid_base(est, base_scale: float) -> Tensor:
    return torch.cat([est.mean_base.reshape(-1), est.std_base.reshape(-1) * base_scale]).to(torch.float32).contiguous()


def sample_sde_iid_fused(est: "ConditionalScoreEstimator", n: int, xs: Tensor, ts: Tensor, lam: Optional[Tensor],
                         step_mats: Tensor, step_vecs: Tensor, eta: float = 1.0, noise: Optional[Tensor] = None,
                         seed: int = 0, row_offset: int = 0, base_scale: float = 1.0) -> Tensor:
    """`sample_sde_fused` with the score of step k replaced by the composed score of the N observations xs (N, C):
    step_mats (steps, 3, D, D) and step_vecs (steps, D) are the tables at ts[:-1].  Same Philox keying and `noise`
    contract; ``base_scale`` multiplies std_base of the initial draw (fnpe: 1 / sqrt(N))."""
    net = est.net
    base = _iid_base(est, base_scale)
    dev = _lib.require_device(xs, ts, net.flat_params, base, noise, lam, step_mats, step_vecs)
    D, N = est.input_shape[0], xs.shape[0]
    steps = ts.numel() - 1
    if noise is not None and tuple(noise.shape) != (steps + 1, n, D):
        raise ValueError(f"noise must have shape {(steps + 1, n, D)}, got {tuple(noise.shape)}")
    if tuple(step_mats.shape) != (steps, 3, D, D) or tuple(step_vecs.shape) != (steps, D):
        raise ValueError(f"tables must have shapes {(steps, 3, D, D)} and {(steps, D)}")
    out = torch.empty(n, D, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    ws = _iid_workspace(est, N, dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_npse_sample_sde_iid(
            _cfg(est), _lib.ptr(packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(base), _lib.ptr(xs), N,
            _lib.ptr(ts), steps, float(eta), _lib.ptr(lam), _lib.ptr(step_mats), _lib.ptr(step_vecs), _lib.ptr(noise),
            int(seed) & (2**64 - 1), int(row_offset), n, _lib.ptr(ws), _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "npse_sample_sde_iid")
    return out


def sde_normals(n: int, D: int, k: int, seed: int, row_offset: int, device) -> Tensor:
    """(n, D) standard-normal draws z_k of the SDE samplers for rows row_offset .. row_offset + n - 1 under ``seed``."""
    out = torch.empty(n, D, dtype=torch.float32, device=device)
    if n:
        with torch.cuda.device(device):
            rc = _lib.load().sbi_amd_npse_sde_normals(int(seed) & (2**64 - 1), int(row_offset), int(k), n, D,
                                                      _lib.ptr(out), _lib.current_stream(out.device))
        _lib.check(rc, "npse_sde_normals")
    return out


@torch.no_grad()
def sample_sde_iid_loop(est: "ConditionalScoreEstimator", n: int, xs: Tensor, ts: Tensor, lam: Optional[Tensor],
                        step_mats: Tensor, step_vecs: Tensor, eta: float = 1.0, noise: Optional[Tensor] = None,
                        base_scale: float = 1.0, seed: Optional[int] = None, row_offset: int = 0) -> Tensor:
    """The plain path: per step one score launch on the n N expanded rows, then composition and update in torch.  The
    route outside the fused envelope and the baseline the fused sampler is measured against.  Draws: ``noise``, else
    with a ``seed`` the fused sampler's own Philox draws (same keying, so the result does not depend on how rows are
    split into calls -- bit for bit, since score, composition and update are all row-wise), else torch's generator."""
    D, N = est.input_shape[0], xs.shape[0]
    dev = xs.device

    def draw(k):
        if noise is not None:
            return noise[k]
        if seed is not None:
            return sde_normals(n, D, k, seed, row_offset, dev)
        return torch.randn(n, D, device=dev)

    theta = (est.mean_base + est.std_base * base_scale * draw(0)).contiguous()
    xe = xs.repeat(n, 1).contiguous()
    for k in range(1, ts.numel()):
        t1, t0 = ts[k - 1], ts[k]
        dt = t1 - t0
        g = est.diffusion_fn(theta, t1.reshape(1))
        f = est.drift_fn(theta, t1.reshape(1))
        s = score_call(est, theta.repeat_interleave(N, dim=0).contiguous(), xe, t1.reshape(1).contiguous())
        sc = compose_iid(s.reshape(n, N, D), theta, lam, step_mats[k - 1], step_vecs[k - 1])
        theta = (theta - (f - (1 + eta**2) / 2 * g**2 * sc) * dt + eta * g * draw(k) * torch.sqrt(dt)).contiguous()
    return theta


def sample_sde_iid(est, n, xs, ts, lam, step_mats, step_vecs, eta=1.0, seed=0, row_offset=0, base_scale=1.0,
                   noise=None) -> Tensor:
    """The default leg: the host loop unless ``IID_DEFAULT_FUSED`` selects the fused sampler inside its envelope.  Both
    draw ``noise`` if given, else Philox keyed by (seed, row + row_offset, step, dim)."""
    if IID_DEFAULT_FUSED and iid_fused_supported(est, xs.shape[0], ts.numel() - 1):
        return sample_sde_iid_fused(est, n, xs, ts, lam, step_mats, step_vecs, eta, noise, seed, row_offset, base_scale)
    return sample_sde_iid_loop(est, n, xs, ts, lam, step_mats, step_vecs, eta, noise, base_scale, seed, row_offset)


class _DSMLossFn(torch.autograd.Function):
    """Autograd bridge: per-row loss whose backward hands sum_i g_i dloss_i/dparams to ``flat_params.grad``
    (the fused kernels run again with the incoming g as row weights)."""

    @staticmethod
    def forward(ctx, flat_params, est, theta, x, times, eps, cv_threshold):
        ctx.est, ctx.args = est, (theta, x, times, eps, cv_threshold)
        return dsm_loss(est, theta, x, times, eps, cv_threshold)

    @staticmethod
    def backward(ctx, g):
        theta, x, times, eps, cv_threshold = ctx.args
        grad = torch.empty_like(ctx.est.net.flat_params.data)
        loss_fwd_bwd(ctx.est, theta, x, times, eps, g.contiguous().float(), 0.0, grad, cv_threshold)
        return grad, None, None, None, None, None, None


# --------------------------------------------------------------------- estimators
class ConditionalScoreEstimator(ConditionalEstimator):
    """p(theta_t | theta_0) = N(mean_t(t) theta_0, std(t)^2); the network predicts the pre-conditioned score
    (score_estimator.py:18-528).  t_min is data, t_max is (almost) the Gaussian base distribution."""

    SCORE_DEFINED = True
    SDE_DEFINED = True
    MARGINALS_DEFINED = True
    sde_type = ""

    def __init__(self, net: VectorFieldMLPParams, input_shape: torch.Size, condition_shape: torch.Size,
                 weight_fn: Union[str, object] = "max_likelihood", beta_min: float = 0.01, beta_max: float = 10.0,
                 t_min: float = 1e-3, t_max: float = 1.0):
        super().__init__(input_shape, condition_shape)
        if len(input_shape) != 1 or len(condition_shape) != 1:
            raise NotImplementedError("sbi_amd NPSE: theta and x must be flat vectors (1-D event shapes)")
        if not isinstance(net, VectorFieldMLPParams):
            raise NotImplementedError("sbi_amd NPSE runs the default vector-field MLP (VectorFieldMLPParams) only; "
                                      "custom score networks are outside the HIP path")
        self.net = net
        self.t_min, self.t_max = float(t_min), float(t_max)
        self.beta_min, self.beta_max = float(beta_min), float(beta_max)
        self._set_weight_fn(weight_fn)
        with torch.no_grad():
            t = torch.tensor([self.t_max])
            mean_0, std_0 = self.mean_0.detach().cpu(), self.std_0.detach().cpu()
            m = self.mean_t_fn(t)
            mean_base = (m * mean_0).reshape(1, -1)
            std_base = torch.sqrt(m**2 * std_0**2 + self.std_fn(t) ** 2).reshape(1, -1)
        self.register_buffer("_mean_base", mean_base.expand(1, *input_shape).clone().float())
        self.register_buffer("_std_base", std_base.expand(1, *input_shape).clone().float())

    # ------------------------------------------------------------------ bookkeeping
    @property
    def embedding_net(self) -> Optional[nn.Module]:
        return None

    @property
    def mean_0(self) -> Tensor:
        return self.net.zstats[: self.net.hyper.D]

    @property
    def std_0(self) -> Tensor:
        return self.net.zstats[self.net.hyper.D : 2 * self.net.hyper.D]

    @property
    def mean_base(self) -> Tensor:
        return self._mean_base

    @property
    def std_base(self) -> Tensor:
        return self._std_base

    def _set_weight_fn(self, weight_fn) -> None:
        """score_estimator.py:478-509; a callable weight would have to run inside the loss kernel."""
        if callable(weight_fn):
            raise NotImplementedError("sbi_amd NPSE: a callable weight_fn is outside the HIP path; use 'identity', "
                                      "'max_likelihood' or 'variance'")
        if weight_fn not in _WEIGHT_CODE:
            raise ValueError(f"Weight function {weight_fn} not recognized.")
        self.weight_fn_name = weight_fn

    def weight_fn(self, times: Tensor) -> Tensor:
        if self.weight_fn_name == "identity":
            return torch.ones_like(times)
        if self.weight_fn_name == "max_likelihood":
            return self.diffusion_fn(torch.ones((1,), device=times.device), times) ** 2
        return self.std_fn(times) ** 2

    def reference_state_dict(self) -> "OrderedDict[str, Tensor]":
        """Keys of sbi's score-estimator ``state_dict()`` (the ones this path owns)."""
        sd = self.net.reference_state_dict()
        sd["_mean_base"] = self._mean_base.detach().clone()
        sd["_std_base"] = self._std_base.detach().clone()
        return sd

    @torch.no_grad()
    def load_reference_state_dict(self, sd: Dict[str, Tensor]) -> None:
        self.net.load_reference_state_dict(sd)
        for key, buf in (("_mean_base", self._mean_base), ("_std_base", self._std_base)):
            if key in sd:
                buf.copy_(sd[key].reshape(1, -1).expand_as(buf))

    # ------------------------------------------------------------------ SDE (overridden per family)
    def _col(self, v: Tensor) -> Tensor:
        return v.unsqueeze(-1)       # one flat event dimension

    def mean_t_fn(self, times: Tensor) -> Tensor:
        raise NotImplementedError

    def std_fn(self, times: Tensor) -> Tensor:
        raise NotImplementedError

    def drift_fn(self, input: Tensor, times: Tensor) -> Tensor:
        raise NotImplementedError

    def diffusion_fn(self, input: Tensor, times: Tensor) -> Tensor:
        raise NotImplementedError

    def mean_fn(self, x0: Tensor, times: Tensor) -> Tensor:
        return self.mean_t_fn(times) * x0

    def noise_schedule(self, times: Tensor) -> Tensor:
        """Linear beta schedule of the vp / subvp families (score_estimator.py:411-425)."""
        return self.beta_min + (self.beta_max - self.beta_min) * times

    def approx_marginal_mean(self, times: Tensor) -> Tensor:
        return self.mean_t_fn(times) * self.mean_0

    def approx_marginal_std(self, times: Tensor) -> Tensor:
        return torch.sqrt(self.mean_t_fn(times) ** 2 * self.std_0**2 + self.std_fn(times) ** 2)

    def train_schedule(self, num_samples: int, t_min: Optional[float] = None, t_max: Optional[float] = None) -> Tensor:
        t_min = self.t_min if t_min is None else t_min
        t_max = self.t_max if t_max is None else t_max
        return torch.rand(num_samples, device=self._mean_base.device) * (t_max - t_min) + t_min

    def solve_schedule(self, num_steps: int, t_min: Optional[float] = None, t_max: Optional[float] = None) -> Tensor:
        t_min = self.t_min if t_min is None else t_min
        t_max = self.t_max if t_max is None else t_max
        return torch.linspace(t_max, t_min, num_steps, device=self._mean_base.device)

    # ------------------------------------------------------------------ forward / loss
    def _flat_args(self, input: Tensor, condition: Tensor, time: Tensor):
        self._check_input_shape(input)
        self._check_condition_shape(condition)
        bshape = torch.broadcast_shapes(input.shape[:-1], condition.shape[:-1])
        D, C = self.input_shape[0], self.condition_shape[0]
        th = input.to(torch.float32).expand(*bshape, D).reshape(-1, D).contiguous()
        cond = condition.to(torch.float32)
        c2 = cond.reshape(1, C).contiguous() if cond.numel() == C else cond.expand(*bshape, C).reshape(-1, C).contiguous()
        t = torch.as_tensor(time, dtype=torch.float32, device=th.device)
        t2 = t.reshape(1).contiguous() if t.numel() == 1 else t.expand(bshape).reshape(-1).contiguous()
        return th, c2, t2, bshape, D

    def forward(self, input: Tensor, condition: Tensor, time: Tensor) -> Tensor:
        """Score at ``(input, time)``; input ``(*batch, D)``, condition ``(*batch_c, C)``, time broadcastable to the
        batch shape (score_estimator.py:149-215)."""
        th, c2, t2, bshape, D = self._flat_args(input, condition, time)
        return score_call(self, th, c2, t2).reshape(*bshape, D)

    def score(self, input: Tensor, condition: Tensor, t: Tensor) -> Tensor:
        return self(input, condition, t)

    def ode_fn(self, input: Tensor, condition: Tensor, times: Tensor) -> Tensor:
        """f - g^2 score / 2 (score_estimator.py:511-528), from the same launch as the score."""
        th, c2, t2, bshape, D = self._flat_args(input, condition, times)
        return score_call(self, th, c2, t2, ode=True).reshape(*bshape, D)

    def loss(self, input: Tensor, condition: Tensor, times: Optional[Tensor] = None, control_variate: bool = True,
             control_variate_threshold: float = 0.3, eps: Optional[Tensor] = None, **kwargs) -> Tensor:
        """Per-row denoising-score-matching loss (score_estimator.py:230-316).  ``times`` come from
        ``train_schedule`` and ``eps`` ~ N(0, I) is drawn here when not given (in sbi's order: times, then eps).
        Differentiable with respect to the parameters through the fused backward kernels."""
        self._check_input_shape(input)
        self._check_condition_shape(condition)
        if input.dim() != 2 or condition.dim() != 2 or input.shape[0] != condition.shape[0]:
            raise ValueError("sbi_amd NPSE loss expects input (B, D) and condition (B, C)")
        theta = input.to(torch.float32).contiguous()
        x = condition.to(torch.float32).contiguous()
        if times is None:
            times = self.train_schedule(theta.shape[0]).to(theta.device)
        if eps is None:
            eps = torch.randn_like(theta)
        times = times.to(device=theta.device, dtype=torch.float32).reshape(-1).contiguous()
        eps = eps.to(torch.float32).contiguous()
        thr = float(control_variate_threshold) if control_variate else 0.0
        if torch.is_grad_enabled() and self.net.flat_params.requires_grad:
            return _DSMLossFn.apply(self.net.flat_params, self, theta, x, times, eps, thr)
        return dsm_loss(self, theta, x, times, eps, thr)


class _BetaSDE(ConditionalScoreEstimator):
    def mean_t_fn(self, times: Tensor) -> Tensor:
        return self._col(torch.exp(-0.25 * times**2.0 * (self.beta_max - self.beta_min) - 0.5 * times * self.beta_min))

    def _one_minus_m2(self, times: Tensor) -> Tensor:
        return 1.0 - torch.exp(-0.5 * times**2.0 * (self.beta_max - self.beta_min) - times * self.beta_min)

    def drift_fn(self, input: Tensor, times: Tensor) -> Tensor:
        phi = -0.5 * self.noise_schedule(times)
        while phi.dim() < input.dim():
            phi = phi.unsqueeze(-1)
        return phi * input


class VPScoreEstimator(_BetaSDE):
    """Variance-preserving SDE (DDPM), score_estimator.py:531-641."""

    sde_type = "vp"

    def std_fn(self, times: Tensor) -> Tensor:
        return torch.sqrt(self._col(self._one_minus_m2(times)))

    def diffusion_fn(self, input: Tensor, times: Tensor) -> Tensor:
        g = torch.sqrt(self.noise_schedule(times))
        while g.dim() < input.dim():
            g = g.unsqueeze(-1)
        return g


class SubVPScoreEstimator(_BetaSDE):
    """Sub-variance-preserving SDE, score_estimator.py:644-769 (its default t_min is 1e-2)."""

    sde_type = "subvp"

    def __init__(self, net, input_shape, condition_shape, weight_fn="max_likelihood", beta_min: float = 0.01,
                 beta_max: float = 10.0, t_min: float = 1e-2, t_max: float = 1.0):
        super().__init__(net, input_shape, condition_shape, weight_fn=weight_fn, beta_min=beta_min, beta_max=beta_max,
                         t_min=t_min, t_max=t_max)

    def std_fn(self, times: Tensor) -> Tensor:
        return self._col(self._one_minus_m2(times))

    def diffusion_fn(self, input: Tensor, times: Tensor) -> Tensor:
        g = torch.sqrt(torch.abs(self.noise_schedule(times) * (
            1 - torch.exp(-2 * self.beta_min * times - (self.beta_max - self.beta_min) * times**2))))
        while g.dim() < input.dim():
            g = g.unsqueeze(-1)
        return g


class VEScoreEstimator(ConditionalScoreEstimator):
    """Variance-exploding SDE (NCSN / SMLD), score_estimator.py:772-1098, with its lognormal training schedule and
    power-law solve schedule (Karras et al. 2022)."""

    sde_type = "ve"

    def __init__(self, net, input_shape, condition_shape, weight_fn="max_likelihood", sigma_min: float = 1e-4,
                 sigma_max: float = 10.0, t_min: float = 1e-3, t_max: float = 1.0, train_schedule: str = "uniform",
                 solve_schedule: str = "uniform", lognormal_mean: float = -1.2, lognormal_std: float = 1.2,
                 power_law_exponent: float = 7.0):
        if sigma_min <= 0:
            raise ValueError(f"sigma_min must be positive, got {sigma_min}")
        if sigma_max <= sigma_min:
            raise ValueError(f"sigma_max ({sigma_max}) must be greater than sigma_min ({sigma_min})")
        if train_schedule not in ("uniform", "lognormal"):
            raise ValueError(f"train_schedule must be one of ('uniform', 'lognormal'), got '{train_schedule}'")
        if solve_schedule not in ("uniform", "power_law"):
            raise ValueError(f"solve_schedule must be one of ('uniform', 'power_law'), got '{solve_schedule}'")
        if train_schedule == "lognormal" and lognormal_std <= 0:
            raise ValueError(f"lognormal_std must be positive, got {lognormal_std}")
        if solve_schedule == "power_law" and power_law_exponent <= 0:
            raise ValueError(f"power_law_exponent must be positive, got {power_law_exponent}")
        self.sigma_min, self.sigma_max = float(sigma_min), float(sigma_max)
        self._train_schedule_type, self._solve_schedule_type = train_schedule, solve_schedule
        self.lognormal_mean, self.lognormal_std = lognormal_mean, lognormal_std
        self.power_law_exponent = power_law_exponent
        super().__init__(net, input_shape, condition_shape, weight_fn=weight_fn, t_min=t_min, t_max=t_max)

    def mean_t_fn(self, times: Tensor) -> Tensor:
        return self._col(torch.ones_like(times))

    def std_fn(self, times: Tensor) -> Tensor:
        return self._col(self.noise_schedule(times))

    def noise_schedule(self, times: Tensor) -> Tensor:
        return self.sigma_min * (self.sigma_max / self.sigma_min) ** times

    def drift_fn(self, input: Tensor, times: Tensor) -> Tensor:
        return torch.tensor([0.0], device=input.device)

    def diffusion_fn(self, input: Tensor, times: Tensor) -> Tensor:
        g = self.noise_schedule(times) * math.sqrt(2 * math.log(self.sigma_max / self.sigma_min))
        while g.dim() < input.dim():
            g = g.unsqueeze(-1)
        return g.to(input.device)

    def train_schedule(self, num_samples: int, t_min: Optional[float] = None, t_max: Optional[float] = None) -> Tensor:
        t_min = self.t_min if t_min is None else t_min
        t_max = self.t_max if t_max is None else t_max
        if t_min >= t_max:
            raise ValueError(f"t_min ({t_min}) must be less than t_max ({t_max}).")
        dev = self._mean_base.device
        if self._train_schedule_type == "uniform":
            return torch.rand(num_samples, device=dev) * (t_max - t_min) + t_min
        log_sigma = self.lognormal_mean + self.lognormal_std * torch.randn(num_samples, device=dev)
        lo, hi = math.log(self.sigma_min), math.log(self.sigma_max)
        unit = (torch.clamp(log_sigma, lo, hi) - lo) / (hi - lo)
        return torch.clamp(unit * (t_max - t_min) + t_min, t_min, t_max)

    def solve_schedule(self, num_steps: int, t_min: Optional[float] = None, t_max: Optional[float] = None) -> Tensor:
        t_min = self.t_min if t_min is None else t_min
        t_max = self.t_max if t_max is None else t_max
        if t_min >= t_max:
            raise ValueError(f"t_min ({t_min}) must be less than t_max ({t_max}).")
        dev = self._mean_base.device
        if self._solve_schedule_type == "uniform":
            return torch.linspace(t_max, t_min, num_steps, device=dev)
        rho_inv = 1.0 / self.power_law_exponent
        steps = torch.linspace(0, 1, num_steps, device=dev)
        hi, lo = self.sigma_max**rho_inv, self.sigma_min**rho_inv
        sigmas = (hi + steps * (lo - hi)) ** self.power_law_exponent
        unit = torch.log(sigmas / self.sigma_min) / math.log(self.sigma_max / self.sigma_min)
        times = unit * (t_max - t_min) + t_min
        times[0] = t_max
        if num_steps > 1:
            times[-1] = t_min
        return times


_ESTIMATORS = {"ve": VEScoreEstimator, "vp": VPScoreEstimator, "subvp": SubVPScoreEstimator}
_VE_KEYS = ("sigma_min", "sigma_max", "train_schedule", "solve_schedule", "lognormal_mean", "lognormal_std",
            "power_law_exponent")
_VP_KEYS = ("beta_min", "beta_max")


def build_score_matching_estimator(batch_theta: Tensor, batch_x: Tensor, sde_type: str = "ve",
                                   z_score_theta: Optional[str] = "independent",
                                   z_score_x: Optional[str] = "independent", hidden_features: int = 100,
                                   num_layers: int = 5, time_embedding_dim: int = 32,
                                   sinusoidal_max_freq: float = 1000.0, weight_fn="max_likelihood",
                                   **kwargs) -> ConditionalScoreEstimator:
    """``build_vector_field_estimator(..., estimator_type="score", net="mlp")`` (vector_field_nets.py:136-339) for the
    configuration family the kernels implement."""
    from sbi_amd.utils.sbiutils import standardizing_stats, z_score_parser, z_standardization

    if sde_type not in _ESTIMATORS:
        raise ValueError(f"Unknown SDE type: {sde_type}")
    est_keys = _VE_KEYS if sde_type == "ve" else _VP_KEYS
    est_kwargs = {k: kwargs.pop(k) for k in list(kwargs) if k in est_keys}
    for k in ("t_min", "t_max"):
        if k in kwargs:
            est_kwargs[k] = kwargs.pop(k)
    defaults = dict(net="mlp", model="mlp", time_emb_type="sinusoidal", gaussian_baseline=False, estimator_type="score",
                    compose_standardization=False, layer_norm=True, skip_connections=True)
    for k, v in kwargs.items():
        if k == "embedding_net" and (v is None or isinstance(v, nn.Identity)):
            continue
        if k in defaults and v == defaults[k]:
            continue
        if k in _VE_KEYS + _VP_KEYS:      # the other family's knobs are ignored, as in the reference's builder
            continue
        raise NotImplementedError(f"sbi_amd NPSE: option {k}={v!r} is outside the HIP path (what runs: net='mlp', "
                                  "flat theta and x, no embedding net, no composed standardisation, weight_fn "
                                  "'identity' | 'max_likelihood' | 'variance')")
    if batch_theta.dim() != 2 or batch_x.dim() != 2:
        raise NotImplementedError("sbi_amd NPSE: theta and x must be (N, D) / (N, C)")
    D, C = batch_theta.shape[1], batch_x.shape[1]
    zt, structured_t = z_score_parser(z_score_theta)
    zx, structured_x = z_score_parser(z_score_x)
    mean_0, std_0 = z_standardization(batch_theta, structured_t) if zt else (torch.zeros(D), torch.ones(D))
    x_mean, x_std = standardizing_stats(batch_x, structured_x) if zx else (torch.zeros(C), torch.ones(C))
    zstats = torch.cat([mean_0.reshape(-1).expand(D).cpu().float(), std_0.reshape(-1).expand(D).cpu().float(),
                        x_mean.reshape(-1).expand(C).cpu().float(), x_std.reshape(-1).expand(C).cpu().float()])
    hyper = FMPEHyper(D=D, C=C, hidden_features=hidden_features, num_layers=num_layers,
                      time_embedding_dim=time_embedding_dim, sinusoidal_max_freq=sinusoidal_max_freq)
    net = VectorFieldMLPParams(hyper, zstats)
    return _ESTIMATORS[sde_type](net, torch.Size([D]), torch.Size([C]), weight_fn=weight_fn, **est_kwargs)
