"""Mixture-density-network posterior estimator ("mdn") on the MI355X HIP kernels (include/sbi_amd_mdn.h).

``MixtureDensityEstimator`` is the drop-in for sbi's class of the same name around a ``MultivariateGaussianMDN``
(sbi/neural_nets/estimators/mixture_density_estimator.py, mog.py, net_builders/mdn.py): a two-layer ReLU MLP on the
(z-scored, embedded) condition with four heads -- logits, means, unconstrained diagonal, strict upper triangle --
of a mixture of K full-covariance Gaussians parameterised by upper-triangular precision factors.  ``log_prob``,
``loss``, ``sample`` and ``get_uncorrected_mog`` run in ``libsbi_amd_nsf.so``; there is no PyTorch / CPU fallback.

Parameters live in ONE flat fp32 ``nn.Parameter`` in torch order under the reference's key names; ``state_dict()``
speaks those names (``net._hidden_net.0.weight`` ..., ``_transform_shift``, ``_transform_scale``,
``_embedding_net.0._mean`` / ``_std``) and ``load_state_dict()`` accepts them.

Multi-round inference on this estimator is NPE-A (``sbi_amd.inference.NPE_A``: plain maximum likelihood every round,
then the closed-form MoG correction of sbi_amd/neural_nets/estimators/mog_ops.py).

Not implemented (refused by name): ``MoG.condition``, the closed-form MoG proposal correction inside NPE-C's loss
(use NPE_A), a custom ``hidden_net``, the MDN as a likelihood estimator, ``z_score_x="transform_to_unconstrained"``.
"""

from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.nsf_flow import NSFFlow

ENVELOPE = "MDN: 1 <= theta-dim <= 16, 1 <= x-dim <= 64, 1 <= hidden_features <= 64, 1 <= num_components <= 16"


@dataclass(frozen=True)
class MDNHyper:
    D: int
    C: int
    hidden_features: int = 50
    num_components: int = 10
    epsilon: float = 1e-4

    @property
    def U(self) -> int:
        return self.D * (self.D - 1) // 2

    def c_config(self) -> _lib.MDNConfigC:
        return _lib.MDNConfigC(self.D, self.C, self.hidden_features, self.num_components, self.epsilon)

    def layer_entries(self) -> List[Tuple[str, Tuple[int, ...]]]:
        """(reference sub-key, shape) in flat order."""
        H, D, C, K = self.hidden_features, self.D, self.C, self.num_components
        lin = [("_hidden_net.0", H, C), ("_hidden_net.2", H, H), ("_logits_layer", K, H), ("_means_layer", K * D, H),
               ("_unconstrained_diagonal_layer", K * D, H)] + ([("_upper_layer", K * self.U, H)] if self.U else [])
        out = []
        for key, o, i in lin:
            out += [(key + ".weight", (o, i)), (key + ".bias", (o,))]
        return out

    def param_count(self) -> int:
        return sum(int(np.prod(s)) for _, s in self.layer_entries())

    def in_envelope(self) -> bool:
        return (1 <= self.D <= 16 and 1 <= self.C <= 64 and 1 <= self.hidden_features <= 64
                and 1 <= self.num_components <= 16)


class MDNNet(nn.Module):
    """Parameter / buffer holder in the role of the reference's ``MultivariateGaussianMDN``.

    ``zstats`` = [theta shift (D) | theta scale (D) | x mean (C) | x std (C)]: z = (theta - shift) / scale (the
    reference's ``_transform_shift`` / ``_transform_scale``), c = (x - mean) / std (its ``standardizing_net``)."""

    supports_atomic = False

    def __init__(self, hyper: MDNHyper, zstats: Tensor, z_score_theta: bool, z_score_x: bool):
        super().__init__()
        self.hyper = hyper
        self.z_score_theta = z_score_theta
        self.z_score_x = z_score_x
        self.flat_params = nn.Parameter(torch.zeros(hyper.param_count(), dtype=torch.float32))
        self.register_buffer("zstats", zstats.to(torch.float32).contiguous())
        self.reset_parameters()

    def _slices(self):
        off = 0
        for key, shape in self.hyper.layer_entries():
            n = int(np.prod(shape))
            yield key, off, n, shape
            off += n

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """The reference's construction order (hidden linears, logits, means, diagonal, upper: torch's Linear default)
        followed by its ``_initialize`` (what ``build_mdn`` always asks for), drawing from torch's global generator."""
        h = self.hyper
        H, D, C, K, eps = h.hidden_features, h.D, h.C, h.num_components, h.epsilon
        mods = [nn.Linear(C, H), nn.Linear(H, H), nn.Linear(H, K), nn.Linear(H, K * D), nn.Linear(H, K * D)]
        if h.U:
            mods.append(nn.Linear(H, K * h.U))
        nn.init.normal_(mods[2].weight, mean=0.0, std=eps)
        nn.init.normal_(mods[2].bias, mean=0.0, std=eps)
        nn.init.normal_(mods[4].weight, mean=0.0, std=eps)
        nn.init.constant_(mods[4].bias, math.log(math.exp(1.0 - eps) - 1.0))
        if h.U:
            nn.init.normal_(mods[5].weight, mean=0.0, std=eps)
            nn.init.zeros_(mods[5].bias)
        flat = torch.cat([t.detach().reshape(-1) for m in mods for t in (m.weight, m.bias)])
        assert flat.numel() == self.flat_params.numel()
        self.flat_params.copy_(flat)

    def native_state_dict(self) -> "OrderedDict[str, Tensor]":
        """The two-tensor form (`flat_params`, `zstats`): what the kernels read, no per-layer views."""
        return OrderedDict(flat_params=self.flat_params.detach(), zstats=self.zstats)

    # -- fused training pass (the FusedTrainStep contract) -------------------------------------------
    def train_workspace_floats(self, n: int) -> int:
        need = _lib.load().sbi_amd_mdn_train_workspace_floats(self.hyper.c_config(), n)
        if need < 0:
            _lib.check(int(need), "mdn_train_workspace_floats")
        return int(need)

    def train_pass(self, theta: Tensor, x: Tensor, row_weight: Optional[Tensor], uniform_weight: float,
                   grad_out: Tensor, workspace: Optional[Tensor] = None, want_grad_theta: bool = False,
                   grad_x_out: Optional[Tensor] = None):
        if grad_x_out is not None:
            raise NotImplementedError("the MDN kernels do not return d loss / d embedded x (no trainable embedding)")
        return mdn_loss_fwd_bwd(self, theta, x, row_weight, uniform_weight, grad_out, want_grad_theta, workspace)


# --------------------------------------------------------------------- kernel calls
def mdn_packed_weights(net: MDNNet) -> Tensor:
    fp = net.flat_params
    key = (fp.data_ptr(), fp._version, str(fp.device))
    cache = net.__dict__.get("_packed_cache")
    if cache is not None and cache[0] == key:
        return cache[1]
    dev = _lib.require_device(fp)
    lib = _lib.load()
    cfg = net.hyper.c_config()
    n = lib.sbi_amd_mdn_packed_floats(cfg)
    if n < 0:
        _lib.check(int(n), f"mdn_packed_floats ({ENVELOPE})")
    packed = cache[1] if (cache is not None and cache[1].device == dev and cache[1].numel() == n) else \
        torch.zeros(int(n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_mdn_pack(cfg, _lib.ptr(fp), _lib.ptr(packed), _lib.current_stream(dev))
    _lib.check(rc, "mdn_pack")
    net.__dict__["_packed_cache"] = (key, packed)
    return packed


def mdn_log_prob_call(net: MDNNet, theta: Tensor, x: Tensor) -> Tensor:
    dev = _lib.require_device(theta, x, net.flat_params, net.zstats)
    n = theta.shape[0]
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return logp
    packed = mdn_packed_weights(net)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_mdn_log_prob(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                              _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(logp),
                                              _lib.current_stream(dev))
    _lib.check(rc, "mdn_log_prob")
    return logp


def mdn_sample_call(net: MDNNet, zeta: Tensor, x: Tensor, u: Optional[Tensor] = None,
                    comp: Optional[Tensor] = None) -> Tensor:
    """theta (n, D) for given normal draws `zeta` and either uniforms `u` (n,) or components `comp` (n,) int32."""
    dev = _lib.require_device(zeta, x, net.flat_params, net.zstats, u)
    if comp is not None and (comp.dtype != torch.int32 or not comp.is_contiguous() or comp.device != dev):
        raise TypeError("sbi_amd: `comp` must be a contiguous int32 tensor on the kernels' device")
    if u is None and comp is None:
        raise ValueError("sbi_amd: mdn_sample_call needs `u` or `comp`")
    n = zeta.shape[0]
    theta = torch.empty_like(zeta)
    if n == 0:
        return theta
    packed = mdn_packed_weights(net)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_mdn_sample(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(u),
                                            _lib.ptr(comp), _lib.ptr(zeta), _lib.ptr(x), n, x.shape[0],
                                            _lib.ptr(theta), _lib.current_stream(dev))
    _lib.check(rc, "mdn_sample")
    return theta


def mdn_components_call(net: MDNNet, x: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(logits (n, K), means (n, K, D), factors (n, K, D + U)) of the condition rows x (n, C)."""
    dev = _lib.require_device(x, net.flat_params, net.zstats)
    h = net.hyper
    n, K, D = x.shape[0], h.num_components, h.D
    logits = torch.empty(n, K, dtype=torch.float32, device=dev)
    means = torch.empty(n, K, D, dtype=torch.float32, device=dev)
    factors = torch.empty(n, K, D + h.U, dtype=torch.float32, device=dev)
    if n:
        packed = mdn_packed_weights(net)
        with torch.cuda.device(dev):
            rc = _lib.load().sbi_amd_mdn_components(h.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(x), n,
                                                    _lib.ptr(logits), _lib.ptr(means), _lib.ptr(factors),
                                                    _lib.current_stream(dev))
        _lib.check(rc, "mdn_components")
    return logits, means, factors


def mdn_loss_fwd_bwd(net: MDNNet, theta: Tensor, x: Tensor, row_weight: Optional[Tensor], uniform_weight: float,
                     grad_out: Tensor, want_grad_theta: bool = False, workspace: Optional[Tensor] = None):
    """Fused training pass: (per-row loss, grad_theta | None); fills grad_out (P,)."""
    dev = _lib.require_device(theta, x, net.flat_params, net.zstats, grad_out, row_weight)
    n = theta.shape[0]
    need = net.train_workspace_floats(n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    gtheta = torch.empty_like(theta) if want_grad_theta else None
    packed = mdn_packed_weights(net)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_mdn_loss_fwd_bwd(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                                  _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(row_weight),
                                                  float(uniform_weight), _lib.ptr(loss), _lib.ptr(grad_out),
                                                  _lib.ptr(gtheta), _lib.ptr(workspace), _lib.current_stream(dev))
    _lib.check(rc, "mdn_loss_fwd_bwd")
    return loss, gtheta


class _MDNLogProbFn(torch.autograd.Function):
    """Autograd bridge: forward = the log_prob kernel; backward = the fused training pass with row weights
    -dL/dlogp."""

    @staticmethod
    def forward(ctx, theta: Tensor, x: Tensor, flat_params: Tensor, net: MDNNet):
        ctx.net = net
        ctx.version = net.flat_params._version
        ctx.save_for_backward(theta, x)
        return mdn_log_prob_call(net, theta, x)

    @staticmethod
    def backward(ctx, grad_logp: Tensor):
        theta, x = ctx.saved_tensors
        net: MDNNet = ctx.net
        if net.flat_params._version != ctx.version:
            raise RuntimeError("MDN parameters were modified in place between log_prob() and backward().")
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("the MDN kernels do not return the gradient wrt the condition")
        gparams = torch.empty_like(net.flat_params)
        w = (-grad_logp).contiguous().to(torch.float32)
        _, gtheta = mdn_loss_fwd_bwd(net, theta, x, w, 0.0, gparams, want_grad_theta=ctx.needs_input_grad[0])
        return gtheta, None, (gparams if ctx.needs_input_grad[2] else None), None


@dataclass
class MoG:
    """A batch of mixtures of Gaussians with sbi's ``MoG`` surface (neural_nets/estimators/mog.py): logits (B, K)
    unnormalised, means (B, K, D), precisions (B, K, D, D), precision_factors (B, K, D, D) upper triangular with
    precision = A^T A (derived by a Cholesky factorisation of precisions + 1e-6 I when not given).  ``log_prob`` and
    ``sample`` run on the gfx950 kernels of include/sbi_amd_mog.h for float32 tensors on a ROCm device inside their
    envelope, and as eager torch otherwise (sbi_amd/neural_nets/estimators/mog_ops.py).  NPE-A (``NPE_A``) corrects
    these mixtures in closed form; ``condition`` is not implemented."""

    logits: Tensor
    means: Tensor
    precisions: Tensor
    precision_factors: Optional[Tensor] = None

    _CHOLESKY_EPSILON: ClassVar[float] = 1e-6

    def __post_init__(self) -> None:
        if self.logits.dim() != 2:
            raise ValueError(f"logits must be 2D (batch_size, num_components), got {self.logits.dim()}D")
        if self.means.dim() != 3:
            raise ValueError(f"means must be 3D (batch_size, num_components, dim), got {self.means.dim()}D")
        if self.precisions.dim() != 4:
            raise ValueError(
                f"precisions must be 4D (batch_size, num_components, dim, dim), got {self.precisions.dim()}D")
        batch_size, num_components = self.logits.shape
        if self.means.shape[:2] != (batch_size, num_components):
            raise ValueError(f"means shape {self.means.shape} incompatible with logits shape {self.logits.shape}")
        if self.precisions.shape[:2] != (batch_size, num_components):
            raise ValueError(
                f"precisions shape {self.precisions.shape} incompatible with logits shape {self.logits.shape}")
        dim = self.means.shape[2]
        if self.precisions.shape[2:] != (dim, dim):
            raise ValueError(
                f"precisions must be square matrices of size ({dim}, {dim}), got {self.precisions.shape[2:]}")
        # one read-back for the three finiteness checks; the names are looked up only when something is wrong
        finite = torch.stack([torch.isfinite(t).all() for t in (self.logits, self.means, self.precisions)]).tolist()
        for ok, name in zip(finite, ("logits", "means", "precisions")):
            if not ok:
                raise ValueError(f"{name} contains NaN or Inf values")
        if self.precision_factors is None:
            eye = torch.eye(dim, device=self.precisions.device, dtype=self.precisions.dtype)
            L, info = torch.linalg.cholesky_ex(self.precisions + self._CHOLESKY_EPSILON * eye)
            if bool((info > 0).any()):
                raise ValueError(
                    "Failed to compute Cholesky decomposition of precision matrix. This indicates the precision "
                    "matrix is not positive definite. Check that your MoG parameters are valid. "
                    f"Original error: leading minor of order {int(info.max())} is not positive definite")
            self.precision_factors = L.transpose(-2, -1)
        else:
            if self.precision_factors.shape != self.precisions.shape:
                raise ValueError(f"precision_factors shape {self.precision_factors.shape} must match precisions "
                                 f"shape {self.precisions.shape}")
            if not bool(torch.isfinite(self.precision_factors).all()):
                raise ValueError("precision_factors contains NaN or Inf values")

    @property
    def num_components(self) -> int:
        return self.logits.shape[1]

    @property
    def dim(self) -> int:
        return self.means.shape[2]

    @property
    def batch_shape(self) -> torch.Size:
        return torch.Size([self.logits.shape[0]])

    @property
    def device(self) -> torch.device:
        return self.logits.device

    @property
    def dtype(self) -> torch.dtype:
        return self.logits.dtype

    @property
    def log_weights(self) -> Tensor:
        return self.logits - torch.logsumexp(self.logits, dim=-1, keepdim=True)

    @property
    def weights(self) -> Tensor:
        return torch.softmax(self.logits, dim=-1)

    def log_prob(self, inputs: Tensor) -> Tensor:
        """(batch_size, dim) -> (batch_size,); (sample_size, batch_size, dim) -> (sample_size, batch_size).  Batch
        column b is evaluated under mixture row b (a one-row mixture serves every column)."""
        from sbi_amd.neural_nets.estimators import mog_ops

        squeeze = inputs.dim() == 2
        if squeeze:
            inputs = inputs.unsqueeze(0)
        S, B, D = inputs.shape
        if B != self.logits.shape[0] and self.logits.shape[0] != 1:
            raise ValueError(f"inputs have batch size {B}, the mixture has {self.logits.shape[0]} rows")
        out = mog_ops.mog_log_prob(self.logits, self.means, self.precisions, self.precision_factors,
                                   inputs.reshape(S * B, D)).reshape(S, B)
        return out[0] if squeeze else out

    def sample(self, sample_shape: torch.Size = torch.Size()) -> Tensor:
        """(*sample_shape, batch_size, dim): one uniform (component, inverse CDF of the weights) and `dim` normals
        per draw, rows sample-major."""
        from sbi_amd.neural_nets.estimators import mog_ops

        shape = torch.Size(sample_shape)
        n = int(shape.numel()) if len(shape) else 1
        B, D = self.logits.shape[0], self.dim
        u = torch.rand(n * B, device=self.device, dtype=self.dtype)
        zeta = torch.randn(n * B, D, device=self.device, dtype=self.dtype)
        out = mog_ops.mog_sample(self.logits, self.means, self.precision_factors, zeta, u=u)
        return out.reshape(*shape, B, D) if len(shape) else out.reshape(B, D)

    def to(self, device) -> "MoG":
        return MoG(self.logits.to(device), self.means.to(device), self.precisions.to(device),
                   self.precision_factors.to(device))

    def detach(self) -> "MoG":
        return MoG(self.logits.detach(), self.means.detach(), self.precisions.detach(),
                   self.precision_factors.detach())

    @classmethod
    def from_gaussian(cls, mean: Tensor, covariance: Tensor) -> "MoG":
        """A one-component mixture from a Gaussian's mean (dim,) / (B, dim) and covariance (dim, dim) / (B, dim, dim)."""
        if mean.dim() == 1:
            mean = mean.unsqueeze(0)
        if covariance.dim() == 2:
            covariance = covariance.unsqueeze(0)
        precision = torch.linalg.inv(covariance)
        factor = torch.linalg.cholesky(precision).transpose(-2, -1)
        logits = torch.zeros(mean.shape[0], 1, device=mean.device, dtype=mean.dtype)
        return cls(logits=logits, means=mean.unsqueeze(1), precisions=precision.unsqueeze(1),
                   precision_factors=factor.unsqueeze(1))

    def condition(self, *args, **kwargs):
        raise NotImplementedError("sbi_amd: MoG.condition (conditioning a mixture on a subset of its dimensions) is "
                                  "not implemented")


class MixtureDensityEstimator(NSFFlow):
    r"""Mixture of Gaussians :math:`p(\theta|x)` whose parameters a small MLP predicts, evaluated by the gfx950
    kernels.  The plumbing around the kernels (embedding net, shape checks, CPU-resident staging) is NSFFlow's."""

    def __init__(self, net: MDNNet, input_shape: torch.Size, condition_shape: torch.Size,
                 embedding_net: Optional[nn.Module] = None) -> None:
        super().__init__(net, input_shape=input_shape, condition_shape=condition_shape, embedding_net=embedding_net)
        if embedding_net is not None and any(p.requires_grad for p in embedding_net.parameters()):
            raise NotImplementedError("sbi_amd mdn: trainable embedding nets are not supported (frozen / "
                                      "parameter-free ones are applied in front of the kernels)")
        self._register_state_dict_hook(MixtureDensityEstimator._emit_reference_keys)
        self._register_load_state_dict_pre_hook(self._accept_reference_keys, with_module=False)

    # -- checkpoints in the reference's key names ------------------------------------------------------
    @staticmethod
    def _emit_reference_keys(module, state_dict, prefix, local_metadata):
        net = module.net
        if getattr(net, "_native_state_dict", False):
            return state_dict
        h = net.hyper
        flat = state_dict.pop(prefix + "net.flat_params")
        zst = state_dict.pop(prefix + "net.zstats")
        out = OrderedDict()
        if net.z_score_theta:
            out[prefix + "_transform_shift"] = zst[: h.D].clone()
            out[prefix + "_transform_scale"] = zst[h.D : 2 * h.D].clone()
        for key, off, n, shape in net._slices():
            out[prefix + "net." + key] = flat[off : off + n].reshape(shape).clone()
        if net.z_score_x:
            out[prefix + "_embedding_net.0._mean"] = zst[2 * h.D : 2 * h.D + h.C].clone()
            out[prefix + "_embedding_net.0._std"] = zst[2 * h.D + h.C :].clone()
        for k, v in state_dict.items():      # (a frozen embedding net's own entries)
            out[k] = v
        state_dict.clear()
        state_dict.update(out)
        return state_dict

    def _accept_reference_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                               error_msgs):
        if prefix + "net.flat_params" in state_dict:
            return      # native form
        net, h = self.net, self.net.hyper
        if prefix + "net._hidden_net.0.weight" not in state_dict:
            return      # nothing of ours: let the regular missing-key report speak
        flat = net.flat_params.detach().clone()
        zst = net.zstats.detach().clone()
        try:
            for key, off, n, shape in net._slices():
                src = state_dict.pop(prefix + "net." + key)
                if tuple(src.shape) != tuple(shape):
                    raise ValueError(f"{key}: expected {shape}, got {tuple(src.shape)}")
                flat[off : off + n] = src.reshape(-1).to(flat)
            if net.z_score_theta:
                zst[: h.D] = state_dict.pop(prefix + "_transform_shift").reshape(-1).to(zst)
                zst[h.D : 2 * h.D] = state_dict.pop(prefix + "_transform_scale").reshape(-1).to(zst)
            if net.z_score_x and self._embedding_net is None:
                zst[2 * h.D : 2 * h.D + h.C] = state_dict.pop(prefix + "_embedding_net.0._mean").reshape(-1).expand(h.C).to(zst)
                zst[2 * h.D + h.C :] = state_dict.pop(prefix + "_embedding_net.0._std").reshape(-1).expand(h.C).to(zst)
        except (KeyError, ValueError) as e:
            error_msgs.append(f"MixtureDensityEstimator: cannot read the reference-keyed checkpoint: {e!r}")
            return
        state_dict[prefix + "net.flat_params"] = flat
        state_dict[prefix + "net.zstats"] = zst
        net.__dict__.pop("_packed_cache", None)

    # -- kernel hooks ------------------------------------------------------------------------------------
    def _raw_log_prob(self, net, theta: Tensor, x: Tensor, want_noise: bool):
        if want_noise:
            raise NotImplementedError("a mixture density network has no base-noise transform (inverse_transform)")
        return mdn_log_prob_call(net, theta, x), None

    def _raw_sample(self, net, noise: Tensor, x: Tensor, want_ld: bool):
        raise NotImplementedError("a mixture density network is not a flow: use sample() / sample_given()")

    def _raw_autograd(self, net, theta: Tensor, x: Tensor, flat: Tensor) -> Tensor:
        return _MDNLogProbFn.apply(theta, x, flat, net)

    def inverse_transform(self, input: Tensor, condition: Tensor) -> Tensor:
        raise NotImplementedError("a mixture density network has no base-noise transform (inverse_transform)")

    def sample_from_noise(self, noise: Tensor, condition: Tensor, with_logabsdet: bool = False):
        raise NotImplementedError("a mixture density network is not a flow: use sample() / sample_given()")

    # -- estimator surface ---------------------------------------------------------------------------------
    def log_prob(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        """(sample_dim, batch_dim) for an input with a sample dimension, (batch_dim,) without one."""
        has_sample_dim = input.dim() > len(self.input_shape) + 1
        lp = super().log_prob(input, condition)
        return lp if has_sample_dim else lp[0]

    def loss(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        has_sample_dim = input.dim() > len(self.input_shape) + 1
        lp = super().log_prob(input if has_sample_dim else input.unsqueeze(0), condition)
        return -lp if has_sample_dim else -lp[0]

    def _embedded_rows(self, condition: Tensor) -> Tensor:
        self._check_condition_shape(condition)
        with torch.no_grad():
            emb = self._embed(condition)
        return emb.reshape(-1, self._cdim).contiguous().float()

    def sample_given(self, zeta: Tensor, condition: Tensor, u: Optional[Tensor] = None,
                     comp: Optional[Tensor] = None) -> Tensor:
        """theta (n, D) for given normal draws: row i pairs with condition[i % rows]; component from the uniforms `u`
        (inverse CDF of the mixture weights) or given by `comp`."""
        x = self._embedded_rows(condition)
        net = self._kernel_net()
        dev = net.flat_params.device
        with torch.no_grad():
            out = mdn_sample_call(net, zeta.to(dev).contiguous().float(), x.to(dev),
                                  None if u is None else u.to(dev).contiguous().float(),
                                  None if comp is None else comp.to(dev, torch.int32).contiguous())
        return out.to(zeta.device)

    def sample(self, sample_shape: torch.Size, condition: Tensor, **kwargs) -> Tensor:
        """(*sample_shape, batch_dim, D): one uniform (component) and D normals per draw, rows sample-major so that
        the kernel's x[row % batch_dim] pairs every draw with its condition."""
        self._check_condition_shape(condition)
        Bc = condition.shape[0]
        n = torch.Size(sample_shape).numel()
        D = self.input_shape[0]
        dev = condition.device
        u = torch.rand(n * Bc, device=dev, dtype=torch.float32)
        zeta = torch.randn(n * Bc, D, device=dev, dtype=torch.float32)
        theta = self.sample_given(zeta, condition, u=u)
        return theta.reshape((*sample_shape, Bc, *self.input_shape))

    def sample_and_log_prob(self, sample_shape: torch.Size, condition: Tensor, **kwargs) -> Tuple[Tensor, Tensor]:
        theta = self.sample(sample_shape, condition)
        Bc = condition.shape[0]
        with torch.no_grad():
            lp = super().log_prob(theta.reshape(-1, Bc, self.input_shape[0]), condition)
        return theta, lp.reshape((*sample_shape, Bc))

    def get_uncorrected_mog(self, condition: Tensor) -> MoG:
        """Mixture parameters of every condition row (the device version of the reference's method)."""
        x = self._embedded_rows(condition)
        net = self._kernel_net()
        dev = net.flat_params.device
        h = net.hyper
        D = h.D
        with torch.no_grad():
            logits, means, fac = mdn_components_call(net, x.to(dev))
            A = torch.zeros(x.shape[0], h.num_components, D, D, dtype=torch.float32, device=dev)
            idx = torch.arange(D, device=dev)
            A[..., idx, idx] = fac[..., :D]
            if h.U:
                r, c = np.triu_indices(D, 1)
                A[..., torch.as_tensor(r, device=dev), torch.as_tensor(c, device=dev)] = fac[..., D:]
            prec = A.transpose(-1, -2) @ A + h.epsilon * torch.eye(D, device=dev)
        to = condition.device
        return MoG(logits=logits.to(to), means=means.to(to), precisions=prec.to(to), precision_factors=A.to(to))
