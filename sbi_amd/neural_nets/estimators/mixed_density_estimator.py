"""Mixed discrete / continuous likelihood estimator (MNLE) on the MI355X HIP kernels (include/sbi_amd_mnle.h).

``MixedDensityEstimator`` is the drop-in for sbi's class of the same name (sbi/neural_nets/estimators/
mixed_density_estimator.py) for the data shape x = [one continuous column, V categorical columns], 1 <= V <= 4: a
``CategoricalMADE`` over the categorical columns given theta and a 1-D neural spline flow over the continuous column
given (category values, theta) through a trainable combined embedding.  ``log_prob``, ``loss``, ``sample`` and the iid
trials potential run in ``libsbi_amd_nsf.so``; there is no PyTorch / CPU fallback.

Parameters live in ONE flat fp32 ``nn.Parameter``; ``state_dict()`` speaks the reference's key names
(``discrete_net.net.initial_layer.weight``, ``...blocks.0.linear_layers.1.bias``, ``...blocks.0.context_layer.weight``,
the buffers ``discrete_net.net.mask`` / ``degrees`` / ``values_lookup``,
``continuous_net.net._embedding_net.0.weight``, ``..._transform._transforms.i.transform_net.spline_predictor.j.*``) and
``load_state_dict()`` accepts them.  The names below ``discrete_net.net`` and ``continuous_net.net`` belong to nflows,
which is not importable next to this package: they are RECALLED (nflows.transforms.made.MADE, nflows.flows.Flow,
nflows' coupling transform attribute ``transform_net``), not checked against an install.

Not implemented (refused by name): more or fewer than one continuous column, more than 4 discrete columns or 16
categories, continuous models other than the NSF, dropout, a custom combined embedding, MNPE, conditioning on theta.
"""

from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.base import ConditionalDensityEstimator

ENVELOPE = ("MNLE: 1..4 discrete columns with <= 16 categories each, theta-dim <= 64, every width <= 64, <= 4 "
            "discrete blocks, <= 16 transforms, num_bins in {4, 5, 8, 10, 16}, 0..4 spline-context layers")
MAX_CATEGORIES = 16


@dataclass(frozen=True)
class MNLEHyper:
    num_categories: Tuple[int, ...]
    C: int
    discrete_hidden: int = 50
    discrete_blocks: int = 2
    embedding: int = 50
    hidden: int = 50
    num_bins: int = 10
    num_transforms: int = 5
    context_layers: int = 1
    tail_bound: float = 10.0
    log_transform: bool = False
    z_score_x: bool = True

    V = property(lambda self: len(self.num_categories))
    F = property(lambda self: len(self.num_categories) + 1)
    Kmax = property(lambda self: max(self.num_categories))

    def c_config(self) -> _lib.MNLEConfigC:
        nc = tuple(self.num_categories) + (0,) * (4 - self.V)
        return _lib.MNLEConfigC(self.V, nc[:4], self.C, self.discrete_hidden, self.discrete_blocks, self.embedding,
                                self.hidden, self.num_bins, self.num_transforms, self.context_layers,
                                int(self.log_transform), self.tail_bound, 1e-3, 1e-3, 1e-3)

    def linears(self) -> List[Tuple[str, int, int]]:
        """(reference key, out, in) of every linear in the flat order of include/sbi_amd_mnle.h."""
        Hd, E, Hc, C, V, L = self.discrete_hidden, self.embedding, self.hidden, self.C, self.V, self.context_layers
        d, c = "discrete_net.net.", "continuous_net.net."
        out = [(d + "initial_layer", Hd, self.F), (d + "context_layer", Hd, C)]
        for b in range(self.discrete_blocks):
            out += [(d + f"blocks.{b}.linear_layers.0", Hd, Hd), (d + f"blocks.{b}.linear_layers.1", Hd, Hd),
                    (d + f"blocks.{b}.context_layer", Hd, C)]
        out += [(d + "final_layer", self.F * self.Kmax, Hd), (c + "_embedding_net.0", E, V + C),
                (c + "_embedding_net.2", E, E)]
        for t in range(self.num_transforms):
            p = c + f"_transform._transforms.{t + int(self.z_score_x)}.transform_net.spline_predictor."
            out.append((p + "0", Hc, E))
            if L > 0:
                out.append((p + "2", Hc, Hc))
            out.append((p + str(2 + 2 * L), 3 * self.num_bins - 1, Hc))
        return out

    def layer_entries(self) -> List[Tuple[str, Tuple[int, ...]]]:
        out = []
        for key, o, i in self.linears():
            out += [(key + ".weight", (o, i)), (key + ".bias", (o,))]
        return out

    def param_count(self) -> int:
        return sum(o * i + o for _, o, i in self.linears())

    def in_envelope(self) -> bool:
        return (1 <= self.V <= 4 and all(1 <= k <= MAX_CATEGORIES for k in self.num_categories) and 1 <= self.C <= 64
                and all(1 <= w <= 64 for w in (self.discrete_hidden, self.embedding, self.hidden))
                and 0 <= self.discrete_blocks <= 4 and 1 <= self.num_transforms <= 16
                and self.num_bins in (4, 5, 8, 10, 16) and 0 <= self.context_layers <= 4)

    # -- MADE degrees / masks (nflows.transforms.made with random_mask=False, restated in oracle/maf_oracle.py)
    def hidden_degrees(self) -> Tensor:
        return torch.arange(self.discrete_hidden) % max(1, self.F - 1) + min(1, self.F - 1)

    def made_mask(self, which: str) -> Tensor:
        hd = self.hidden_degrees()
        if which == "initial":
            return (hd[:, None] >= torch.arange(1, self.F + 1)).float()
        if which == "hidden":
            return (hd[:, None] >= hd).float()
        out_deg = torch.repeat_interleave(torch.arange(1, self.F + 1), self.Kmax)
        return (out_deg[:, None] > hd).float()


class MNLENet(nn.Module):
    """Parameter / buffer holder.  ``zstats`` = [x shift, x scale (z = x * scale + shift), theta mean (C), theta std
    (C), values_lookup (V x 16: every variable's sorted raw values)]."""

    def __init__(self, hyper: MNLEHyper, zstats: Tensor):
        super().__init__()
        self.hyper = hyper
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
        """torch's Linear default for every layer in flat order; the second linear of every residual block
        uniform(-1e-3, 1e-3) (nflows' MaskedResidualBlock zero_initialization)."""
        parts = []
        for key, o, i in self.hyper.linears():
            m = nn.Linear(i, o)
            if key.endswith("linear_layers.1"):
                nn.init.uniform_(m.weight, -1e-3, 1e-3)
                nn.init.uniform_(m.bias, -1e-3, 1e-3)
            parts += [m.weight.detach().reshape(-1), m.bias.detach().reshape(-1)]
        self.flat_params.copy_(torch.cat(parts))

    @property
    def lookup(self) -> Tensor:
        h = self.hyper
        return self.zstats[2 + 2 * h.C:].reshape(h.V, MAX_CATEGORIES)

    def train_workspace_floats(self, n: int) -> int:
        need = _lib.load().sbi_amd_mnle_train_workspace_floats(self.hyper.c_config(), n)
        if need < 0:
            _lib.check(int(need), "mnle_train_workspace_floats")
        return int(need)

    def train_pass(self, x: Tensor, theta: Tensor, row_weight: Optional[Tensor], uniform_weight: float,
                   grad_out: Tensor, workspace: Optional[Tensor] = None, want_grad_theta: bool = False,
                   grad_x_out: Optional[Tensor] = None):
        """The FusedTrainStep contract with the likelihood's roles: input = x (n, 1 + V), condition = theta."""
        if want_grad_theta:
            raise NotImplementedError("the MNLE kernels do not return d loss / d x")
        xc, idx, val = split_input(self, x, validate=False)
        loss, _ = mnle_loss_fwd_bwd(self, xc, idx, val, theta, row_weight, uniform_weight, grad_out, False, workspace,
                                    grad_cond_out=grad_x_out)
        return loss, None


# --------------------------------------------------------------------- value <-> index mapping
def map_values_to_indices(net: MNLENet, values: Tensor, validate: bool = True) -> Tensor:
    """(n, V) raw categorical values -> int32 indices by searchsorted in every variable's sorted training values;
    unseen values raise the reference's ValueError."""
    h = net.hyper
    lookup = net.lookup.to(values.device)
    out = torch.empty(values.shape, dtype=torch.int32, device=values.device)
    for i in range(h.V):
        c = h.num_categories[i]
        uniq = lookup[i, :c].contiguous()
        col = values[..., i].contiguous()
        idx = torch.searchsorted(uniq, col)
        if validate:
            clamped = idx.clamp(0, c - 1)
            bad = (idx != clamped) | (uniq[clamped] != col)
            if bool(bad.any()):
                raise ValueError(f"Variable {i} contains values not seen during training: "
                                 f"{col[bad].unique().tolist()}. Valid values are: {uniq.tolist()}")
        out[..., i] = idx.clamp(0, c - 1)
    return out


def split_input(net: MNLENet, x: Tensor, validate: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """x (n, 1 + V) -> (continuous column (n,), indices (n, V) int32, raw values (n, V))."""
    val = x[:, 1:].contiguous().float()
    return x[:, 0].contiguous().float(), map_values_to_indices(net, val, validate), val


# --------------------------------------------------------------------- kernel calls
def mnle_packed_weights(net: MNLENet) -> Tensor:
    fp = net.flat_params
    key = (fp.data_ptr(), fp._version, str(fp.device))
    cache = net.__dict__.get("_packed_cache")
    if cache is not None and cache[0] == key:
        return cache[1]
    dev = _lib.require_device(fp)
    lib = _lib.load()
    cfg = net.hyper.c_config()
    n = lib.sbi_amd_mnle_packed_floats(cfg)
    if n < 0:
        _lib.check(int(n), f"mnle_packed_floats ({ENVELOPE})")
    packed = cache[1] if (cache is not None and cache[1].device == dev and cache[1].numel() == n) else \
        torch.zeros(int(n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_mnle_pack(cfg, _lib.ptr(fp), _lib.ptr(packed), _lib.current_stream(dev))
    _lib.check(rc, "mnle_pack")
    net.__dict__["_packed_cache"] = (key, packed)
    return packed


def _check_idx(idx: Optional[Tensor], dev) -> None:
    if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous() or idx.device != dev):
        raise TypeError("sbi_amd: category indices must be a contiguous int32 tensor on the kernels' device")


def mnle_log_prob_call(net: MNLENet, x_cont: Optional[Tensor], d_idx: Optional[Tensor], d_val: Optional[Tensor],
                       theta: Tensor, parts: int = 3, n: Optional[int] = None,
                       want_logits: bool = False):
    """log p of n paired rows (condition row i % theta rows); parts bit 0: discrete term, bit 1: continuous term."""
    dev = _lib.require_device(theta, net.flat_params, net.zstats, x_cont, d_val)
    _check_idx(d_idx, dev)
    h = net.hyper
    if n is None:
        n = (x_cont if x_cont is not None else d_idx).shape[0]
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    logits = torch.empty(n, h.V, h.Kmax, dtype=torch.float32, device=dev) if want_logits else None
    if n:
        packed = mnle_packed_weights(net)
        with torch.cuda.device(dev):
            rc = _lib.load().sbi_amd_mnle_log_prob(h.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                                   _lib.ptr(x_cont), _lib.ptr(d_idx), _lib.ptr(d_val), _lib.ptr(theta),
                                                   n, theta.shape[0], parts, _lib.ptr(logp), _lib.ptr(logits),
                                                   _lib.current_stream(dev))
        _lib.check(rc, "mnle_log_prob")
    return (logp, logits) if want_logits else logp


def mnle_trials_call(net: MNLENet, x_cont: Tensor, d_idx: Tensor, d_val: Tensor, theta: Tensor) -> Tensor:
    """out[j] = sum over the trials (rows of x_cont / d_idx / d_val) of log p(x_t | theta_j), in trial order."""
    dev = _lib.require_device(theta, net.flat_params, net.zstats, x_cont, d_val)
    _check_idx(d_idx, dev)
    T, N = x_cont.shape[0], theta.shape[0]
    out = torch.empty(N, dtype=torch.float32, device=dev)
    if N:
        ws = torch.empty(T * N, dtype=torch.float32, device=dev)
        packed = mnle_packed_weights(net)
        with torch.cuda.device(dev):
            rc = _lib.load().sbi_amd_mnle_log_prob_trials(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                                          _lib.ptr(x_cont), _lib.ptr(d_idx), _lib.ptr(d_val),
                                                          _lib.ptr(theta), T, N, _lib.ptr(out), _lib.ptr(ws),
                                                          _lib.current_stream(dev))
        _lib.check(rc, "mnle_log_prob_trials")
    return out


def mnle_sample_call(net: MNLENet, u: Tensor, noise: Tensor, theta: Tensor) -> Tuple[Tensor, Tensor]:
    """(indices (n, V) int32, continuous column (n,)) for uniforms u (n, V) and normal draws noise (n,)."""
    dev = _lib.require_device(theta, net.flat_params, net.zstats, u, noise)
    n = noise.shape[0]
    idx = torch.empty(n, net.hyper.V, dtype=torch.int32, device=dev)
    xc = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        packed = mnle_packed_weights(net)
        with torch.cuda.device(dev):
            rc = _lib.load().sbi_amd_mnle_sample(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                                 _lib.ptr(u), _lib.ptr(noise), _lib.ptr(theta), n, theta.shape[0],
                                                 _lib.ptr(idx), _lib.ptr(xc), _lib.current_stream(dev))
        _lib.check(rc, "mnle_sample")
    return idx, xc


def mnle_loss_fwd_bwd(net: MNLENet, x_cont: Tensor, d_idx: Tensor, d_val: Tensor, theta: Tensor,
                      row_weight: Optional[Tensor], uniform_weight: float, grad_out: Tensor,
                      want_grad_cond: bool = False, workspace: Optional[Tensor] = None,
                      grad_cond_out: Optional[Tensor] = None):
    """Fused training pass: (per-row loss, d / d theta | None); fills grad_out (P,)."""
    dev = _lib.require_device(theta, net.flat_params, net.zstats, x_cont, d_val, grad_out, row_weight, grad_cond_out)
    _check_idx(d_idx, dev)
    n = x_cont.shape[0]
    need = net.train_workspace_floats(n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    gcond = grad_cond_out if grad_cond_out is not None else (torch.empty_like(theta) if want_grad_cond else None)
    packed = mnle_packed_weights(net)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_mnle_loss_fwd_bwd(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                                   _lib.ptr(x_cont), _lib.ptr(d_idx), _lib.ptr(d_val), _lib.ptr(theta),
                                                   n, theta.shape[0], _lib.ptr(row_weight), float(uniform_weight),
                                                   _lib.ptr(loss), _lib.ptr(grad_out), _lib.ptr(gcond),
                                                   _lib.ptr(workspace), _lib.current_stream(dev))
    _lib.check(rc, "mnle_loss_fwd_bwd")
    return loss, gcond


class _MNLELogProbFn(torch.autograd.Function):
    """Autograd bridge: forward = the log_prob kernel; backward = the fused training pass with row weights -dL/dlogp
    (parameter gradient, and d / d theta for posterior.map() or a trainable theta embedding)."""

    @staticmethod
    def forward(ctx, theta: Tensor, flat_params: Tensor, net: MNLENet, x_cont: Tensor, d_idx: Tensor, d_val: Tensor):
        ctx.net = net
        ctx.version = net.flat_params._version
        ctx.save_for_backward(theta, x_cont, d_idx, d_val)
        return mnle_log_prob_call(net, x_cont, d_idx, d_val, theta)

    @staticmethod
    def backward(ctx, grad_logp: Tensor):
        theta, x_cont, d_idx, d_val = ctx.saved_tensors
        net: MNLENet = ctx.net
        if net.flat_params._version != ctx.version:
            raise RuntimeError("MNLE parameters were modified in place between log_prob() and backward().")
        gparams = torch.empty_like(net.flat_params)
        w = (-grad_logp).contiguous().to(torch.float32)
        _, gth = mnle_loss_fwd_bwd(net, x_cont, d_idx, d_val, theta, w, 0.0, gparams,
                                   want_grad_cond=ctx.needs_input_grad[0])
        return gth, (gparams if ctx.needs_input_grad[1] else None), None, None, None, None


class _PartView(nn.Module):
    """``.discrete_net`` / ``.continuous_net``: one term of the joint density through the kernels' `parts` mask."""

    def __init__(self, owner: "MixedDensityEstimator", part: int):
        super().__init__()
        self.__dict__["_owner"] = owner        # (not a submodule: the owner holds the parameters)
        self.part = part

    @property
    def net(self):
        return self._owner.net

    def log_prob(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        """Discrete view: input (..., V) raw values, condition theta.  Continuous view: input (..., 1), condition
        (..., V + C) = [raw values, theta] as the reference's combined condition."""
        o = self._owner
        h = o.net.hyper
        if self.part == 1:
            x = torch.cat([torch.ones_like(input[..., :1]), input], -1)
            return o._log_prob_parts(x, condition, 1)
        x = torch.cat([input, condition[..., : h.V]], -1)
        return o._log_prob_parts(x, condition[..., h.V:], 2)

    def loss(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        return -self.log_prob(input.unsqueeze(0), condition)[0]

    def sample(self, sample_shape: torch.Size, condition: Tensor, **kwargs) -> Tensor:
        full = self._owner.sample(sample_shape, condition)
        return full[..., 1:] if self.part == 1 else full[..., :1]


class MixedDensityEstimator(ConditionalDensityEstimator):
    r"""p(x | theta) for x = [continuous, V categorical columns]: log_prob / loss / sample on the gfx950 kernels."""

    def __init__(self, net: MNLENet, input_shape: torch.Size, condition_shape: torch.Size,
                 embedding_net: Optional[nn.Module] = None, log_transform_input: bool = False) -> None:
        super().__init__(net, input_shape=input_shape, condition_shape=condition_shape)
        self.condition_embedding = embedding_net if embedding_net is not None else nn.Identity()
        self.log_transform_input = log_transform_input
        self.__dict__["discrete_net"] = _PartView(self, 1)
        self.__dict__["continuous_net"] = _PartView(self, 2)
        self._register_state_dict_hook(MixedDensityEstimator._emit_reference_keys)
        self._register_load_state_dict_pre_hook(self._accept_reference_keys, with_module=False)

    @property
    def embedding_net(self) -> Optional[nn.Module]:
        return None if isinstance(self.condition_embedding, nn.Identity) else self.condition_embedding

    def forward(self, input: Tensor):
        raise NotImplementedError("The forward method is not implemented for mixed neural density estimation, use "
                                  "'.sample(...)' to generate samples though a forward pass.")

    # -- checkpoints in the reference's key names ------------------------------------------------------
    @staticmethod
    def _emit_reference_keys(module, state_dict, prefix, local_metadata):
        net = module.net
        h = net.hyper
        flat = state_dict.pop(prefix + "net.flat_params")
        zst = state_dict.pop(prefix + "net.zstats")
        out = OrderedDict()
        for key, off, n, shape in net._slices():
            out[prefix + key] = flat[off: off + n].reshape(shape).clone()
        for t in range(h.num_transforms):      # the shared context layer is registered once per use in the reference
            sp = prefix + (f"continuous_net.net._transform._transforms.{t + int(h.z_score_x)}.transform_net."
                           "spline_predictor.")
            for j in range(1, h.context_layers):
                out[sp + f"{2 + 2 * j}.weight"] = out[sp + "2.weight"]
                out[sp + f"{2 + 2 * j}.bias"] = out[sp + "2.bias"]
        d = prefix + "discrete_net.net."
        out[d + "initial_layer.mask"] = h.made_mask("initial")
        out[d + "initial_layer.degrees"] = h.hidden_degrees()
        for b in range(h.discrete_blocks):
            for j in (0, 1):
                out[d + f"blocks.{b}.linear_layers.{j}.mask"] = h.made_mask("hidden")
                out[d + f"blocks.{b}.linear_layers.{j}.degrees"] = h.hidden_degrees()
        out[d + "final_layer.mask"] = h.made_mask("final")
        out[d + "final_layer.degrees"] = torch.repeat_interleave(torch.arange(1, h.F + 1), h.Kmax)
        cat_mask = torch.zeros(h.V, h.Kmax)
        for i, c in enumerate(h.num_categories):
            cat_mask[i, :c] = 1
        out[d + "mask"] = cat_mask
        out[d + "values_lookup"] = zst[2 + 2 * h.C:].reshape(h.V, MAX_CATEGORIES)[:, : h.Kmax].clone()
        if h.z_score_x:
            t = prefix + "continuous_net.net._transform._transforms.0."
            out[t + "_shift"] = zst[0:1].clone()
            out[t + "_scale"] = zst[1:2].clone()
        for t in range(h.num_transforms):      # the coupling transforms' index buffers at x_numel == 1: dummy mask [1]
            tp = prefix + f"continuous_net.net._transform._transforms.{t + int(h.z_score_x)}."
            out[tp + "identity_features"] = torch.zeros(0, dtype=torch.long)
            out[tp + "transform_features"] = torch.zeros(1, dtype=torch.long)
        out[prefix + "condition_embedding.0._mean"] = zst[2: 2 + h.C].clone()
        out[prefix + "condition_embedding.0._std"] = zst[2 + h.C: 2 + 2 * h.C].clone()
        for k, v in state_dict.items():
            out[k] = v
        state_dict.clear()
        state_dict.update(out)
        return state_dict

    def _accept_reference_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                               error_msgs):
        if prefix + "net.flat_params" in state_dict:
            return
        net, h = self.net, self.net.hyper
        if prefix + "discrete_net.net.initial_layer.weight" not in state_dict:
            return
        flat = net.flat_params.detach().clone()
        zst = net.zstats.detach().clone()
        try:
            for key, off, n, shape in net._slices():
                src = state_dict.pop(prefix + key)
                if tuple(src.shape) != tuple(shape):
                    raise ValueError(f"{key}: expected {shape}, got {tuple(src.shape)}")
                flat[off: off + n] = src.reshape(-1).to(flat)
            for k in [k for k in state_dict if k.startswith(prefix + "discrete_net.net.") and
                      (k.endswith(".mask") or k.endswith(".degrees")) and k != prefix + "discrete_net.net.mask"]:
                state_dict.pop(k)
            state_dict.pop(prefix + "discrete_net.net.mask", None)
            lk = state_dict.pop(prefix + "discrete_net.net.values_lookup", None)
            if lk is not None:
                zst[2 + 2 * h.C:].reshape(h.V, MAX_CATEGORIES)[:, : h.Kmax] = lk.to(zst)
            if h.z_score_x:
                t = prefix + "continuous_net.net._transform._transforms.0."
                zst[0] = state_dict.pop(t + "_shift").reshape(-1)[0]
                zst[1] = state_dict.pop(t + "_scale").reshape(-1)[0]
            m = state_dict.pop(prefix + "condition_embedding.0._mean", None)
            s = state_dict.pop(prefix + "condition_embedding.0._std", None)
            if m is not None:
                zst[2: 2 + h.C] = m.reshape(-1).expand(h.C).to(zst)
                zst[2 + h.C: 2 + 2 * h.C] = s.reshape(-1).expand(h.C).to(zst)
            # the reference registers the shared context layer of a transform once per use, and the theta
            # standardisation a second time inside the categorical net: duplicates of what was read above
            for k in [k for k in state_dict if ".spline_predictor." in k or "discrete_net.net.embedding_net." in k
                      or k.endswith(".identity_features") or k.endswith(".transform_features")]:
                state_dict.pop(k)
        except (KeyError, ValueError) as e:
            error_msgs.append(f"MixedDensityEstimator: cannot read the reference-keyed checkpoint: {e!r}")
            return
        state_dict[prefix + "net.flat_params"] = flat
        state_dict[prefix + "net.zstats"] = zst
        net.__dict__.pop("_packed_cache", None)

    # -- kernels ---------------------------------------------------------------------------------------
    def _embed(self, condition: Tensor) -> Tensor:
        return self.condition_embedding(condition)

    def _rows(self, input: Tensor, condition: Tensor):
        """Paired (n, 1 + V) / (n, C) rows of the common (sample, batch) grid."""
        self._check_condition_shape(condition)
        self._check_input_shape(input)
        inp, cond, batch = self._broadcast_and_align(input, condition)
        S = inp.shape[0]
        x = inp.reshape(S * batch, -1).contiguous().float()
        c = self._embed(cond.reshape(S * batch, *self.condition_shape)).reshape(S * batch, -1).contiguous().float()
        return x, c, S, batch

    def _log_prob_parts(self, input: Tensor, condition: Tensor, parts: int) -> Tensor:
        x, c, S, batch = self._rows(input, condition)
        net = self.net
        dev = net.flat_params.device
        x, c = x.to(dev), c.to(dev)
        xc, idx, val = split_input(net, x, validate=bool(parts & 1))
        if parts == 3 and torch.is_grad_enabled() and (net.flat_params.requires_grad or c.requires_grad):
            lp = _MNLELogProbFn.apply(c, net.flat_params, net, xc, idx, val)
        else:
            with torch.no_grad():
                lp = mnle_log_prob_call(net, xc, idx, val, c.detach(), parts)
        return lp.reshape(S, batch).to(input.device)

    def log_prob(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        """(sample_dim, batch_dim); an input without a sample dimension counts as sample_dim = 1."""
        return self._log_prob_parts(input, condition, 3)

    def loss(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        return -self.log_prob(input.unsqueeze(0), condition)[0]

    def log_prob_iid_trials(self, x_o: Tensor, theta: Tensor) -> Optional[Tensor]:
        """sum_t log p(x_t | theta_j) per theta row in ONE pass over the (trial, theta) grid read in place (the hook
        of LikelihoodBasedPotential)."""
        if x_o.dim() != 2 or theta.dim() != 2:
            return None
        net = self.net
        dev = net.flat_params.device
        with torch.no_grad():
            xc, idx, val = split_input(net, x_o.to(dev).float())
            c = self._embed(theta.to(dev)).reshape(theta.shape[0], -1).contiguous().float()
            return mnle_trials_call(net, xc, idx, val, c)

    def sample_given(self, u: Tensor, noise: Tensor, condition: Tensor) -> Tensor:
        """x (n, 1 + V) for given uniforms u (n, V) and normal draws noise (n,); row i pairs with condition[i % rows]."""
        net = self.net
        dev = net.flat_params.device
        with torch.no_grad():
            c = self._embed(condition.to(dev)).reshape(condition.shape[0], -1).contiguous().float()
            idx, xc = mnle_sample_call(net, u.to(dev).contiguous().float(), noise.to(dev).contiguous().float(), c)
            vals = torch.gather(net.lookup, 1, idx.long().t()).t()
        return torch.cat([xc[:, None], vals], 1).to(condition.device)

    def sample(self, sample_shape: torch.Size, condition: Tensor, track_gradients: bool = False, **kwargs) -> Tensor:
        """(*sample_shape, batch_dim, 1 + V); rows sample-major so that the kernel's c[row % batch] pairs each draw."""
        self._check_condition_shape(condition)
        Bc = condition.shape[0]
        n = torch.Size(sample_shape).numel()
        dev = condition.device
        u = torch.rand(n * Bc, self.net.hyper.V, device=dev, dtype=torch.float32)
        noise = torch.randn(n * Bc, device=dev, dtype=torch.float32)
        return self.sample_given(u, noise, condition).reshape((*sample_shape, Bc, -1))
