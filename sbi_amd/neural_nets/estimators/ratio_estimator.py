"""The ratio estimator of NRE on the HIP kernels (csrc/nre.hip).

API mirror of sbi's ``RatioEstimator`` (sbi/neural_nets/ratio_estimators.py) holding the network of
``build_resnet_classifier`` (sbi/neural_nets/net_builders/classifier.py:172-235): z-scored theta and x, concatenated,
through nflows' ``ResidualNet(in = D + C, out = 1, hidden H, NB blocks, relu)``.  The weights live in ONE flat fp32
buffer in nflows' parameter order (``RatioNet.flat_params``) next to a z-score buffer (``zstats``: theta mean, theta
std, x mean, x std); ``state_dict()`` speaks sbi's key names and ``load_state_dict()`` takes them.  Every evaluation --
forward, autograd with respect to theta and the parameters, the iid-trials sum -- is a kernel launch; a CPU-resident
estimator stages its inputs and weights through the current ROCm device.
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.base import ConditionalEstimator


class RatioHyper:
    """Shape of the classifier: theta features D, x features C, hidden H, residual blocks NB."""

    def __init__(self, D: int, C: int, hidden_features: int = 50, num_blocks: int = 2):
        self.D, self.C, self.H, self.NB = int(D), int(C), int(hidden_features), int(num_blocks)

    def c_config(self) -> _lib.NREConfigC:
        return _lib.NREConfigC(self.D, self.C, self.H, self.NB)

    def entries(self) -> List[Tuple[str, Tuple[int, ...]]]:
        """(nflows key, shape) in the order of the flat buffer."""
        H, NB = self.H, self.NB
        out = [("initial_layer.weight", (H, self.D + self.C)), ("initial_layer.bias", (H,))]
        for b in range(NB):
            for i in range(2):
                out += [(f"blocks.{b}.linear_layers.{i}.weight", (H, H)), (f"blocks.{b}.linear_layers.{i}.bias", (H,))]
        out += [("final_layer.weight", (1, H)), ("final_layer.bias", (1,))]
        return out

    def param_count(self) -> int:
        return sum(int(torch.Size(s).numel()) for _, s in self.entries())

    def offsets(self) -> Dict[str, int]:
        off, res = 0, {}
        for k, s in self.entries():
            res[k] = off
            off += int(torch.Size(s).numel())
        return res


class RatioNet(nn.Module):
    """The kernels' view of the classifier: `flat_params` (P) and `zstats` (2 D + 2 C)."""

    def __init__(self, hyper: RatioHyper, zstats: Tensor):
        super().__init__()
        self.hyper = hyper
        self.flat_params = nn.Parameter(torch.zeros(hyper.param_count()))
        self.register_buffer("zstats", zstats.detach().to(torch.float32).clone())
        self._native_state_dict = False
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """nn.Linear's default initialisation in nflows' construction order (initial layer, blocks, final layer),
        with the last linear of every block drawn from U(-1e-3, 1e-3) as nflows' ResidualBlock does."""
        views = self.views(self.flat_params.data)
        H, NB = self.hyper.H, self.hyper.NB

        def linear(prefix: str):
            w, b = views[prefix + ".weight"], views[prefix + ".bias"]
            nn.init.kaiming_uniform_(w, a=5 ** 0.5)
            bound = 1 / w.shape[1] ** 0.5
            nn.init.uniform_(b, -bound, bound)

        linear("initial_layer")
        for blk in range(NB):
            linear(f"blocks.{blk}.linear_layers.0")
            linear(f"blocks.{blk}.linear_layers.1")
            nn.init.uniform_(views[f"blocks.{blk}.linear_layers.1.weight"], -1e-3, 1e-3)
            nn.init.uniform_(views[f"blocks.{blk}.linear_layers.1.bias"], -1e-3, 1e-3)
        linear("final_layer")
        del H

    def views(self, flat: Tensor) -> "OrderedDict[str, Tensor]":
        out, off = OrderedDict(), 0
        for k, s in self.hyper.entries():
            n = int(torch.Size(s).numel())
            out[k] = flat[off : off + n].view(s)
            off += n
        return out

    def native_state_dict(self) -> "OrderedDict[str, Tensor]":
        self._native_state_dict = True
        try:
            return self.state_dict()
        finally:
            self._native_state_dict = False

    def packed(self, dev: torch.device, flat: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """(packed image, zstats) on `dev`, re-packed only when the weights changed since the last call."""
        fp = self.flat_params if flat is None else flat
        key = (fp.data_ptr(), fp._version, self.zstats.data_ptr(), self.zstats._version, str(dev))
        held = self.__dict__.get("_packed_cache")
        if held is not None and held[0] == key:
            return held[1], held[2]
        lib = _lib.load()
        cfg = self.hyper.c_config()
        n = lib.sbi_amd_nre_packed_floats(cfg)
        if n < 0:
            _lib.check(int(n), "nre_packed_floats")
        flat_d = fp.detach().to(dev, torch.float32).contiguous()
        zs = self.zstats.detach().to(dev, torch.float32).contiguous()
        pk = torch.empty(int(n), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sbi_amd_nre_pack(cfg, _lib.ptr(flat_d), _lib.ptr(pk), _lib.current_stream(dev)), "nre_pack")
        self.__dict__["_packed_cache"] = (key, pk, zs)
        return pk, zs

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_packed_cache", None)
        return state


def _device_of(*ts: Tensor) -> torch.device:
    for t in ts:
        if t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("sbi_amd: the NRE hot path runs only on a ROCm device (MI355X) and none is visible. There is "
                           "deliberately no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


def _kernel_log_ratio(net: RatioNet, theta: Tensor, x: Tensor, x_rows: int, dev: torch.device) -> Tensor:
    lib = _lib.load()
    pk, zs = net.packed(dev)
    th = theta.detach().to(dev, torch.float32).contiguous()
    xx = x.detach().to(dev, torch.float32).contiguous()
    n = th.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_nre_log_ratio(net.hyper.c_config(), _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(th), _lib.ptr(xx),
                                       n, int(x_rows), _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "nre_log_ratio")
    return out


class _NRELogRatioFn(torch.autograd.Function):
    """log r(theta_r, x_r) with gradients with respect to theta and the flat parameters through the training kernels
    (forward with stash, backward from the upstream gradient as the per-pair weights)."""

    @staticmethod
    def forward(ctx, theta: Tensor, x: Tensor, flat: Tensor, net: RatioNet, x_rows: int):
        dev = _device_of(theta, flat)
        lib = _lib.load()
        cfg = net.hyper.c_config()
        pk, zs = net.packed(dev, flat)
        th = theta.detach().to(dev, torch.float32).contiguous()
        xx = x.detach().to(dev, torch.float32).contiguous()
        n = th.shape[0]
        ws = torch.empty(int(lib.sbi_amd_nre_train_workspace_floats(cfg, max(n, 1))), dtype=torch.float32, device=dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n > 0:
            with torch.cuda.device(dev):
                rc = lib.sbi_amd_nre_train_forward(cfg, _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(th), _lib.ptr(xx), n,
                                                   int(x_rows), _lib.ptr(out), _lib.ptr(ws), _lib.current_stream(dev))
            _lib.check(rc, "nre_train_forward")
        ctx.state = (net, pk, zs, ws, n, dev, theta.device, flat.device)
        return out.to(theta.device)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        net, pk, zs, ws, n, dev, th_dev, fl_dev = ctx.state
        lib = _lib.load()
        w = grad_out.detach().to(dev, torch.float32).contiguous()
        g = torch.empty(net.hyper.param_count(), dtype=torch.float32, device=dev)
        gth = torch.empty(n, net.hyper.D, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        if n > 0:
            with torch.cuda.device(dev):
                rc = lib.sbi_amd_nre_train_backward(net.hyper.c_config(), _lib.ptr(pk), _lib.ptr(zs), n, _lib.ptr(w),
                                                    _lib.ptr(g), _lib.ptr(gth), _lib.ptr(ws),
                                                    _lib.current_stream(dev))
            _lib.check(rc, "nre_train_backward")
        else:
            g.zero_()
        ctx.state = None
        return (gth.to(th_dev) if gth is not None else None, None,
                g.to(fl_dev) if ctx.needs_input_grad[2] else None, None, None)


class RatioEstimator(ConditionalEstimator):
    """sbi's ``RatioEstimator`` (ratio_estimators.py) for the ResNet classifier: ``theta_shape``, ``x_shape``,
    ``combine_theta_and_x``, ``unnormalized_log_ratio``, ``forward``; theta and x must agree on their batch prefix."""

    def __init__(self, net: RatioNet, theta_shape, x_shape, z_score_theta: bool = True, z_score_x: bool = True):
        super().__init__(input_shape=theta_shape, condition_shape=x_shape)
        self.net = net
        self._z_theta, self._z_x = bool(z_score_theta), bool(z_score_x)
        self._register_state_dict_hook(RatioEstimator._emit_sbi_keys)
        self._register_load_state_dict_pre_hook(self._accept_sbi_keys, with_module=False)

    theta_shape = property(lambda self: self.input_shape)
    x_shape = property(lambda self: self.condition_shape)

    # -- state dict in sbi's key names -------------------------------------------------------------------------
    def sbi_state_dict(self, prefix: str = "") -> "OrderedDict[str, Tensor]":
        h = self.net.hyper
        out = OrderedDict()
        for k, v in self.net.views(self.net.flat_params.detach()).items():
            out[prefix + "net." + k] = v.clone()
        zs = self.net.zstats.detach()
        D, C = h.D, h.C
        if self._z_theta:
            out[prefix + "embedding_net_theta.0._mean"] = zs[:D].clone()
            out[prefix + "embedding_net_theta.0._std"] = zs[D : 2 * D].clone()
        if self._z_x:
            out[prefix + "embedding_net_x.0._mean"] = zs[2 * D : 2 * D + C].clone()
            out[prefix + "embedding_net_x.0._std"] = zs[2 * D + C :].clone()
        return out

    @staticmethod
    def _emit_sbi_keys(module, state_dict, prefix, local_metadata):
        if getattr(module.net, "_native_state_dict", False):
            return state_dict
        for k in ("net.flat_params", "net.zstats"):
            state_dict.pop(prefix + k, None)
        state_dict.update(module.sbi_state_dict(prefix))
        return state_dict

    def _accept_sbi_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        if prefix + "net.flat_params" in state_dict:
            return
        h = self.net.hyper
        flat = self.net.flat_params.detach().clone()
        zst = self.net.zstats.detach().clone()
        views = self.net.views(flat)
        used = []
        try:
            for k, v in views.items():
                src = state_dict[prefix + "net." + k]
                v.copy_(src.reshape(v.shape))
                used.append(prefix + "net." + k)
        except KeyError:
            return      # not ours: the regular missing-key report speaks
        D, C = h.D, h.C
        for name, lo, n in (("embedding_net_theta", 0, D), ("embedding_net_x", 2 * D, C)):
            mk, sk = prefix + name + ".0._mean", prefix + name + ".0._std"
            if mk in state_dict:
                zst[lo : lo + n] = state_dict[mk].reshape(-1).expand(n)
                zst[lo + n : lo + 2 * n] = state_dict[sk].reshape(-1).expand(n)
                used += [mk, sk]
        for k in used:
            del state_dict[k]
        state_dict[prefix + "net.flat_params"] = flat
        state_dict[prefix + "net.zstats"] = zst

    # -- sbi's surface -------------------------------------------------------------------------------------------
    def _get_shape_prefix(self, theta: Tensor, x: Tensor) -> torch.Size:
        theta_prefix = theta.shape[: theta.dim() - len(self.theta_shape)]
        x_prefix = x.shape[: x.dim() - len(self.x_shape)]
        if theta_prefix != x_prefix:
            raise ValueError(f"{tuple(theta_prefix)=} != {tuple(x_prefix)=}. Make them agree, since we do not "
                             "broadcast for you.")
        return theta_prefix

    def _flat_pairs(self, theta: Tensor, x: Tensor) -> Tuple[Tensor, Tensor, torch.Size]:
        self._check_input_shape(theta)
        self._check_condition_shape(x)
        prefix = self._get_shape_prefix(theta, x)
        return theta.reshape(-1, self.net.hyper.D), x.reshape(-1, self.net.hyper.C), prefix

    def combine_theta_and_x(self, theta: Tensor, x: Tensor) -> Tensor:
        """[z_theta ; z_x] of every pair, shape (*batch_shape, D + C) (the classifier's input)."""
        th, xx, prefix = self._flat_pairs(theta, x)
        h, zs = self.net.hyper, self.net.zstats.to(th.device)
        zt = (th - zs[: h.D]) / zs[h.D : 2 * h.D]
        zx = (xx - zs[2 * h.D : 2 * h.D + h.C]) / zs[2 * h.D + h.C :]
        return torch.cat([zt, zx], dim=-1).reshape(*prefix, -1)

    def unnormalized_log_ratio(self, theta: Tensor, x: Tensor) -> Tensor:
        """log r(theta, x) per pair, shape (*batch_shape)."""
        th, xx, prefix = self._flat_pairs(theta, x)
        return self._log_ratio_rows(th, xx, th.shape[0]).reshape(prefix)

    def forward(self, *args, **kwargs) -> Tensor:
        return self.unnormalized_log_ratio(*args, **kwargs)

    def loss(self, input: Tensor, condition: Tensor, **kwargs) -> Tensor:
        raise NotImplementedError("The ratio estimator has no loss of its own: the NRE trainers define it.")

    def _log_ratio_rows(self, th: Tensor, xx: Tensor, x_rows: int) -> Tensor:
        """Rows r of `th` against xx[r % x_rows]; autograd through the kernels when a gradient is asked for."""
        flat = self.net.flat_params
        if torch.is_grad_enabled() and (th.requires_grad or flat.requires_grad):
            return _NRELogRatioFn.apply(th, xx, flat, self.net, x_rows)
        dev = _device_of(th, flat)
        return _kernel_log_ratio(self.net, th, xx, x_rows, dev).to(th.device)

    def log_ratio_one_x(self, theta: Tensor, x_o: Tensor) -> Tensor:
        """log r(theta_r, x_o) for a single x_o row (the folded kernel path), no gradient."""
        th = theta.reshape(-1, self.net.hyper.D)
        with torch.no_grad():
            return _kernel_log_ratio(self.net, th, x_o.reshape(1, -1), 1, _device_of(th, self.net.flat_params))

    def log_ratio_iid_trials(self, x_trials: Tensor, theta: Tensor) -> Tensor:
        """sum_i log r(theta_c, x_i) per theta row, one kernel pass with no pairs materialised (no gradient)."""
        h = self.net.hyper
        th = theta.reshape(-1, h.D)
        dev = _device_of(th, self.net.flat_params)
        lib = _lib.load()
        pk, zs = self.net.packed(dev)
        xt = x_trials.detach().reshape(-1, h.C).to(dev, torch.float32).contiguous()
        thd = th.detach().to(dev, torch.float32).contiguous()
        T, N = xt.shape[0], thd.shape[0]
        out = torch.empty(N, dtype=torch.float32, device=dev)
        if N == 0:
            return out.to(theta.device)
        ws = torch.empty(T * N, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = lib.sbi_amd_nre_log_ratio_trials(h.c_config(), _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(xt), T,
                                                  _lib.ptr(thd), N, _lib.ptr(out), None, _lib.ptr(ws),
                                                  _lib.current_stream(dev))
        _lib.check(rc, "nre_log_ratio_trials")
        return out.to(theta.device)
