"""sbi's default density estimator, the affine masked autoregressive flow (`maf`), on the MI355X HIP kernels.

``MAFFlow`` is the drop-in for sbi's ``NFlowsFlow(build_maf(...))`` (sbi/neural_nets/net_builders/flow.py:115-209):
T x [MaskedAffineAutoregressiveTransform (MADE conditioner, tanh, separate context layer, feed-forward blocks),
RandomPermutation], z-scoring of both sides, standard-normal base.  The estimator surface is inherited from
``NSFFlow``; the arithmetic runs in ``libsbi_amd_nsf.so`` through include/sbi_amd_maf_affine.h.  No PyTorch / CPU
fallback.

Parameters live in ONE flat fp32 ``nn.Parameter`` in nflows' order (initial_layer, context_layer, blocks.b.linear,
final_layer per transform; the (2D, H) final layer in nflows' interleaved row order: row 2d the unconstrained scale
of dim d, row 2d+1 its shift).  The static MADE degree masks are folded into the packed image and into the weight
gradients by the kernels.  nflows 0.14 could not be imported where this was written: the parity with it is unpinned
(the reading is tests/maf_affine_oracle.py), and ``epsilon`` travels in the config struct.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.maf_flow import MAFNet
from sbi_amd.neural_nets.estimators.nsf_flow import NSFFlow


@dataclass(frozen=True)
class MAFAffineHyper:
    """Hyper-parameters ``build_maf`` bakes into the flow (flow.py:115-131)."""

    D: int
    C: int
    hidden_features: int = 50
    num_transforms: int = 5
    num_blocks: int = 2
    epsilon: float = 1e-3    # nflows: scale = softplus(unconstrained_scale) + 1e-3

    def c_config(self) -> _lib.MAFAffineConfigC:
        return _lib.MAFAffineConfigC(self.D, self.C, self.hidden_features, self.num_transforms, self.num_blocks,
                                     self.epsilon)

    def layer_entries(self) -> List[Tuple[str, Tuple[int, ...], int]]:
        """(nflows sub-key, shape, mask kind) in flat order for one transform (kinds as csrc/maf_kernel.h maf_mask)."""
        H, D, C = self.hidden_features, self.D, self.C
        pre = "autoregressive_net."
        out = [(pre + "initial_layer.weight", (H, D), 0), (pre + "initial_layer.bias", (H,), -1),
               (pre + "context_layer.weight", (H, C), 1), (pre + "context_layer.bias", (H,), -1)]
        for b in range(self.num_blocks):
            out += [(pre + f"blocks.{b}.linear.weight", (H, H), 2), (pre + f"blocks.{b}.linear.bias", (H,), -1)]
        out += [(pre + "final_layer.weight", (2 * D, H), 3), (pre + "final_layer.bias", (2 * D,), -1)]
        return out

    def layer_params(self) -> int:
        return sum(int(np.prod(s)) for _, s, _ in self.layer_entries())

    def param_count(self) -> int:
        return self.num_transforms * self.layer_params()

    # -- MADE degrees / masks (nflows transforms/made.py, random_mask=False, output_multiplier=2) -------------
    def hidden_degrees(self) -> Tensor:
        mx, mn = max(1, self.D - 1), min(1, self.D - 1)
        return torch.arange(self.hidden_features) % mx + mn

    def output_degrees(self) -> Tensor:
        return torch.repeat_interleave(torch.arange(1, self.D + 1), 2)

    def mask(self, kind: int) -> Optional[Tensor]:
        hd = self.hidden_degrees()
        if kind == 0:
            return (hd[:, None] >= torch.arange(1, self.D + 1)[None, :]).float()
        if kind == 2:
            return (hd[:, None] >= hd[None, :]).float()
        if kind == 3:
            return (self.output_degrees()[:, None] > hd[None, :]).float()
        return None

    def final_tile_rows(self) -> Tensor:
        """nflows row of the final layer held by row r of the packed image's two 16-row tiles (-1: a zero row):
        image row 16 * tile + d  <-  nflows row 2 d + tile (tile 0 scale logits, tile 1 shifts)."""
        rows = torch.full((32,), -1, dtype=torch.long)
        for tile in range(2):
            for d in range(self.D):
                rows[16 * tile + d] = 2 * d + tile
        return rows


class MAFAffineNet(MAFNet):
    """Parameter / buffer holder in the role of nflows' ``Flow`` for the affine MAF (flat_params, zstats, perms and
    the nflows-keyed state-dict exchange are MAFNet's, on this hyper's layer list)."""

    supports_atomic = False    # one-call training pass only

    def __init__(self, hyper: MAFAffineHyper, zstats: Tensor, z_score_theta: bool, z_score_x: bool,
                 dtype: torch.dtype = torch.float32):
        super().__init__(hyper, zstats, z_score_theta, z_score_x, dtype=dtype)
        # checkpoints are interchangeable with the reference's: `state_dict()` speaks the keys of a real
        # NFlowsFlow(build_maf(...)) (weights, `mask` / `degrees` buffers, permutations, z-scoring) and
        # `load_state_dict()` accepts them as well as the native form (flat_params, zstats, perms)
        self._register_state_dict_hook(MAFAffineNet._emit_nflows_keys)
        self._register_load_state_dict_pre_hook(self._accept_nflows_keys, with_module=False)

    _NATIVE_KEYS = ("flat_params", "zstats", "perms")

    @staticmethod
    def _emit_nflows_keys(module, state_dict, prefix, local_metadata):
        for k in MAFAffineNet._NATIVE_KEYS:
            state_dict.pop(prefix + k, None)
        for k, v in module.nflows_state_dict(prefix=prefix).items():
            state_dict[k] = v
        return state_dict

    def _accept_nflows_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                            error_msgs):
        if prefix + "flat_params" in state_dict:
            return      # native form
        mine = [k for k in state_dict if k.startswith(prefix + "_transform.") or
                k.startswith(prefix + "_embedding_net.0._")]
        if not mine:
            return      # nothing of ours: let the regular missing-key report speak
        try:
            self.load_nflows_state_dict(state_dict, prefix=prefix)
        except (KeyError, ValueError) as e:
            error_msgs.append(f"MAFAffineNet: cannot read the nflows-keyed checkpoint: {e!r}")
            return
        for k in mine:
            del state_dict[k]
        for k in MAFAffineNet._NATIVE_KEYS:
            state_dict[prefix + k] = getattr(self, k).detach().clone()

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """nflows' construction order per transform: MaskedLinear initial, nn.Linear context, block linears, final
        MaskedLinear -- each the default nn.Linear init -- then RandomPermutation's torch.randperm."""
        h = self.hyper
        H, D, C = h.hidden_features, h.D, h.C
        chunks: List[Tensor] = []
        for t in range(h.num_transforms):
            mods = [nn.Linear(D, H), nn.Linear(C, H)] + [nn.Linear(H, H) for _ in range(h.num_blocks)] + \
                   [nn.Linear(H, 2 * D)]
            for m in mods:
                chunks += [m.weight.detach().reshape(-1), m.bias.detach().reshape(-1)]
            self.perms[t] = torch.randperm(D).to(torch.int32)
        flat = torch.cat(chunks)
        assert flat.numel() == self.flat_params.numel()
        self.flat_params.copy_(flat)

    def _mask_buffers(self, t: int):
        h = self.hyper
        first = 1 if self.z_score_theta else 0
        pre = f"_transform._transforms.{first + 2 * t}.autoregressive_net."
        hd = h.hidden_degrees()
        yield pre + "initial_layer.", h.mask(0), hd.clone()
        for b in range(h.num_blocks):
            yield pre + f"blocks.{b}.linear.", h.mask(2), hd.clone()
        yield pre + "final_layer.", h.mask(3), h.output_degrees()

    def train_workspace_floats(self, n: int) -> int:
        need = _lib.load().sbi_amd_maf_affine_train_workspace_floats(self.hyper.c_config(), n)
        if need < 0:
            _lib.check(int(need), "maf_affine_train_workspace_floats")
        return int(need)

    def plan_waves(self, n: int, trials: bool = False) -> int:
        """Waves per workgroup (16 rows each) log_prob, sample and the training pass (``trials``: the iid-trials
        kernel, ``n`` thetas) launch with for ``n`` rows; a host-side answer, raises where those calls would refuse
        the configuration."""
        nw = _lib.load().sbi_amd_maf_affine_plan_waves(self.hyper.c_config(), n, 1 if trials else 0)
        if nw < 0:
            _lib.check(int(nw), "maf_affine_plan_waves")
        return int(nw)

    def train_pass(self, theta: Tensor, x: Tensor, row_weight: Optional[Tensor], uniform_weight: float,
                   grad_out: Tensor, workspace: Optional[Tensor] = None, want_grad_theta: bool = False,
                   grad_x_out: Optional[Tensor] = None):
        return maf_affine_loss_fwd_bwd(self, theta, x, row_weight, uniform_weight, grad_out, want_grad_theta,
                                       workspace, grad_x_out=grad_x_out)


# --------------------------------------------------------------------- kernel calls
def maf_affine_packed_weights(net: MAFAffineNet) -> Tensor:
    fp = net.flat_params
    key = (fp.data_ptr(), fp._version, str(fp.device), net.perms._version)
    cache = net.__dict__.get("_packed_cache")
    if cache is not None and cache[0] == key:
        return cache[1]
    dev = _lib.require_device(fp)
    lib = _lib.load()
    cfg = net.hyper.c_config()
    n = lib.sbi_amd_maf_affine_packed_floats(cfg)
    if n < 0:
        _lib.check(int(n), "maf_affine_packed_floats")
    packed = cache[1] if (cache is not None and cache[1].device == dev and cache[1].numel() == n) else \
        torch.zeros(int(n), dtype=torch.float32, device=dev)
    perms = net.perms.contiguous()
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_maf_affine_pack(cfg, _lib.ptr(fp), perms.data_ptr(), _lib.ptr(packed),
                                         _lib.current_stream(dev))
    _lib.check(rc, "maf_affine_pack")
    net.__dict__["_packed_cache"] = (key, packed)
    return packed


def maf_affine_log_prob_call(net: MAFAffineNet, theta: Tensor, x: Tensor, want_noise: bool):
    dev = _lib.require_device(theta, x, net.flat_params, net.zstats)
    lib = _lib.load()
    n = theta.shape[0]
    logp = torch.empty(n, dtype=torch.float32, device=dev)
    noise = torch.empty_like(theta) if want_noise else None
    if n == 0:
        return logp, noise
    packed = maf_affine_packed_weights(net)
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_maf_affine_log_prob(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                             _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(logp),
                                             _lib.ptr(noise), _lib.current_stream(dev))
    _lib.check(rc, "maf_affine_log_prob")
    return logp, noise


def maf_affine_sample_call(net: MAFAffineNet, noise: Tensor, x: Tensor, want_ld: bool):
    dev = _lib.require_device(noise, x, net.flat_params, net.zstats)
    lib = _lib.load()
    n = noise.shape[0]
    theta = torch.empty_like(noise)
    ld = torch.empty(n, dtype=torch.float32, device=dev) if want_ld else None
    if n == 0:
        return theta, ld
    packed = maf_affine_packed_weights(net)
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_maf_affine_sample(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                           _lib.ptr(noise), _lib.ptr(x), n, x.shape[0], _lib.ptr(theta), _lib.ptr(ld),
                                           _lib.current_stream(dev))
    _lib.check(rc, "maf_affine_sample")
    return theta, ld


def maf_affine_trials_call(net: MAFAffineNet, x_trials: Tensor, theta: Tensor) -> Tensor:
    """out[c] = sum over the trials (rows of x_trials, the flow inputs) of log q(x_i | theta_c), in trial order."""
    dev = _lib.require_device(x_trials, theta, net.flat_params, net.zstats)
    out = torch.empty(theta.shape[0], dtype=torch.float32, device=dev)
    if theta.shape[0] == 0:
        return out
    packed = maf_affine_packed_weights(net)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_maf_affine_log_prob_trials(
            net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(x_trials), x_trials.shape[0],
            _lib.ptr(theta), theta.shape[0], _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "maf_affine_log_prob_trials")
    return out


def maf_affine_loss_fwd_bwd(net: MAFAffineNet, theta: Tensor, x: Tensor, row_weight: Optional[Tensor],
                            uniform_weight: float, grad_out: Tensor, want_grad_theta: bool = False,
                            workspace: Optional[Tensor] = None, grad_x_out: Optional[Tensor] = None):
    """Fused training pass: (per-row loss, grad_theta | None); fills grad_out (P,) and, if given, grad_x_out (n, C)
    with d loss / d x (one condition row per theta row)."""
    dev = _lib.require_device(theta, x, net.flat_params, net.zstats, grad_out, row_weight, grad_x_out)
    if grad_x_out is not None and (x.shape[0] != theta.shape[0] or tuple(grad_x_out.shape) != tuple(x.shape)
                                   or grad_x_out.dtype != torch.float32 or not grad_x_out.is_contiguous()):
        raise ValueError("grad_x_out must be a contiguous fp32 (n, C) tensor, with one condition row per theta row")
    lib = _lib.load()
    n = theta.shape[0]
    need = net.train_workspace_floats(n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    gtheta = torch.empty_like(theta) if want_grad_theta else None
    packed = maf_affine_packed_weights(net)
    with torch.cuda.device(dev):
        rc = lib.sbi_amd_maf_affine_loss_fwd_bwd(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats),
                                                 _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(row_weight),
                                                 float(uniform_weight), _lib.ptr(loss), _lib.ptr(grad_out),
                                                 _lib.ptr(gtheta), _lib.ptr(grad_x_out), _lib.ptr(workspace),
                                                 _lib.current_stream(dev))
    _lib.check(rc, "maf_affine_loss_fwd_bwd")
    return loss, gtheta


class _MAFAffineLogProbFn(torch.autograd.Function):
    """Autograd bridge: forward = the log_prob kernel; backward = the fused training pass with row weights
    -dL/dlogp (it re-runs the forward with the per-transform stash: the training pass is one call)."""

    @staticmethod
    def forward(ctx, theta: Tensor, x: Tensor, flat_params: Tensor, net: MAFAffineNet):
        ctx.net = net
        ctx.version = net.flat_params._version
        ctx.save_for_backward(theta, x)
        logp, _ = maf_affine_log_prob_call(net, theta, x, want_noise=False)
        return logp

    @staticmethod
    def backward(ctx, grad_logp: Tensor):
        theta, x = ctx.saved_tensors
        net: MAFAffineNet = ctx.net
        if net.flat_params._version != ctx.version:
            raise RuntimeError("maf parameters were modified in place between log_prob() and backward().")
        gx = None
        if ctx.needs_input_grad[1]:      # NLE: theta is the condition (rejection sampling and MAP ascend on it)
            if x.shape[0] != theta.shape[0]:
                raise RuntimeError("gradient wrt the condition needs one condition row per theta row")
            gx = torch.empty_like(x)
        gparams = torch.empty_like(net.flat_params)
        w = (-grad_logp).contiguous().to(torch.float32)
        _, gtheta = maf_affine_loss_fwd_bwd(net, theta, x, w, 0.0, gparams, want_grad_theta=ctx.needs_input_grad[0],
                                            grad_x_out=gx)
        return gtheta, gx, (gparams if ctx.needs_input_grad[2] else None), None


class MAFFlow(NSFFlow):
    r"""Affine masked autoregressive flow :math:`p(\theta|x)` evaluated by the gfx950 kernels."""

    def __init__(self, net: MAFAffineNet, input_shape: torch.Size, condition_shape: torch.Size,
                 embedding_net: Optional[nn.Module] = None) -> None:
        super().__init__(net, input_shape=input_shape, condition_shape=condition_shape, embedding_net=embedding_net)
        if embedding_net is not None and any(p.requires_grad for p in embedding_net.parameters()):
            raise NotImplementedError("sbi_amd maf: trainable embedding nets are not supported (frozen / "
                                      "parameter-free ones are applied in front of the kernels); NSFConfig trains "
                                      "an embedding net end to end")

    def _raw_log_prob(self, net, theta: Tensor, x: Tensor, want_noise: bool):
        return maf_affine_log_prob_call(net, theta, x, want_noise)

    def _raw_sample(self, net, noise: Tensor, x: Tensor, want_ld: bool):
        return maf_affine_sample_call(net, noise, x, want_ld)

    def _raw_autograd(self, net, theta: Tensor, x: Tensor, flat: Tensor) -> Tensor:
        return _MAFAffineLogProbFn.apply(theta, x, flat, net)

    def log_prob_iid_trials(self, input: Tensor, condition: Tensor) -> Optional[Tensor]:
        """sum_i log q(input_i | condition_c) per condition row: one pass of sbi_amd_maf_affine_log_prob_trials."""
        with torch.no_grad():
            x_trials = input.reshape(-1, self.input_shape[0]).contiguous().float()
            theta = self._embed(condition).reshape(-1, self._cdim).contiguous().float()
            net = self._kernel_net()
            dev = net.flat_params.device
            out = maf_affine_trials_call(net, x_trials.to(dev), theta.to(dev))
        return out.to(condition.device)
