"""``LRUEmbedding`` -- sbi/neural_nets/embedding_nets/lru.py (Orvieto et al. 2023) on the lru_embed HIP kernels.

Same signatures, defaults, ``ValueError`` messages and ``state_dict`` keys as the reference: ``input_layer``, a stack of
``LRUBlock`` (optional layer norm -> ``LRU`` -> GELU -> dropout -> sigmoid gate -> dropout -> skip), an aggregation over
time and ``output_layer``.  An ``LRU`` is the diagonal complex recurrence ``x_t = lambda x_{t-1} + gamma B u_t``, ``y_t =
Re(C x_t) + D u_t``; bidirectional, the second half of the states runs in reversed time.  Two routes, same semantics:

* the eager route: the written formula in torch, a loop over time in complex arithmetic, differentiable to any order;
* the kernel route: a ``torch.autograd.Function`` on ``sbi_amd_lru_forward`` / ``_backward`` (include/sbi_amd_lru.h)
  that returns ``features`` (B, hidden_dim); ``output_layer`` stays an ordinary linear map behind it.  1 + num_blocks
  launches forward and 2 num_blocks + 2 backward, whatever T.  It is taken for an fp32 (B, T, input_dim) input on a ROCm
  device that does not require grad (the kernels have no d/dx), without layer norm, without active dropout, with
  ``aggregate_fcn`` "mean" or "last_step", when the host-side plan accepts the sizes.  Everything else runs eager -- a
  fallback, never a refusal.  ``LRUBlock`` and ``LRU`` on their own are always eager.

``mode="loop"`` and ``mode="scan"`` are the same function and take the same route here; both have a backward, so the
reference's warning about ``"scan"`` is not raised.  The flat fp32 weight image (complex ``B`` and ``C`` through
``torch.view_as_real``) is rebuilt from the parameters with one ``torch.cat`` per call.
"""

from __future__ import annotations

import ctypes
import math
from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from sbi_amd import _lib

# (input_dim, hidden_dim, state_dim, num_blocks, bidirectional, aggregation)
Dims = Tuple[int, int, int, int, int, int]
PARAMS_PER_BLOCK = 8      # log_nu, log_theta, B, C, D, log_gamma, gate weight, gate bias

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (input_dim <= 64, hidden_dim <= 128, states <= 128, "
                        "num_blocks <= 8, T <= 65535, B T < 2^31 - 64)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "one block's weights plus the time tiles exceed 160 KiB of LDS",
}


def _aggregate_mean(h: Tensor) -> Tensor:
    return h.mean(dim=1)


def _aggregate_last_step(h: Tensor) -> Tensor:
    return h[:, -1, :]


# module-level functions: a net that holds one stays picklable
_AGGREGATIONS = {"mean": _aggregate_mean, "last_step": _aggregate_last_step}
_AGGREGATION_CODES = {"mean": 0, "last_step": 1}


def lru_config(dims: Dims) -> _lib.LRUConfigC:
    return _lib.LRUConfigC(*[int(d) for d in dims])


def plan(dims: Dims, batch: int, steps: int) -> int:
    """0 when the kernels take `batch` sequences of `steps` steps through a net of these sizes, else E_* (host side)."""
    if batch < 1 or steps < 1:
        return _lib.E_BADARG
    return int(_lib.load().sbi_amd_lru_plan(ctypes.byref(lru_config(dims)), batch, steps, None, None))


def plan_reason(rc: int) -> str:
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def param_count(dims: Dims) -> int:
    return int(_lib.load().sbi_amd_lru_param_count(ctypes.byref(lru_config(dims)), None))


def real_view(p: Tensor) -> Tensor:
    return torch.view_as_real(p) if p.is_complex() else p


def flat_image(params: Sequence[Tensor]) -> Tensor:
    """fp32 image in ``state_dict`` order, complex entries as interleaved (re, im)"""
    return torch.cat([real_view(p.detach()).reshape(-1) for p in params])


def split_like(flat: Tensor, params: Sequence[Tensor]) -> List[Tensor]:
    out = []
    for g, p in zip(flat.split([real_view(p).numel() for p in params]), params):
        # (a copy for complex entries: view_as_complex wants an even storage offset, which an odd hidden_dim breaks)
        out.append(torch.view_as_complex(g.view(*p.shape, 2).clone()) if p.is_complex() else g.view_as(p))
    return out


def params_on(params: Sequence[Tensor], x: Tensor) -> bool:
    return all(p.device == x.device and p.dtype in (torch.float32, torch.complex64) for p in params)


# ---- the written formula ----------------------------------------------------------------------------------------------
def _recurrence(lam: Tensor, v: Tensor, state: Tensor) -> Tensor:
    """x_t = lam x_{t-1} + v_t along dim 1, x_{-1} = state: (B, T, S) complex"""
    xs = []
    x = state
    for t in range(v.shape[1]):
        x = lam * x + v[:, t]
        xs.append(x)
    return torch.stack(xs, dim=1)


def lru_apply(u: Tensor, log_nu: Tensor, log_theta: Tensor, B: Tensor, C: Tensor, D: Tensor, log_gamma: Tensor,
              state_dim: int, bidirectional: bool, state: Optional[Tensor] = None) -> Tensor:
    """One LRU on u (batch, T, H): y_t = Re(C x_t) + D u_t, the second half of a bidirectional unit in reversed time."""
    lam = torch.exp(torch.complex(-torch.exp(log_nu), torch.exp(log_theta)))
    v = u.to(B.dtype) @ (B * torch.exp(log_gamma).unsqueeze(-1)).mT
    if state is None:
        state = torch.zeros(u.shape[0], lam.shape[0], dtype=v.dtype, device=u.device)
    S = state_dim
    if bidirectional:
        fwd = _recurrence(lam[:S], v[..., :S], state[:, :S])
        rev = _recurrence(lam[S:], v[..., S:].flip(1), state[:, S:]).flip(1)
        x = torch.cat([fwd, rev], dim=-1)
    else:
        x = _recurrence(lam, v, state)
    return (x @ C.mT).real + u * D


def lru_functional(x: Tensor, params: Sequence[Tensor], dims: Dims) -> Tensor:
    """features of a net without layer norm and dropout on its parameters in ``state_dict`` order: what the kernels
    implement"""
    _, _, S, nb, bidir, agg = dims
    h = torch.nn.functional.linear(x, params[0], params[1])
    for i in range(nb):
        log_nu, log_theta, B, C, D, log_gamma, Wg, bg = params[2 + PARAMS_PER_BLOCK * i: 2 + PARAMS_PER_BLOCK * (i + 1)]
        y = torch.nn.functional.gelu(lru_apply(h, log_nu, log_theta, B, C, D, log_gamma, S, bool(bidir)))
        h = y * torch.sigmoid(torch.nn.functional.linear(y, Wg, bg)) + h
    return h.mean(dim=1) if agg == 0 else h[:, -1, :]


class _LRUEmbedFn(torch.autograd.Function):
    """features (B, hidden_dim) on the kernels; x (B, T, input_dim) contiguous fp32 on the device."""

    @staticmethod
    def forward(ctx, x: Tensor, dims: Dims, *params: Tensor) -> Tensor:
        lib = _lib.load()
        cfg = lru_config(dims)
        flat = flat_image(params)
        B, T = x.shape[0], x.shape[1]
        out = torch.empty(B, dims[1], dtype=torch.float32, device=x.device)
        ws = _workspace(cfg, B, T, 0, x.device)
        _lib.check(lib.sbi_amd_lru_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), B, T, out.data_ptr(),
                                           ws.data_ptr(), _lib.current_stream(x.device)), "lru_forward")
        ctx.dims = dims
        ctx.save_for_backward(x, flat, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, flat, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        dims = ctx.dims
        if torch.is_grad_enabled():
            # double backward (create_graph=True): differentiate the written formula instead
            with torch.enable_grad():
                wanted = [t for t, n in zip(params, need[2:]) if n]
                got = iter(torch.autograd.grad(lru_functional(x, params, dims), wanted, grad_out, create_graph=True))
            return (None, None, *[next(got) if n else None for n in need[2:]])
        lib = _lib.load()
        cfg = lru_config(dims)
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        B, T = x.shape[0], x.shape[1]
        ws = _workspace(cfg, B, T, 1, x.device)
        _lib.check(lib.sbi_amd_lru_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), B, T, grad_out.data_ptr(),
                                            grad_flat.data_ptr(), ws.data_ptr(), _lib.current_stream(x.device)),
                   "lru_backward")
        grads = [g if n else None for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (None, None, *grads)


def _workspace(cfg, B: int, T: int, backward: int, device) -> Tensor:
    nbytes = int(_lib.load().sbi_amd_lru_workspace_bytes(ctypes.byref(cfg), B, T, backward))
    if nbytes < 0:
        _lib.check(nbytes, "lru_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


# ---- the modules ------------------------------------------------------------------------------------------------------
class LRU(nn.Module):
    """A single Linear Recurrent Unit with output_dim = input_dim, so D is a vector and units stack without linear
    layers in between.

    Args:
        input_dim: width of the sequence (batch, T, input_dim).
        state_dim: number of complex states per direction.
        r_min, r_max: ring of |lambda| at initialisation, 0 <= r_min < r_max <= 1.
        phase_max: largest phase of lambda at initialisation, at most 2 pi.
        bidirectional: a second set of state_dim states runs in reversed time.
        mode: "loop" or "scan"; the same function here.
    """

    def __init__(self, input_dim: int, state_dim: int, r_min: float, r_max: float, phase_max: float,
                 bidirectional: bool, mode: str):
        super().__init__()
        if not isinstance(input_dim, int) or input_dim <= 0:
            raise ValueError("input_dim must be a positive integer.")
        if not isinstance(state_dim, int) or state_dim <= 0:
            raise ValueError("state_dim must be a positive integer.")
        if not (0 <= r_min < r_max <= 1):
            raise ValueError(f"Invalid {r_min=} and/or {r_max=}. They must satisfy 0 <= r_min < r_max <= 1.")
        if not (0 <= phase_max <= 2 * torch.pi):
            raise ValueError(f"Invalid {phase_max=}. It must satisfy 0 <= phase_max <= 2 pi.")
        if mode not in ("loop", "scan"):
            raise ValueError(f"Invalid {mode=}. Must be 'loop' or 'scan'.")
        self.state_dim = state_dim
        self.bidirectional = bidirectional
        self.mode = mode
        n = state_dim * (2 if bidirectional else 1)

        # ring initialisation (section 3.2 of the paper): |lambda|^2 uniform in [r_min^2, r_max^2], phase in [0, phase_max]
        radius_sq = torch.rand(n) * (r_max**2 - r_min**2) + r_min**2
        self.log_nu = nn.Parameter(torch.log(-0.5 * torch.log(radius_sq)))
        self.log_theta = nn.Parameter(torch.log(phase_max * torch.rand(n)))
        # Glorot-scaled complex projections
        scale = 1.0 / math.sqrt(2 * input_dim)
        self.B = nn.Parameter(torch.complex(torch.randn(n, input_dim) * scale, torch.randn(n, input_dim) * scale))
        self.C = nn.Parameter(torch.complex(torch.randn(input_dim, n) * scale, torch.randn(input_dim, n) * scale))
        self.D = nn.Parameter(torch.randn(input_dim))
        # gamma normalises the input so that the state's variance does not depend on |lambda|
        self.log_gamma = nn.Parameter(torch.log(torch.sqrt(1 - self.lambda_abs.detach() ** 2)))

    @property
    def lambda_abs(self) -> Tensor:
        return torch.exp(-torch.exp(self.log_nu))

    @property
    def lambda_complex(self) -> Tensor:
        return torch.exp(torch.complex(-torch.exp(self.log_nu), torch.exp(self.log_theta)))

    @property
    def gamma(self) -> Tensor:
        return torch.exp(self.log_gamma)

    def forward(self, input: Tensor, state: Optional[Tensor] = None, mode: Optional[str] = None) -> Tensor:
        """(batch, T, input_dim) -> (batch, T, input_dim); `state` (batch, states) complex is the state before the
        first step of either direction (zero by default)."""
        expected_state_shape = (input.size(0), self.state_dim * (2 if self.bidirectional else 1))
        if state is not None:
            state = state.to(device=input.device)
            assert state.shape == expected_state_shape, (
                f"Invalid state shape {state.shape}, expected {expected_state_shape}")
        mode = mode or self.mode
        if mode not in ("loop", "scan"):
            raise ValueError(f"Invalid {mode=}. Must be 'loop' or 'scan'.")
        return lru_apply(input, self.log_nu, self.log_theta, self.B, self.C, self.D, self.log_gamma, self.state_dim,
                         self.bidirectional, state)


class LRUBlock(nn.Module):
    """[layer norm ->] LRU -> GELU -> dropout -> y sigmoid(W y + b) -> dropout -> + input; meant to sit between linear
    layers that set the width, so that blocks stack directly."""

    def __init__(self, hidden_dim: int, state_dim: int, r_min: float, r_max: float, phase_max: float,
                 bidirectional: bool, mode: str, dropout: float, apply_input_normalization: bool):
        super().__init__()
        self.input_norm = nn.LayerNorm(hidden_dim) if apply_input_normalization else nn.Identity()
        self.lru = LRU(input_dim=hidden_dim, state_dim=state_dim, r_min=r_min, r_max=r_max, phase_max=phase_max,
                       bidirectional=bidirectional, mode=mode)
        self.dropout = nn.Dropout(dropout)
        self.nonlinearity = nn.GELU()
        self.state_mixing_gate = nn.Linear(hidden_dim, hidden_dim)
        self.sigmoid = nn.Sigmoid()

    def forward(self, input: Tensor) -> Tensor:
        y = self.dropout(self.nonlinearity(self.lru(self.input_norm(input))))
        y = self.dropout(y * self.sigmoid(self.state_mixing_gate(y)))
        return y + input


class LRUEmbedding(nn.Module):
    """sbi's ``LRUEmbedding``: an embedding net for sequences (batch, T, input_dim) of one length.

    Args:
        input_dim: width of an observation's time step.
        output_dim: number of features.
        state_dim: complex states per direction of every LRU.
        hidden_dim: width of the blocks.
        num_blocks: number of LRU blocks, at least 1.
        r_min, r_max, phase_max: ring initialisation of lambda (r_max < 1 for a stable system; a small phase_max,
            e.g. below pi / 10, is advised for long sequences).
        bidirectional: run every LRU in both time directions (doubles the states).
        mode: "loop" or "scan": the same function and the same route here, both with a backward.
        dropout: rate of the two dropout layers of every block.
        apply_input_normalization: a layer norm in front of every LRU.
        aggregate_fcn: "mean", "last_step" or a callable (batch, T, hidden_dim) -> (batch, hidden_dim).

    ``force_eager = True`` on an instance pins the eager route: no lru kernel is launched.
    """

    force_eager = False

    def __init__(self, input_dim: int, output_dim: int, state_dim: int = 20, hidden_dim: int = 40, num_blocks: int = 2,
                 r_min: float = 0.0, r_max: float = 1.0, phase_max: float = 2 * math.pi, bidirectional: bool = True,
                 mode: str = "loop", dropout: float = 0.0, apply_input_normalization: bool = False,
                 aggregate_fcn: Union[str, Callable] = "mean"):
        super().__init__()
        self.input_layer = nn.Linear(input_dim, hidden_dim)
        if num_blocks < 1:
            raise ValueError("num_blocks must be >= 1.")
        self.lru_blocks = nn.Sequential(*[
            LRUBlock(hidden_dim=hidden_dim, state_dim=state_dim, r_min=r_min, r_max=r_max, phase_max=phase_max,
                     bidirectional=bidirectional, mode=mode, dropout=dropout,
                     apply_input_normalization=apply_input_normalization) for _ in range(num_blocks)])
        if isinstance(aggregate_fcn, str):
            if aggregate_fcn not in _AGGREGATIONS:
                raise ValueError(f"aggregate_fcn {aggregate_fcn} not implemented, use one of "
                                 f"{sorted(_AGGREGATIONS)} or pass a function.")
            self.aggregation = _AGGREGATIONS[aggregate_fcn]
        else:
            self.aggregation = aggregate_fcn
        self.output_layer = nn.Linear(hidden_dim, output_dim)
        self._aggregation_code = _AGGREGATION_CODES.get(aggregate_fcn) if isinstance(aggregate_fcn, str) else None
        self._layer_norm = bool(apply_input_normalization)
        self._dropout = float(dropout)
        self._dims: Dims = (int(input_dim), int(hidden_dim), int(state_dim), int(num_blocks), int(bool(bidirectional)),
                            int(self._aggregation_code or 0))

    @property
    def dims(self) -> Dims:
        return self._dims

    def kernel_parameters(self) -> List[Tensor]:
        """input layer and blocks in ``state_dict`` order (without layer norms): the kernels' flat image."""
        out: List[Tensor] = [self.input_layer.weight, self.input_layer.bias]
        for blk in self.lru_blocks:
            u = blk.lru
            out += [u.log_nu, u.log_theta, u.B, u.C, u.D, u.log_gamma, blk.state_mixing_gate.weight,
                    blk.state_mixing_gate.bias]
        return out

    def static_route(self) -> Tuple[bool, str]:
        """The part of the routing decision that does not depend on the input."""
        if self.force_eager:
            return False, "force_eager is set"
        if self._layer_norm:
            return False, "apply_input_normalization (no layer norm in the kernels)"
        if self._dropout > 0 and self.training:
            return False, "dropout in training mode (no dropout in the kernels)"
        if self._aggregation_code is None:
            return False, "aggregate_fcn is a callable"
        return True, "kernel"

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        ok, why = self.static_route()
        if not ok:
            return ok, why
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.dim() != 3 or x.shape[2] != self._dims[0]:
            return False, "input is not (batch, T, input_dim)"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        if not params_on(self.kernel_parameters(), x):
            return False, "parameters are not float32 / complex64 on the input's device"
        rc = plan(self._dims, x.shape[0], x.shape[1])
        if rc != 0:
            return False, plan_reason(rc)
        return True, "kernel"

    def features(self, x: Tensor) -> Tensor:
        """The aggregated hidden state (batch, hidden_dim) in front of ``output_layer``."""
        if self.kernel_route(x)[0]:
            return _LRUEmbedFn.apply(x.contiguous(), self._dims, *self.kernel_parameters())
        return self.aggregation(self.lru_blocks(self.input_layer(x)))

    def forward(self, input: Tensor) -> Tensor:
        """(batch, T, input_dim) -> (batch, output_dim)."""
        return self.output_layer(self.features(input))
