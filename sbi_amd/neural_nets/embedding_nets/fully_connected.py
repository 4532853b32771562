"""``FCEmbedding`` -- sbi/neural_nets/embedding_nets/fully_connected.py on the embed HIP kernels.

Same signature, defaults and ``state_dict`` keys as the reference: ``num_layers`` ``nn.Linear`` layers, each followed
by the activation (the last one too), an optional layer norm after every layer but the last.  ``forward`` has two
routes with the same semantics:

* the eager route: ``self.net(x)``, the written formula;
* the kernel route: a ``torch.autograd.Function`` on ``sbi_amd_fc_embed_forward`` / ``_backward``
  (include/sbi_amd_embed.h), taken for an fp32 input on a ROCm device when the activation is ``nn.ReLU``, there is no
  layer norm and the host-side plan accepts the shape.  Everything else runs eager -- a fallback, never a refusal.

``kernel_route(x)`` answers ``(bool, reason)`` for a given input.  The kernels read one flat fp32 weight image in
``state_dict`` order; it is rebuilt from the ``nn.Linear`` parameters with one ``torch.cat`` per call, so ``.to()``,
``copy.deepcopy``, ``load_state_dict`` and in-place optimizer updates need no bookkeeping.
"""

from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

import torch
from torch import Tensor, nn

from sbi_amd import _lib

Dims = Tuple[int, int, int, int]     # (in_dim, hidden, out_dim, num_layers)

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (in_dim <= 64, hidden <= 128, out_dim <= 64, "
                        "2 <= num_layers <= 4, T <= 65535)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "weight image plus row tiles exceed 160 KiB of LDS",
}


def fc_config(dims: Dims) -> _lib.FCEmbedConfigC:
    return _lib.FCEmbedConfigC(*[int(d) for d in dims])


def plan(dims: Dims, rows: int, trials: int = 1) -> int:
    """0 when the kernels take `rows` x `trials` rows through a net of these sizes, else E_* (a host-side answer)."""
    if rows < 1 or trials < 1:
        return _lib.E_BADARG
    return int(_lib.load().sbi_amd_embed_plan(ctypes.byref(fc_config(dims)), rows, trials, None, None))


def plan_reason(rc: int) -> str:
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def fc_functional(x: Tensor, params: Sequence[Tensor]) -> Tensor:
    """relu(W x + b) layer by layer on (weight, bias, weight, bias, ...): the formula the kernels implement."""
    for w, b in zip(params[0::2], params[1::2]):
        x = torch.relu(torch.nn.functional.linear(x, w, b))
    return x


def flat_image(params: Sequence[Tensor]) -> Tensor:
    return torch.cat([p.detach().reshape(-1) for p in params])


def split_like(flat: Tensor, params: Sequence[Tensor]) -> List[Tensor]:
    return [g.view_as(p) for g, p in zip(flat.split([p.numel() for p in params]), params)]


def params_on(params: Sequence[Tensor], x: Tensor) -> bool:
    return all(p.device == x.device and p.dtype == torch.float32 for p in params)


def workspace(dims: Dims, rows: int, device) -> Tensor:
    nbytes = int(_lib.load().sbi_amd_embed_workspace_bytes(ctypes.byref(fc_config(dims)), rows))
    if nbytes < 0:
        _lib.check(nbytes, "embed_workspace_bytes")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


class _FCEmbedFn(torch.autograd.Function):
    """out = net(x) on the kernels; x (N, in_dim) contiguous fp32 on the device."""

    @staticmethod
    def forward(ctx, x: Tensor, dims: Dims, *params: Tensor) -> Tensor:
        lib = _lib.load()
        flat = flat_image(params)
        out = torch.empty(x.shape[0], dims[2], dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_fc_embed_forward(ctypes.byref(fc_config(dims)), flat.data_ptr(), x.data_ptr(),
                                                x.shape[0], out.data_ptr(), _lib.current_stream(x.device)),
                   "fc_embed_forward")
        ctx.dims = dims
        ctx.save_for_backward(x, flat, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, flat, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # double backward (create_graph=True): differentiate the written formula instead
            with torch.enable_grad():
                wanted = [t for t, n in zip([x, *params], [need[0], *need[2:]]) if n]
                got = iter(torch.autograd.grad(fc_functional(x, params), wanted, grad_out, create_graph=True))
            return tuple(next(got) if n else None for n in need)
        lib = _lib.load()
        dims = ctx.dims
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        grad_x = torch.empty_like(x) if need[0] else None
        ws = workspace(dims, x.shape[0], x.device)
        _lib.check(lib.sbi_amd_fc_embed_backward(ctypes.byref(fc_config(dims)), flat.data_ptr(), x.data_ptr(),
                                                 x.shape[0], grad_out.data_ptr(), grad_flat.data_ptr(),
                                                 _lib.ptr(grad_x), ws.data_ptr(), _lib.current_stream(x.device)),
                   "fc_embed_backward")
        grads = [g if n else None for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (grad_x, None, *grads)


class FCEmbedding(nn.Module):
    """sbi's ``FCEmbedding``: an MLP of ``num_layers`` Linear layers, every one followed by the activation.

    Args:
        input_dim: width of a row of x.
        output_dim: width of the embedding.
        num_layers: how many Linear layers, the input and the output layer included (2 at the least).
        num_hiddens: width of every layer between the first and the last.
        enable_layer_norm: a LayerNorm after every Linear but the last; True runs the eager route.
        activation: the activation's class; anything but nn.ReLU runs the eager route.

    ``force_eager = True`` on an instance pins the eager route.
    """

    force_eager = False

    def __init__(self, input_dim: int, output_dim: int = 20, num_layers: int = 2, num_hiddens: int = 50,
                 enable_layer_norm: bool = False, activation: nn.Module = nn.ReLU):
        super().__init__()
        num_layers = max(int(num_layers), 2)
        norm = nn.LayerNorm if enable_layer_norm else nn.Identity
        widths = [input_dim] + [num_hiddens] * (num_layers - 1) + [output_dim]
        modules: List[nn.Module] = []
        for i in range(num_layers):
            modules.append(nn.Linear(widths[i], widths[i + 1]))
            if i < num_layers - 1:
                modules.append(norm(num_hiddens))     # nn.Identity keeps the reference's module indices
            modules.append(activation())
        self.net = nn.Sequential(*modules)
        self._dims: Dims = (int(input_dim), int(num_hiddens), int(output_dim), num_layers)
        self._relu = activation is nn.ReLU
        self._layer_norm = bool(enable_layer_norm)

    @property
    def dims(self) -> Dims:
        return self._dims

    def linear_parameters(self) -> List[Tensor]:
        """(weight, bias) of every ``nn.Linear`` in ``state_dict`` order: the kernels' flat image."""
        out: List[Tensor] = []
        for m in self.net:
            if isinstance(m, nn.Linear):
                out += [m.weight, m.bias]
        return out

    def static_route(self) -> Tuple[bool, str]:
        """The part of the routing decision that does not depend on the input."""
        if self.force_eager:
            return False, "force_eager is set"
        if not self._relu:
            return False, "activation is not nn.ReLU"
        if self._layer_norm:
            return False, "layer norm is enabled"
        return True, "kernel"

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        ok, why = self.static_route()
        if not ok:
            return ok, why
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.dim() < 1 or x.shape[-1] != self._dims[0]:
            return False, "input shape does not match input_dim"
        if not params_on(self.linear_parameters(), x):
            return False, "parameters are not float32 on the input's device"
        rc = plan(self._dims, x.numel() // self._dims[0])
        if rc != 0:
            return False, plan_reason(rc)
        return True, "kernel"

    def forward(self, x: Tensor) -> Tensor:
        """Network forward pass: (batch_size, num_features) -> (batch_size, output_dim)."""
        if not self.kernel_route(x)[0]:
            return self.net(x)
        x2 = x.reshape(-1, self._dims[0]).contiguous()
        out = _FCEmbedFn.apply(x2, self._dims, *self.linear_parameters())
        return out.reshape(*x.shape[:-1], self._dims[2])
