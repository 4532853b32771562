"""``PermutationInvariantEmbedding`` -- sbi/neural_nets/embedding_nets/permutation_invariant.py on the embed HIP
kernels: amortised inference on a varying number of iid trials, missing trials encoded as NaN.

``forward`` has two routes with the same semantics: the eager composition below (``_eager``) and a
``torch.autograd.Function`` on ``sbi_amd_perminv_forward`` / ``_backward`` (include/sbi_amd_embed.h).  The kernel route
pools in the launch and its backward recomputes the trial-net activations, so no (batch x trials, hidden) tensor is ever
materialised.  ``kernel_route(x)`` answers ``(bool, reason)``.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets.fully_connected import (Dims, FCEmbedding, fc_functional, flat_image, params_on,
                                                                plan, plan_reason, split_like, workspace)


def _pool(x: Tensor, trial_out: Tensor, mean: bool, dim: int = 1) -> Tensor:
    """[pooled | count] from the trial embeddings of x: the semantics both routes share."""
    missing = torch.isnan(x).all(-1, keepdim=True)                  # a trial whose entries are all NaN
    counts = (~missing).sum(dim=dim).to(trial_out.dtype)            # valid trials of each batch element
    pooled = torch.where(missing, torch.zeros((), dtype=trial_out.dtype, device=trial_out.device), trial_out).sum(dim=dim)
    if mean:
        pooled = pooled / counts
    return torch.cat([pooled, counts], dim=1)


def _zero_nan(x: Tensor) -> Tensor:
    return torch.where(torch.isnan(x), torch.zeros((), dtype=x.dtype, device=x.device), x)


def _perminv_config(trial: Dims, head: Dims, mean: bool) -> _lib.PermInvConfigC:
    return _lib.PermInvConfigC(_lib.FCEmbedConfigC(*trial), _lib.FCEmbedConfigC(*head), int(mean))


class _PermInvFn(torch.autograd.Function):
    """out = head([pool(trial_net(x)) | count]); x (B, T, Dx) contiguous fp32 on the device, no d/dx."""

    @staticmethod
    def forward(ctx, x: Tensor, trial: Dims, head: Dims, mean: bool, *params: Tensor) -> Tensor:
        lib = _lib.load()
        n_trial = 2 * trial[3]
        flat_t, flat_h = flat_image(params[:n_trial]), flat_image(params[n_trial:])
        B, T = x.shape[0], x.shape[1]
        out = torch.empty(B, head[2], dtype=torch.float32, device=x.device)
        head_in = torch.empty(B, head[0], dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_perminv_forward(ctypes.byref(_perminv_config(trial, head, mean)), flat_t.data_ptr(),
                                               flat_h.data_ptr(), x.data_ptr(), B, T, out.data_ptr(),
                                               head_in.data_ptr(), _lib.current_stream(x.device)), "perminv_forward")
        ctx.cfg = (trial, head, mean)
        ctx.save_for_backward(x, flat_t, flat_h, head_in, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, flat_t, flat_h, head_in, *params = ctx.saved_tensors
        trial, head, mean = ctx.cfg
        n_trial = 2 * trial[3]
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # double backward (create_graph=True): differentiate the written formula instead
            with torch.enable_grad():
                emb = fc_functional(_zero_nan(x), params[:n_trial])
                out = fc_functional(_pool(x, emb, mean), params[n_trial:])
                wanted = [p for p, n in zip(params, need[4:]) if n]
                got = iter(torch.autograd.grad(out, wanted, grad_out, create_graph=True))
            return (None, None, None, None, *[next(got) if n else None for n in need[4:]])
        lib = _lib.load()
        B, T = x.shape[0], x.shape[1]
        grad_out = grad_out.contiguous()
        grad_t, grad_h = torch.empty_like(flat_t), torch.empty_like(flat_h)
        grad_head_in = torch.empty_like(head_in)
        ws_t, ws_h = workspace(trial, B * T, x.device), workspace(head, B, x.device)
        ws = ws_t if ws_t.numel() >= ws_h.numel() else ws_h
        _lib.check(lib.sbi_amd_perminv_backward(ctypes.byref(_perminv_config(trial, head, mean)), flat_t.data_ptr(),
                                                flat_h.data_ptr(), x.data_ptr(), B, T, head_in.data_ptr(),
                                                grad_out.data_ptr(), grad_t.data_ptr(), grad_h.data_ptr(),
                                                grad_head_in.data_ptr(), ws.data_ptr(),
                                                _lib.current_stream(x.device)), "perminv_backward")
        grads = split_like(grad_t, params[:n_trial]) + split_like(grad_h, params[n_trial:])
        return (None, None, None, None, *[g if n else None for g, n in zip(grads, need[4:])])


class PermutationInvariantEmbedding(nn.Module):
    """Permutation invariant embedding network (sbi's ``PermutationInvariantEmbedding``).

    x (batch, trials, input_dim) -> (batch, output_dim): the trial_net embeds every trial on its own, the embeddings
    of an element's valid trials are summed or averaged, and an ``FCEmbedding`` (``fc_subnet``) maps ``[pooled | number
    of valid trials]`` to the output.  Missing trials are NaN padding: a NaN entry reads as 0, and a trial whose entries
    are ALL NaN adds exactly +0 to the pooled sum and is not counted.

    Args:
        trial_net: module for one trial, (rows, input_dim) -> (rows, trial_net_output_dim).  Our ``FCEmbedding`` with
            ReLU and no layer norm runs on the kernels; any other module runs the eager route.
        trial_net_output_dim: width of the trial_net's output.
        aggregation_fn: "sum" or "mean" over the valid trials.
        num_hiddens, num_layers, output_dim: sizes of ``fc_subnet``.
        aggregation_dim: the trials' dimension of x; 1 on the kernel route.

    Departures from sbi:

    * Count.  sbi computes ``isnan(x).sum(1).reshape(-1)[:B]``, which for input_dim > 1 reads the counts of batch
      elements 0 .. B / input_dim instead of each element's own.  Here the count of element b is the number of its
      trials that are not entirely NaN.  The two agree when input_dim == 1, B == 1 or all counts are equal.
    * All-NaN element under "mean".  sbi asserts ``not isnan(combined).any()``, a device read-back on every forward.
      Here nothing is read back: an element without a valid trial gives NaN in its own output row and leaves every
      other row untouched.  (Under "sum" its row is the head applied to ``[0 ... 0, 0]``.)
    * Only NaN is masked; +-Inf entries are passed on as they are and make that element's row non-finite (sbi's
      ``nan_to_num`` clamps them to the largest finite float).

    ``force_eager = True`` on an instance pins the eager route.  The eager route is eager torch all the way down: it
    runs the sub-nets' ``nn.Sequential`` and launches none of the embed kernels, whatever the sub-nets' own flags say.
    """

    force_eager = False

    def __init__(self, trial_net: nn.Module, trial_net_output_dim: int, aggregation_fn: Optional[str] = "sum",
                 num_hiddens: int = 100, num_layers: int = 2, output_dim: int = 20, aggregation_dim: int = 1):
        assert aggregation_fn in ("mean", "sum"), "aggregation_fn must be 'mean' or 'sum'."     # (sbi's message)
        super().__init__()
        self.trial_net, self.aggregation_fn, self.aggregation_dim = trial_net, aggregation_fn, aggregation_dim
        self.fc_subnet = FCEmbedding(input_dim=trial_net_output_dim + 1,     # + 1: the number of trials
                                     output_dim=output_dim, num_layers=num_layers, num_hiddens=num_hiddens)

    def _eager(self, x: Tensor) -> Tensor:
        """The written formula in eager torch all the way down: our own sub-nets run their `nn.Sequential`, never
        their kernel route (a custom trial_net runs as whatever it is)."""
        trial = self.trial_net.net if isinstance(self.trial_net, FCEmbedding) else self.trial_net
        emb = trial(_zero_nan(x))
        return self.fc_subnet.net(_pool(x, emb, self.aggregation_fn == "mean", self.aggregation_dim))

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        if self.force_eager:
            return False, "force_eager is set"
        if self.aggregation_dim != 1:
            return False, "aggregation_dim is not 1"
        if not isinstance(self.trial_net, FCEmbedding):
            return False, "trial_net is not sbi_amd's FCEmbedding"
        for name, net in (("trial_net", self.trial_net), ("fc_subnet", self.fc_subnet)):
            ok, why = net.static_route()
            if not ok:
                return False, f"{name}: {why}"
        if self.fc_subnet.dims[0] != self.trial_net.dims[2] + 1:
            return False, "trial_net_output_dim does not match the trial_net"
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.dim() != 3 or x.shape[-1] != self.trial_net.dims[0]:
            return False, "input is not (batch, trials, input_dim)"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        if not params_on(self.trial_net.linear_parameters() + self.fc_subnet.linear_parameters(), x):
            return False, "parameters are not float32 on the input's device"
        B, T = x.shape[0], x.shape[1]
        for name, rc in (("trial_net", plan(self.trial_net.dims, B, T)), ("fc_subnet", plan(self.fc_subnet.dims, B))):
            if rc != 0:
                return False, f"{name}: {plan_reason(rc)}"
        return True, "kernel"

    def forward(self, x: Tensor) -> Tensor:
        """Network forward pass: (batch_size, permutation_dim, input_dim) -> (batch_size, output_dim)."""
        if not self.kernel_route(x)[0]:
            return self._eager(x)
        return _PermInvFn.apply(x.contiguous(), self.trial_net.dims, self.fc_subnet.dims, self.aggregation_fn == "mean",
                                *self.trial_net.linear_parameters(), *self.fc_subnet.linear_parameters())


def masks_nan_trials(estimator) -> bool:
    """True when the estimator's embedding net is a ``PermutationInvariantEmbedding`` (directly, or as the last module
    of the ``Standardize -> embedding`` wrapper the builders put in front): only then is a NaN-padded x meaningful."""
    emb = getattr(estimator, "embedding_net", None)
    if isinstance(emb, nn.Sequential) and len(emb) > 0:
        emb = emb[-1]
    return isinstance(emb, PermutationInvariantEmbedding)
