"""``SpectralConvEmbedding`` -- sbi/neural_nets/embedding_nets/SC_embedding.py (the Fourier-neural-operator embedding of
Lingsch et al. / Li et al. for series on equispaced or arbitrary 1-D grids) on the sc_embed HIP kernels.

Same signatures, defaults, messages and ``state_dict`` keys as the reference: ``fc0`` lifts the input channels to
``conv_channels``; every layer adds a spectral convolution (``SpectralConv1d_SMM``: a transform truncated to ``modes``
Fourier modes through the dense operator of ``VFT``, a complex channel mix per mode, the inverse transform) to a pointwise
``Conv1d`` and applies GELU; ``conv_last`` returns the mixed coefficients themselves and ``fc_last`` reduces their
channels.  Input (batch, in_channels, n_points) on the equispaced grid, or (batch, 2, in_channels, n_points) with the
positions in ``x[:, 1, 0, :]``; output (batch, 2 * modes * out_channels).  Two routes with the same semantics:

* the eager route: the written formula on the submodules, with ``VFT``'s (batch, modes, n_points) operator;
* the kernel route: a ``torch.autograd.Function`` on ``sbi_amd_sc_forward`` / ``_backward`` (include/sbi_amd_sc.h) that
  covers the whole module, ``fc0`` to ``fc_last``: one launch forward, one and a reduction backward; the operator and
  the per-layer maps never exist in global memory.  It is taken for an fp32 input on a ROCm device that does not
  require grad (the kernels have no d/dx), when the parameters are fp32 / complex64 on that device and the host-side
  plan accepts the shape.  Everything else runs eager -- a fallback, never a refusal.  The complex weights go through
  the function as ``torch.view_as_real(weights1)``, so their ``.grad`` is complex64 in torch's convention.

``VFT`` and ``SpectralConv1d_SMM`` are always eager.  Departure from the reference: ``VFT`` builds its operators on
the device of ``point_positions``, or on ``device=`` on the equispaced grid (the reference builds them on the host and
cannot take a device tensor there); ``SpectralConvEmbedding`` passes the input's device and dtype.
"""

from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets.fully_connected import flat_image, split_like

# (in_channels, modes, out_channels, conv_channels, num_layers)
Dims = Tuple[int, int, int, int, int]

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (channels <= 32, modes <= 64, num_layers <= 8, n_points <= "
                        "65535, B C n_points < 2^31)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "the sample's maps, twiddles and gradient accumulators do not fit 160 KiB of LDS",
}


def sc_config(dims: Dims, n_points: int, has_positions: bool) -> _lib.SCConfigC:
    cfg = _lib.SCConfigC()
    cfg.in_channels, cfg.modes, cfg.out_channels, cfg.conv_channels, cfg.num_layers = (int(d) for d in dims)
    cfg.n_points, cfg.has_positions = int(n_points), int(bool(has_positions))
    return cfg


def plan(dims: Dims, n_points: int, batch: int, has_positions: bool) -> Tuple[int, int]:
    """(rc, parts): rc is 0 when the kernels take `batch` samples of `n_points` points through a module of these sizes,
    else E_*; parts is the number of ranges the sums over the points are cut into.  A host-side answer."""
    if batch < 1:
        return _lib.E_BADARG, 0
    parts = ctypes.c_int32(0)
    rc = int(_lib.load().sbi_amd_sc_plan(ctypes.byref(sc_config(dims, n_points, has_positions)), batch, None, None,
                                         ctypes.byref(parts)))
    return rc, int(parts.value)


def plan_reason(rc: int) -> str:
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def param_count(dims: Dims) -> int:
    return int(_lib.load().sbi_amd_sc_param_count(ctypes.byref(sc_config(dims, 2, False)), None))


def _split_input(x: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
    """(values (batch, channels, n_points), positions (batch, n_points) or None)"""
    if x.ndim == 3:
        return x, None
    if x.ndim == 4:
        return x[:, 0], x[:, 1, 0, :]
    raise ValueError("Input tensor should be 3D (batch_size, channels, n_points) or 4D (batch_size, 2, channels, "
                     f"n_points). The tensor that was passed has shape {x.shape}.")


def sc_functional(x: Tensor, params: Sequence[Tensor], dims: Dims) -> Tensor:
    """The formula the kernels implement, on (fc0.weight, fc0.bias, weights1 of every layer, (weight, bias) of every
    pointwise layer, conv_last.weights1, fc_last.weight, fc_last.bias) with the spectral weights complex."""
    _, modes, _, _, L = dims
    values, positions = _split_input(x)
    batch, _, n = values.shape
    vft = VFT(batch, n, modes, positions, device=values.device, dtype=values.dtype)
    fc0w, fc0b = params[0], params[1]
    spectral, point = params[2:2 + L], params[2 + L:2 + 3 * L]
    last, flw, flb = params[2 + 3 * L], params[3 + 3 * L], params[4 + 3 * L]
    h = torch.nn.functional.linear(values.permute(0, 2, 1), fc0w, fc0b)
    for l in range(L):
        y = vft.inverse(_mix(vft.forward(h.to(vft.V_fwd.dtype)), spectral[l].to(vft.V_fwd.dtype))).real
        h = torch.nn.functional.gelu(y + torch.nn.functional.linear(h, point[2 * l][..., 0], point[2 * l + 1]))
    z = _real_rows(_mix(vft.forward(h.to(vft.V_fwd.dtype)), last.to(vft.V_fwd.dtype)))
    return torch.nn.functional.linear(z, flw, flb).reshape(batch, -1)


def _real_rows(coeff: Tensor) -> Tensor:
    """(batch, modes, channels) complex -> (batch, 2 * modes, channels): row 2 k the real, row 2 k + 1 the imaginary
    part of mode k.  Stacked, not a permuted view_as_real: that one's backward needs even strides and fails on a
    device for one channel."""
    return torch.stack([coeff.real, coeff.imag], dim=2).reshape(coeff.shape[0], 2 * coeff.shape[1], coeff.shape[2])


def _mix(coeff: Tensor, weights: Tensor) -> Tensor:
    """(batch, modes, in) x (in, out, modes) -> (batch, modes, out): one complex channel mix per mode"""
    return torch.einsum("bxi,iox->bxo", coeff, weights)


class _SCEmbedFn(torch.autograd.Function):
    """out = module(x) on the kernels; x (B, C, n) or (B, 2, C, n) contiguous fp32 on the device; the spectral weights
    as view_as_real pairs."""

    @staticmethod
    def _views(x: Tensor, cin: int):
        n = x.shape[-1]
        if x.ndim == 3:
            return x.data_ptr(), x.stride(0), n, None, 0
        return x.data_ptr(), x.stride(0), n, x.data_ptr() + 4 * cin * n, x.stride(0)

    @staticmethod
    def forward(ctx, x: Tensor, dims: Dims, *params: Tensor) -> Tensor:
        lib = _lib.load()
        cfg = sc_config(dims, x.shape[-1], x.ndim == 4)
        flat = flat_image(params)
        out = torch.empty(x.shape[0], 2 * dims[1] * dims[2], dtype=torch.float32, device=x.device)
        xp, xbs, xcs, pp, pbs = _SCEmbedFn._views(x, dims[0])
        _lib.check(lib.sbi_amd_sc_forward(ctypes.byref(cfg), flat.data_ptr(), xp, xbs, xcs, pp, pbs, x.shape[0],
                                          out.data_ptr(), _lib.current_stream(x.device)), "sc_forward")
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
                cplx = [torch.view_as_complex(p) if p.ndim == 4 else p for p in params]
                wanted = [t for t, n in zip(params, need[2:]) if n]
                got = iter(torch.autograd.grad(sc_functional(x, cplx, dims), wanted, grad_out, create_graph=True))
            return (None, None, *[next(got) if n else None for n in need[2:]])
        lib = _lib.load()
        cfg = sc_config(dims, x.shape[-1], x.ndim == 4)
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        nbytes = int(lib.sbi_amd_sc_workspace_bytes(ctypes.byref(cfg), x.shape[0]))
        if nbytes < 0:
            _lib.check(nbytes, "sc_workspace_bytes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        xp, xbs, xcs, pp, pbs = _SCEmbedFn._views(x, dims[0])
        _lib.check(lib.sbi_amd_sc_backward(ctypes.byref(cfg), flat.data_ptr(), xp, xbs, xcs, pp, pbs, x.shape[0],
                                           grad_out.data_ptr(), grad_flat.data_ptr(), ws.data_ptr(),
                                           _lib.current_stream(x.device)), "sc_backward")
        # a real-pair gradient goes back through view_as_real: its own storage, so that the pairs are aligned
        grads = [(g.clone() if g.ndim == 4 else g) if n else None
                 for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (None, None, *grads)


# ---- the modules ------------------------------------------------------------------------------------------------------
class VFT:
    """Truncated Fourier transform on an equispaced or an arbitrary 1-D grid as a dense operator:
    ``V_fwd[b, k, n] = exp(-2 pi i k t_n)`` (batch, modes, n_points) and ``V_inv``, its conjugate transpose.

    Args:
        batch_size: number of samples.
        n_points: number of grid points.
        modes: number of Fourier modes kept, at most n_points // 2 + 1.
        point_positions: (batch_size, n_points) positions normalised with the domain length; n / n_points when None.
        device, dtype: where the operators of the equispaced grid are built (those of `point_positions` otherwise).
    """

    def __init__(self, batch_size: int, n_points: int, modes: int, point_positions: Optional[Tensor] = None,
                 device=None, dtype: Optional[torch.dtype] = None):
        self.number_points = n_points
        self.batch_size = batch_size
        self.modes = modes
        if point_positions is not None:
            times = point_positions[:, None, :]
            device, dtype = point_positions.device, point_positions.dtype
        else:
            grid = torch.arange(n_points, device=device) / n_points
            times = grid.to(dtype or torch.float32).expand(batch_size, 1, n_points)
        self.new_times = times * 2 * math.pi
        self.X_ = torch.arange(modes, device=device).to(self.new_times.dtype).expand(batch_size, modes)[:, :, None]
        self.V_fwd, self.V_inv = self.make_matrix()

    def make_matrix(self) -> Tuple[Tensor, Tensor]:
        """(V_fwd (batch, modes, n_points), V_inv (batch, n_points, modes))"""
        phase = self.X_ * self.new_times
        forward_mat = torch.complex(torch.cos(phase), -torch.sin(phase))
        return forward_mat, forward_mat.conj().transpose(1, 2)

    def _scale(self, norm: str, divide_for: str) -> float:
        if norm == "ortho":
            return 1.0 / math.sqrt(self.number_points)
        return 1.0 / self.number_points if norm == divide_for else 1.0

    def forward(self, data: Tensor, norm: str = "forward") -> Tensor:
        """(batch, n_points, channels) complex -> (batch, modes, channels); `norm` as in ``torch.fft``"""
        return torch.matmul(self.V_fwd, data) * self._scale(norm, "forward")

    def inverse(self, data: Tensor, norm: str = "forward") -> Tensor:
        """(batch, modes, channels) complex -> (batch, n_points, channels)"""
        return torch.matmul(self.V_inv, data) * self._scale(norm, "backward")


class SpectralConv1d_SMM(nn.Module):
    """A 1-D spectral convolution: transform, one learned complex (in_channels x out_channels) mix per mode, inverse
    transform.  ``weights1`` is complex64 (in_channels, out_channels, modes), uniform in [0, 1 / (in * out)) in both
    parts."""

    def __init__(self, in_channels: int, out_channels: int, modes: int):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.modes = modes
        self.scale = 1 / (in_channels * out_channels)
        self.weights1 = nn.Parameter(self.scale * torch.rand(in_channels, out_channels, self.modes, dtype=torch.cfloat))

    def compl_mul1d(self, input: Tensor, weights: Tensor) -> Tensor:
        """(batch, in_channels, modes) x (in_channels, out_channels, modes) -> (batch, out_channels, modes)"""
        return torch.einsum("bix,iox->box", input, weights)

    def _coefficients(self, x: Tensor, transform: VFT) -> Tensor:
        x_ft = transform.forward(x.to(transform.V_fwd.dtype), norm="forward")
        weights = self.weights1.to(x_ft.dtype)      # nn.Module.double() leaves a complex parameter as it is
        return self.compl_mul1d(x_ft.permute(0, 2, 1), weights).permute(0, 2, 1)      # (batch, modes, out)

    def forward(self, x: Tensor, transform: VFT) -> Tensor:
        """(batch, n_points, in_channels) -> the real part of the convolution, (batch, n_points, out_channels)"""
        return transform.inverse(self._coefficients(x, transform), norm="forward").real

    def last_layer(self, x: Tensor, transform: VFT) -> Tensor:
        """(batch, n_points, in_channels) -> the mixed coefficients, row 2 k the real and row 2 k + 1 the imaginary
        part of mode k: (batch, 2 * modes, out_channels)"""
        return _real_rows(self._coefficients(x, transform))


class SpectralConvEmbedding(nn.Module):
    """sbi's ``SpectralConvEmbedding``: convolutions in Fourier space for 1-D data with one or more channels.

    Args:
        in_channels: channels of the input.
        modes: Fourier modes kept by every spectral convolution, at most n_points // 2 + 1.
        out_channels: channels of the output; the embedding has 2 * modes * out_channels features.
        conv_channels: channels of every layer.
        num_layers: number of (spectral + pointwise convolution, GELU) layers.

    ``force_eager = True`` on an instance pins the eager route: no sc_embed kernel is launched.
    """

    force_eager = False

    def __init__(self, in_channels: int, modes: int = 10, out_channels: int = 1, conv_channels: int = 5,
                 num_layers: int = 3):
        super().__init__()
        self.modes = modes
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.conv_channels = conv_channels
        self.num_layers = num_layers
        self.fc0 = nn.Linear(in_channels, conv_channels)
        self.conv_layers = nn.ModuleList([SpectralConv1d_SMM(conv_channels, conv_channels, modes)
                                          for _ in range(num_layers)])
        self.w_layers = nn.ModuleList([nn.Conv1d(conv_channels, conv_channels, 1) for _ in range(num_layers)])
        self.conv_last = SpectralConv1d_SMM(conv_channels, conv_channels, modes)
        self.fc_last = nn.Linear(conv_channels, out_channels)

    @property
    def dims(self) -> Dims:
        return (int(self.in_channels), int(self.modes), int(self.out_channels), int(self.conv_channels),
                int(self.num_layers))

    def kernel_parameters(self) -> List[Tensor]:
        """Every parameter in ``state_dict`` order, the kernels' flat image (complex entries as they are)."""
        return list(self.parameters())

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        if self.force_eager:
            return False, "force_eager is set"
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.ndim not in (3, 4) or (x.ndim == 4 and x.shape[1] != 2) or x.shape[-2] != self.in_channels:
            return False, "input shape is neither (batch, in_channels, n_points) nor (batch, 2, in_channels, n_points)"
        if self.modes > x.shape[-1] // 2 + 1:
            return False, "modes exceed n_points // 2 + 1"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        if not all(p.device == x.device and p.dtype == (torch.complex64 if p.is_complex() else torch.float32)
                   for p in self.parameters()):
            return False, "parameters are not float32 / complex64 on the input's device"
        rc, _ = plan(self.dims, x.shape[-1], x.shape[0], x.ndim == 4)
        if rc != 0:
            return False, plan_reason(rc)
        return True, "kernel"

    def forward(self, x: Tensor) -> Tensor:
        """(batch, in_channels, n_points), or (batch, 2, in_channels, n_points) with the positions of every channel in
        x[:, 1] (those of channel 0 are used) -> (batch, 2 * modes * out_channels)"""
        batch_size = x.shape[0]
        values, positions = _split_input(x)
        n_points = values.shape[-1]
        assert self.modes <= n_points // 2 + 1, "Modes should be at most floor(n_points/2) + 1"
        if self.kernel_route(x)[0]:
            params = [torch.view_as_real(p) if p.is_complex() else p for p in self.parameters()]
            return _SCEmbedFn.apply(x.contiguous(), self.dims, *params)
        h = self.fc0(values.permute(0, 2, 1))                            # (batch, n_points, conv_channels)
        transform = VFT(batch_size, n_points, self.modes, positions, device=h.device, dtype=h.dtype)
        for conv, w in zip(self.conv_layers, self.w_layers):
            h = torch.nn.functional.gelu(conv(h, transform) + w(h.permute(0, 2, 1)).permute(0, 2, 1))
        z = self.conv_last.last_layer(h, transform)                      # (batch, 2 * modes, conv_channels)
        return self.fc_last(z).reshape(batch_size, -1)
