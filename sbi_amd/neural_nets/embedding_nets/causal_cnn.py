"""``CausalCNNEmbedding`` -- sbi/neural_nets/embedding_nets/causal_cnn.py (a WaveNet-style embedding for long raw
traces) on the causal_cnn HIP kernels.

Same signatures, defaults, messages and ``state_dict`` keys as the reference: ``causal_cnns``, a stack of
[``causalConv1d`` (left zero-pad -> dilated ``Conv1d``) -> activation], an ``AvgPool1d`` as ``pooling_layer``, and
``aggregation``, by default ``WaveNetSRLikeAggregator`` (non-causal convolutions, max-pools, a global average).  The
causal stack and the pool have two routes with the same semantics:

* the eager route: ``self.pooling_layer(self.causal_cnns(x))``, the written formula;
* the kernel route: a ``torch.autograd.Function`` on ``sbi_amd_ccnn_forward`` / ``_backward``
  (include/sbi_amd_causal_cnn.h) that returns ``features`` (B, C_last, T // pool_kernel_size): one launch forward, one
  and a reduction backward, whatever T; no per-layer (B, C, T) map exists.  It is taken for an fp32 input on a ROCm
  device that does not require grad (the kernels have no d/dx), when the parameters are fp32 on that device, the
  activation is ``nn.LeakyReLU`` or ``nn.ReLU`` and the host-side plan accepts the shape.  Everything else runs eager
  -- a fallback, never a refusal.

``aggregation`` sees T // pool_kernel_size steps and is ordinary torch on both routes, so any module can be passed.
Departures from the reference: building the default aggregator prints nothing, and a caller's
``intermediate_channel_sizes`` list is not changed.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets.cnn import _validate_cnn_input_shape, calculate_filter_output_size
from sbi_amd.neural_nets.embedding_nets.fully_connected import flat_image, params_on, split_like

# (in_channels, T, out_channels, dilations, kernel_size, pool_kernel_size, negative_slope)
Dims = Tuple[int, int, Tuple[int, ...], Tuple[int, ...], int, int, float]

MAX_LAYERS = 16             # CC_MAX_LAYERS of csrc/causal_cnn_kernel.h
CYCLE = 10                  # "exponential_cyclic" starts again at dilation 1 after 2^9

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (channels <= 32, 2 <= kernel_size <= 4, num_conv_layers <= "
                        "16, T <= 2^20, B C T < 2^31, negative_slope >= 0)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "no time tile as long as the receptive field fits 160 KiB of LDS",
}


def ccnn_config(dims: Dims) -> _lib.CausalCNNConfigC:
    cin, T, couts, dils, k, pool, slope = dims
    cfg = _lib.CausalCNNConfigC()
    cfg.in_channels, cfg.T, cfg.num_conv_layers = int(cin), int(T), len(couts)
    cfg.kernel_size, cfg.pool_kernel_size, cfg.negative_slope = int(k), int(pool), float(slope)
    for i, (c, d) in enumerate(zip(couts[:MAX_LAYERS], dils[:MAX_LAYERS])):
        cfg.out_channels[i], cfg.dilation[i] = int(c), int(d)
    return cfg


def plan(dims: Dims, batch: int) -> Tuple[int, int]:
    """(rc, tile_steps): rc is 0 when the kernels take `batch` sequences through a stack of these sizes, else E_*;
    tile_steps is the time-tile length the plan chose (0 without one).  A host-side answer."""
    if batch < 1:
        return _lib.E_BADARG, 0
    if len(dims[2]) > MAX_LAYERS or len(dims[2]) != len(dims[3]):
        return _lib.E_UNSUPPORTED, 0
    tile = ctypes.c_int32(0)
    rc = int(_lib.load().sbi_amd_ccnn_plan(ctypes.byref(ccnn_config(dims)), batch, ctypes.byref(tile), None, None))
    return rc, int(tile.value)


def plan_reason(rc: int) -> str:
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def param_count(dims: Dims) -> int:
    return int(_lib.load().sbi_amd_ccnn_param_count(ctypes.byref(ccnn_config(dims)), None))


def receptive_field(dims: Dims) -> int:
    return sum(int(d) * (int(dims[4]) - 1) for d in dims[3])


def causal_functional(x: Tensor, params: Sequence[Tensor], dims: Dims) -> Tensor:
    """avg_pool(leaky_relu(conv(left-padded x)) layer by layer) on (weight, bias, ...): the formula the kernels
    implement"""
    _, _, _, dils, k, pool, slope = dims
    for w, b, d in zip(params[0::2], params[1::2], dils):
        x = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (d * (k - 1), 0)), w, b, dilation=d)
        x = torch.nn.functional.leaky_relu(x, slope)
    return torch.nn.functional.avg_pool1d(x, pool)


class _CausalCNNEmbedFn(torch.autograd.Function):
    """features = avg_pool(causal_cnns(x)) on the kernels; x (B, C, T) contiguous fp32 on the device."""

    @staticmethod
    def forward(ctx, x: Tensor, dims: Dims, *params: Tensor) -> Tensor:
        lib = _lib.load()
        cfg = ccnn_config(dims)
        flat = flat_image(params)
        out = torch.empty(x.shape[0], dims[2][-1], dims[1] // dims[5], dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_ccnn_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.shape[0],
                                            out.data_ptr(), _lib.current_stream(x.device)), "ccnn_forward")
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
                got = iter(torch.autograd.grad(causal_functional(x, params, dims), wanted, grad_out, create_graph=True))
            return (None, None, *[next(got) if n else None for n in need[2:]])
        lib = _lib.load()
        cfg = ccnn_config(dims)
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        nbytes = int(lib.sbi_amd_ccnn_workspace_bytes(ctypes.byref(cfg), x.shape[0]))
        if nbytes < 0:
            _lib.check(nbytes, "ccnn_workspace_bytes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_ccnn_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.shape[0],
                                             grad_out.data_ptr(), grad_flat.data_ptr(), ws.data_ptr(),
                                             _lib.current_stream(x.device)), "ccnn_backward")
        grads = [g if n else None for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (None, None, *grads)


# ---- the modules ------------------------------------------------------------------------------------------------------
def causalConv1d(in_channels: int, out_channels: int, kernel_size: int, dilation: int = 1,
                 stride: int = 1) -> nn.Module:
    """A causal 1-D convolution: the input is padded on the left by dilation (kernel_size - 1) zeros, so that output
    step t sees input steps <= t only and (at stride 1) the length is kept.  Stride and dilation cannot both exceed 1.
    Returns ``nn.Sequential(pad, conv)``."""
    assert not (dilation > 1 and stride > 1), "we don't allow combining stride with dilation."
    pad = nn.ZeroPad1d((dilation * (kernel_size - 1), 0))
    conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride=stride, padding=0, dilation=dilation)
    return nn.Sequential(pad, conv)


def WaveNetSRLikeAggregator(in_channels: int, num_timepoints: int, output_dim: int,
                            activation: nn.Module = nn.LeakyReLU(inplace=True), kernel_sizes: Optional[List] = None,
                            intermediate_channel_sizes: Optional[List] = None,
                            stride_sizes: Union[int, List] = 1) -> nn.Module:
    """The non-causal aggregator of WaveNet's speech-recognition variant: [``Conv1d`` (padding "same") -> activation ->
    ``MaxPool1d`` (2, or 1 once at most two steps are left)] per entry of `kernel_sizes`, then a global average, so the
    output is (batch, output_dim, 1) whatever the input length.

    Args:
        in_channels, num_timepoints: shape of the input (batch, in_channels, num_timepoints).
        output_dim: channels of the last convolution, the number of features.
        activation: module applied after every convolution.
        kernel_sizes: one kernel size per convolution; two by default, min(9, n) and min(5, n // 2).
        intermediate_channel_sizes: channels between the convolutions ([64] by default), one entry fewer than
            `kernel_sizes`.  The list is not changed.
        stride_sizes: one stride for all convolutions, or one per convolution.
    """
    if kernel_sizes is None:
        kernel_sizes = [min(9, num_timepoints), min(5, int(num_timepoints / 2))]
    if intermediate_channel_sizes is None:
        intermediate_channel_sizes = [64]
    assert len(intermediate_channel_sizes) == len(kernel_sizes) - 1, (
        "Provided kernel size list should be exactly one element longer than channel size list.")
    channels = [in_channels, *intermediate_channel_sizes, output_dim]
    if isinstance(stride_sizes, List):
        assert len(stride_sizes) == len(kernel_sizes), (
            "Provided stride size list should be have the same size asthe kernel size list.")
    else:
        stride_sizes = [stride_sizes] * len(kernel_sizes)

    layers: List[nn.Module] = []
    steps = num_timepoints
    for i, (k, s) in enumerate(zip(kernel_sizes, stride_sizes)):
        layers += [nn.Conv1d(channels[i], channels[i + 1], kernel_size=k, stride=s, padding="same"), activation,
                   nn.MaxPool1d(kernel_size=2 if steps > 2 else 1)]
        steps = int(calculate_filter_output_size(steps, (k - 1) / 2, 1, k, s) / 2)
    return nn.Sequential(*layers, nn.AdaptiveAvgPool1d(1))


def _dilations(dilation: Union[str, List], num_conv_layers: int) -> List[int]:
    if not isinstance(dilation, str):
        assert isinstance(dilation, List), "Please pass dilation size as list or a string option."
        return dilation
    scheme = dilation.lower()
    if scheme == "exponential_cyclic":
        return [2 ** (i % CYCLE) for i in range(num_conv_layers)]
    if scheme == "exponential":
        return [2 ** i for i in range(num_conv_layers)]
    if scheme == "none":
        return [1] * num_conv_layers
    raise ValueError(f"{dilation} is not a valid option, please use \"none\",\"exponential\",or "
                     "\"exponential_cyclic\", or pass a list of dilation sizes.")


class CausalCNNEmbedding(nn.Module):
    """sbi's ``CausalCNNEmbedding``: dilated causal 1-D convolutions over a long series, an average pool, and an
    aggregator that brings the pooled map down to a feature vector.

    Args:
        input_shape: (num_timepoints,), without batch or channel dimensions.  Inputs may be flat, channel-first, or
            (one channel) bare (batch, num_timepoints).
        in_channels: number of input channels.
        out_channels_per_layer: output channels of every causal layer (16 each by default); num_conv_layers entries.
        dilation: "none" (1 everywhere), "exponential" (1, 2, 4, ...), "exponential_cyclic" (exponential, back to 1
            after 2^9: WaveNet's scheme, the default) or a list with one dilation per layer.
        num_conv_layers: number of causal layers.
        activation: module applied after every causal convolution; ``nn.LeakyReLU`` and ``nn.ReLU`` run on the
            kernels, any other module on the eager route.
        pool_kernel_size: window and stride of the ``AvgPool1d`` behind the causal stack.
        kernel_size: kernel size of every causal convolution.
        aggregator: module (batch, C_last, T // pool_kernel_size) -> features; ``WaveNetSRLikeAggregator`` by default.
        output_dim: number of features of the default aggregator.

    ``force_eager = True`` on an instance pins the eager route: no causal_cnn kernel is launched.
    """

    force_eager = False

    def __init__(self, input_shape: Tuple, in_channels: int = 1, out_channels_per_layer: Optional[List] = None,
                 dilation: Union[str, List] = "exponential_cyclic", num_conv_layers: int = 5,
                 activation: nn.Module = nn.LeakyReLU(inplace=True), pool_kernel_size: int = 160, kernel_size: int = 2,
                 aggregator: Optional[nn.Module] = None, output_dim: int = 20):
        super().__init__()
        assert isinstance(input_shape, Tuple), "input_shape must be a Tuple of size 1, e.g. (timepoints,)."
        assert len(input_shape) == 1, "Currently only 1D causal CNNs are supported."
        self.input_shape = (in_channels, *input_shape)
        steps = input_shape[0]
        assert steps >= pool_kernel_size, ("Please ensure that the pool kernel size is not larger than the number of "
                                           "observed timepoints.")
        dilations = _dilations(dilation, num_conv_layers)
        assert max(dilations) < steps, ("Your maximal dilations size used is larger than the number of timepoints in "
                                        "your input, please provide a list with smaller dilations.")
        if out_channels_per_layer is None:
            out_channels_per_layer = [16] * num_conv_layers
        widths = [in_channels, *out_channels_per_layer]

        stack: List[nn.Module] = []
        for i in range(num_conv_layers):
            stack += [causalConv1d(widths[i], widths[i + 1], kernel_size, dilations[i], 1), activation]
        self.causal_cnns = nn.Sequential(*stack)
        self.pooling_layer = nn.AvgPool1d(kernel_size=pool_kernel_size)
        if aggregator is None:
            pooled_steps = int(steps / pool_kernel_size)
            assert pooled_steps > 1, ("Your dimensionality is already small,Please ensure a larger input size or use a "
                                      "custom aggregator.")
            aggregator = WaveNetSRLikeAggregator(out_channels_per_layer[-1], pooled_steps, output_dim=output_dim)
        self.aggregation = aggregator

        if isinstance(activation, nn.LeakyReLU):
            self._slope: Optional[float] = float(activation.negative_slope)
        elif isinstance(activation, nn.ReLU):
            self._slope = 0.0
        else:
            self._slope = None
        self._dims: Dims = (int(in_channels), int(steps), tuple(int(c) for c in out_channels_per_layer[:num_conv_layers]),
                            tuple(int(d) for d in dilations[:num_conv_layers]), int(kernel_size), int(pool_kernel_size),
                            0.0 if self._slope is None else self._slope)

    @property
    def dims(self) -> Dims:
        return self._dims

    def conv_parameters(self) -> List[Tensor]:
        """(weight, bias) of every causal convolution in ``state_dict`` order: the kernels' flat image."""
        out: List[Tensor] = []
        for m in self.causal_cnns:
            if isinstance(m, nn.Sequential):
                out += [m[1].weight, m[1].bias]
        return out

    def static_route(self) -> Tuple[bool, str]:
        """The part of the routing decision that does not depend on the input."""
        if self.force_eager:
            return False, "force_eager is set"
        if self._slope is None:
            return False, "activation is neither nn.LeakyReLU nor nn.ReLU"
        return True, "kernel"

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        ok, why = self.static_route()
        if not ok:
            return ok, why
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.dim() < 2 or x.numel() != x.shape[0] * self.input_shape[0] * self.input_shape[1]:
            return False, "input shape does not match input_shape"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        if not params_on(self.conv_parameters(), x):
            return False, "parameters are not float32 on the input's device"
        rc, _ = plan(self._dims, x.shape[0])
        if rc != 0:
            return False, plan_reason(rc)
        return True, "kernel"

    def features(self, x: Tensor) -> Tensor:
        """The pooled output of the causal stack: x in any accepted layout -> (batch, C_last, T // pool_kernel_size)."""
        batch_size = x.size(0)
        _validate_cnn_input_shape(x, self.input_shape)
        x = x.reshape(batch_size, *self.input_shape)      # also gives single-channel data its channel dimension
        if self.kernel_route(x)[0]:
            return _CausalCNNEmbedFn.apply(x.contiguous(), self._dims, *self.conv_parameters())
        return self.pooling_layer(self.causal_cnns(x))

    def forward(self, x: Tensor) -> Tensor:
        """(batch, [channels,] num_timepoints) or flat -> (batch, features of the aggregator, flattened)."""
        return self.aggregation(self.features(x)).reshape(x.size(0), -1)
