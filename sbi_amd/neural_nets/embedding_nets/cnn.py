"""``CNNEmbedding`` -- sbi/neural_nets/embedding_nets/cnn.py on the cnn_embed HIP kernels.

Same signature, defaults, messages and ``state_dict`` keys as the reference: ``num_conv_layers`` x [``Conv{1,2}d``
(kernel_size, stride 1, padding 1) -> ``ReLU`` -> ``MaxPool{1,2}d`` (pool_kernel_size)] as ``cnn_subnet``, a flatten,
and an ``FCEmbedding`` head as ``linear_subnet``.  The convolution stack has two routes with the same semantics:

* the eager route: ``self.cnn_subnet(x)``, the written formula;
* the kernel route: a ``torch.autograd.Function`` on ``sbi_amd_cnn_forward`` / ``_backward`` (include/sbi_amd_cnn.h):
  one launch for the whole stack forward, the parameter gradients of all conv layers backward.  It is taken for an
  fp32 input on a ROCm device that does not require grad (the kernels have no d/dx) when the parameters are fp32 on
  that device and the host-side plan accepts the shape and the batch (at most 1024 samples: beyond, eager torch
  measured faster).  Everything else runs eager -- a fallback, never a refusal.

The head keeps its own routing (``FCEmbedding.kernel_route``).  ``kernel_route(x)`` answers ``(bool, reason)`` for the
convolution stack.  The flat fp32 weight image is rebuilt from the ``nn.Conv*d`` parameters with one ``torch.cat`` per
call, so ``.to()``, ``copy.deepcopy``, ``load_state_dict`` and in-place optimizer updates need no bookkeeping.
"""

from __future__ import annotations

import ctypes
from math import prod
from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets.fully_connected import FCEmbedding, flat_image, params_on, split_like

# (ndim, in_channels, spatial, out_channels, kernel_size, pool_kernel_size)
Dims = Tuple[int, int, Tuple[int, ...], Tuple[int, ...], int, int]

MAX_KERNEL_BATCH = 1024     # CN_MAX_BATCH of csrc/cnn_embed_kernel.h

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (in_channels <= 8, out_channels <= 32, kernel_size <= 7, "
                        "2 <= pool_kernel_size <= 4, num_conv_layers <= 4)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "weights plus one sample's maps exceed 160 KiB of LDS",
}


def cnn_config(dims: Dims) -> _lib.CNNConfigC:
    ndim, cin, spatial, couts, k, pk = dims
    cfg = _lib.CNNConfigC()
    cfg.ndim, cfg.in_channels, cfg.num_conv_layers = int(ndim), int(cin), len(couts)
    cfg.kernel_size, cfg.pool_kernel_size = int(k), int(pk)
    for i, n in enumerate(spatial[:2]):
        cfg.spatial[i] = int(n)
    for i, c in enumerate(couts[:4]):
        cfg.out_channels[i] = int(c)
    return cfg


def plan(dims: Dims, batch: int) -> int:
    """0 when the kernels take `batch` samples through a stack of these sizes, else E_* (a host-side answer)."""
    if batch < 1:
        return _lib.E_BADARG
    if len(dims[3]) > 4:
        return _lib.E_UNSUPPORTED
    return int(_lib.load().sbi_amd_cnn_plan(ctypes.byref(cnn_config(dims)), batch, None, None))


def plan_reason(rc: int, batch: int = 1) -> str:
    if rc == _lib.E_UNSUPPORTED and batch > MAX_KERNEL_BATCH:
        return f"batch above {MAX_KERNEL_BATCH}: eager torch measured faster there"
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def feature_count(dims: Dims) -> int:
    return int(_lib.load().sbi_amd_cnn_feature_count(ctypes.byref(cnn_config(dims))))


def param_count(dims: Dims) -> int:
    return int(_lib.load().sbi_amd_cnn_param_count(ctypes.byref(cnn_config(dims)), None))


def cnn_functional(x: Tensor, params: Sequence[Tensor], pool_kernel_size: int) -> Tensor:
    """max_pool(relu(conv(x))) layer by layer on (weight, bias, ...), flattened: the formula the kernels implement."""
    two = params[0].dim() == 4
    conv = torch.nn.functional.conv2d if two else torch.nn.functional.conv1d
    pool = torch.nn.functional.max_pool2d if two else torch.nn.functional.max_pool1d
    for w, b in zip(params[0::2], params[1::2]):
        x = pool(torch.relu(conv(x, w, b, stride=1, padding=1)), pool_kernel_size)
    return x.reshape(x.shape[0], -1)


class _CNNEmbedFn(torch.autograd.Function):
    """features = flatten(cnn_subnet(x)) on the kernels; x (B, C, spatial...) contiguous fp32 on the device."""

    @staticmethod
    def forward(ctx, x: Tensor, dims: Dims, *params: Tensor) -> Tensor:
        lib = _lib.load()
        cfg = cnn_config(dims)
        flat = flat_image(params)
        out = torch.empty(x.shape[0], feature_count(dims), dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_cnn_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.shape[0],
                                           out.data_ptr(), _lib.current_stream(x.device)), "cnn_forward")
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
                got = iter(torch.autograd.grad(cnn_functional(x, params, dims[5]), wanted, grad_out, create_graph=True))
            return (None, None, *[next(got) if n else None for n in need[2:]])
        lib = _lib.load()
        cfg = cnn_config(dims)
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        nbytes = int(lib.sbi_amd_cnn_workspace_bytes(ctypes.byref(cfg), x.shape[0]))
        if nbytes < 0:
            _lib.check(nbytes, "cnn_workspace_bytes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_cnn_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.shape[0],
                                            grad_out.data_ptr(), grad_flat.data_ptr(), ws.data_ptr(),
                                            _lib.current_stream(x.device)), "cnn_backward")
        grads = [g if n else None for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (None, None, *grads)


def _validate_cnn_input_shape(x: Tensor, input_shape: Tuple) -> None:
    """ValueError unless x's trailing shape is the channel-first shape, its flat size, or (one channel) the bare
    spatial shape (the reference's check and message)."""
    trailing_shape = tuple(x.shape[1:])
    valid_shapes = (input_shape, (prod(input_shape),))
    if input_shape[0] == 1:
        valid_shapes += (input_shape[1:],)
    if trailing_shape not in valid_shapes:
        raise ValueError("Expected flat or channel-first input with trailing shape "
                         f"in {valid_shapes}, but got {trailing_shape}.")


def calculate_filter_output_size(input_size, padding, dilation, kernel, stride) -> int:
    """Output extent of a convolution or pooling filter (the formula of torch's Conv2d documentation)."""
    span = int(input_size) + 2 * int(padding) - int(dilation) * (int(kernel) - 1) - 1
    return int(span / int(stride) + 1)


def get_new_cnn_output_size(input_shape: Tuple, conv_layer: Union[nn.Conv1d, nn.Conv2d],
                            pool: Union[nn.MaxPool1d, nn.MaxPool2d]) -> Union[Tuple[int], Tuple[int, int]]:
    """Spatial shape after `conv_layer` and then `pool` are applied to a map of `input_shape`."""
    assert isinstance(input_shape, Tuple), "input shape must be Tuple."
    assert 0 < len(input_shape) < 3, "input shape must be 1 or 2d."
    assert isinstance(conv_layer.padding, Tuple), "conv layer attributes must be Tuple."
    assert isinstance(pool.padding, int), "pool layer attributes must be integers."
    out = []
    for i, n in enumerate(input_shape):
        after_conv = calculate_filter_output_size(n, conv_layer.padding[i], conv_layer.dilation[i],
                                                  conv_layer.kernel_size[i], conv_layer.stride[i])
        out.append(calculate_filter_output_size(after_conv, pool.padding, pool.dilation, pool.kernel_size, pool.stride))
    return tuple(out)


_SHAPE_MESSAGE = "input_shape must be a Tuple of size 1 or 2, e.g., (width, [height])."
_SHAPE_MESSAGE_LONG = ("input_shape must be a Tuple of size 1 or 2, e.g.,\n"
                       "            (width, [height]). Number of input channels are passed separately")


def _zero_size_message(layer: int) -> str:
    return (f"CNN output size is zero at layer {layer + 1}. Either reduce\n"
            f"                 num_cnn_layers to {layer} or adjust the kernel_size\n"
            "                 and pool_kernel_size accordingly.")


class CNNEmbedding(nn.Module):
    """sbi's ``CNNEmbedding``: a 1-D or 2-D convolution stack (by ``len(input_shape)``) and an ``FCEmbedding`` head.

    Args:
        input_shape: spatial shape without batch or channel dimensions, e.g. (28,) or (28, 28).  Inputs may be flat,
            channel-first, or (one channel) bare spatial.
        in_channels: number of input channels.
        out_channels_per_layer: output channels of every conv layer ([6, 12] by default); as many as num_conv_layers.
        num_conv_layers: number of conv -> ReLU -> max-pool blocks.
        num_linear_layers, num_linear_units, output_dim: sizes of the ``FCEmbedding`` head.
        kernel_size: kernel size of every convolution (stride 1, padding 1).
        pool_kernel_size: window and stride of every max-pool.

    ``force_eager = True`` on an instance pins the eager route all the way down: the convolutions run
    ``self.cnn_subnet`` and the head its ``nn.Sequential``; no cnn or embed kernel is launched.
    """

    force_eager = False

    def __init__(self, input_shape: Tuple, in_channels: int = 1, out_channels_per_layer: Optional[List] = None,
                 num_conv_layers: int = 2, num_linear_layers: int = 2, num_linear_units: int = 50,
                 output_dim: int = 20, kernel_size: int = 5, pool_kernel_size: int = 2):
        super().__init__()
        assert isinstance(input_shape, Tuple), _SHAPE_MESSAGE
        assert 0 < len(input_shape) < 3, _SHAPE_MESSAGE_LONG
        two = len(input_shape) == 2
        conv_module, pool_module = (nn.Conv2d, nn.MaxPool2d) if two else (nn.Conv1d, nn.MaxPool1d)
        if out_channels_per_layer is None:
            out_channels_per_layer = [6, 12]
        assert len(out_channels_per_layer) == num_conv_layers, "out_channels needs as many entries as num_cnn_layers."
        self.input_shape = (in_channels, *input_shape)

        layers: List[nn.Module] = []
        size = input_shape
        for i in range(num_conv_layers):
            conv = conv_module(in_channels=in_channels if i == 0 else out_channels_per_layer[i - 1],
                               out_channels=out_channels_per_layer[i], kernel_size=kernel_size, stride=1, padding=1)
            pool = pool_module(kernel_size=pool_kernel_size)
            layers += [conv, nn.ReLU(inplace=True), pool]
            size = get_new_cnn_output_size(size, conv, pool)
            assert all(size), _zero_size_message(i)
        self.cnn_subnet = nn.Sequential(*layers)
        self.linear_subnet = FCEmbedding(input_dim=int(out_channels_per_layer[-1]) * prod(int(n) for n in size),
                                         output_dim=output_dim, num_layers=num_linear_layers,
                                         num_hiddens=num_linear_units)
        self._dims: Dims = (len(input_shape), int(in_channels), tuple(int(n) for n in input_shape),
                            tuple(int(c) for c in out_channels_per_layer), int(kernel_size), int(pool_kernel_size))

    @property
    def dims(self) -> Dims:
        return self._dims

    def conv_parameters(self) -> List[Tensor]:
        """(weight, bias) of every convolution in ``state_dict`` order: the kernels' flat image."""
        out: List[Tensor] = []
        for m in self.cnn_subnet:
            if isinstance(m, (nn.Conv1d, nn.Conv2d)):
                out += [m.weight, m.bias]
        return out

    def static_route(self) -> Tuple[bool, str]:
        """The part of the routing decision that does not depend on the input."""
        if self.force_eager:
            return False, "force_eager is set"
        return True, "kernel"

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        ok, why = self.static_route()
        if not ok:
            return ok, why
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.dim() < 2 or x.numel() != x.shape[0] * prod(self.input_shape):
            return False, "input shape does not match input_shape"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        if not params_on(self.conv_parameters(), x):
            return False, "parameters are not float32 on the input's device"
        rc = plan(self._dims, x.shape[0])
        if rc != 0:
            return False, plan_reason(rc, x.shape[0])
        return True, "kernel"

    def features(self, x: Tensor) -> Tensor:
        """The convolution stack alone: x in any accepted layout -> (batch_size, F), flattened channel-major."""
        batch_size = x.size(0)
        _validate_cnn_input_shape(x, self.input_shape)
        x = x.reshape(batch_size, *self.input_shape)      # also gives single-channel data its channel dimension
        if self.kernel_route(x)[0]:
            return _CNNEmbedFn.apply(x.contiguous(), self._dims, *self.conv_parameters())
        return self.cnn_subnet(x).reshape(batch_size, -1)

    def forward(self, x: Tensor) -> Tensor:
        """Network forward pass: (batch_size, [channels,] *input_shape) or flat -> (batch_size, output_dim)."""
        features = self.features(x)
        if self.force_eager:
            return self.linear_subnet.net(features)
        return self.linear_subnet(features)
