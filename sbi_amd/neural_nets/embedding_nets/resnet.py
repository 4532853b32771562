"""``ResNetEmbedding1D`` / ``ResNetEmbedding2D`` -- sbi/neural_nets/embedding_nets/resnet.py (residual networks on
vectors and on images) with the 1D trunk on the resnet_embed HIP kernels.

Same signatures, defaults, messages and ``state_dict`` keys as the reference: ``initial``, then ``blocks.{i}`` with
``y = act(f(x) + downsampling(residual(x)))``, then the head ``final``.  Two routes with the same semantics:

* the eager route: the whole surface of both classes (a custom ``construct_mapping``, any activation,
  ``change_c_mode="zeros"``, all of ``ResNetEmbedding2D``, host tensors, other dtypes, double backward) -- a fallback,
  never a refusal;
* the kernel route, ``ResNetEmbedding1D`` only: ``initial`` plus every block as ONE ``torch.autograd.Function`` on
  ``sbi_amd_resnet_forward`` / ``_backward`` (include/sbi_amd_resnet.h).  It is taken for an fp32 (rows, c_in) input on
  a ROCm device that does not require grad (the kernels have no d/dx), fp32 parameters on that device,
  ``activation=nn.ReLU``, the default ``construct_mapping`` with only ``c_hidden`` in its kwargs, no
  ``residual_block_kwargs``, a shape the host-side plan accepts within ``MAX_WORKSPACE_BYTES`` and fewer rows than
  ``MAX_ROWS_TRAINING`` / ``MAX_ROWS_FORWARD``, from where on eager torch measured faster.
  ``module.kernel_route(x)`` tells which and why; ``module.force_eager = True`` pins eager.

The head ``final`` (Linear -> act -> Linear -> act -> Linear, 1000 wide by default) is ordinary torch in BOTH routes:
its GEMMs are what rocBLAS is for, and they are 5 launches against the trunk's ~140.  The bitwise row-independence
of the kernel route therefore covers the trunk output (``module.trunk(x)``), not the head.

Departure from the reference: ``ResNetEmbedding2D`` builds ``final`` on its first forward on the device and in the dtype
of the activations it sees; the reference builds it on the host in fp32 whatever the module was moved to.
"""

from __future__ import annotations

import ctypes
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Type, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets.fully_connected import flat_image, params_on, split_like

MAX_WORKSPACE_BYTES = 1 << 30
# Calls with at least this many rows run eager: (a call that needs gradients, a forward-only call).  Measured at the
# defaults (c_in 10, 20 blocks, 128 / 128, head 1000) against the module's own eager route
# (profiles/resnet_embed_bench.json); each threshold is the first measured batch size at which the kernels lost: they
# win from batch 1 to 8192 (forward + backward 3.9 x to 1.27 x, forward 3.9 x to 1.64 x) and lose at 65 536 (0.89 x and
# 0.57 x).  Nothing was measured between 8192 and 65 536.
MAX_ROWS_TRAINING = 65536
MAX_ROWS_FORWARD = 65536

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (c_in, c_internal, c_hidden <= 128, n_blocks <= 64, "
                        "rows < 2^31 - 64)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "the row tile does not fit 160 KiB of LDS",
}


# ---- the formulas, written once ----------------------------------------------------------------------------------------
def zero_pad(x: Tensor, c_out: int) -> Tensor:
    """(batch, c_in, height, width) -> (batch, c_out, height, width): the new channels are zeros."""
    if x.ndim != 4:
        raise ValueError("Only 4D input tensors are supported.")
    if c_out <= x.shape[1]:
        raise ValueError("c_out must be larger than c_in to apply zero padding.")
    fill = torch.zeros(x.shape[0], c_out - x.shape[1], x.shape[2], x.shape[3], device=x.device)
    return torch.cat([x, fill], dim=1)


def _three_layers(layer: Callable[[int, int, int], nn.Module], widths: Sequence[int],
                  activation: Type[nn.Module]) -> nn.Sequential:
    """layer(0) -> act -> layer(1) -> act -> layer(2) over widths[0] -> widths[1] -> widths[2] -> widths[3]"""
    mods: List[nn.Module] = []
    for i in range(3):
        mods.append(layer(i, widths[i], widths[i + 1]))
        if i < 2:
            mods.append(activation())
    return nn.Sequential(*mods)


def construct_simple_conv_net(c_in: int, c_out: int, c_hidden: int, activation: Type[nn.Module],
                              downsample: bool) -> nn.Module:
    """Three 3x3 convolutions c_in -> c_hidden -> c_hidden -> c_out; the first has stride 2 when `downsample`."""
    return _three_layers(
        lambda i, a, b: nn.Conv2d(a, b, kernel_size=3, stride=2 if (downsample and i == 0) else 1, padding=1),
        (c_in, c_hidden, c_hidden, c_out), activation)


def construct_simple_fc_net(c_in: int, c_out: int, c_hidden: int, activation: Type[nn.Module]) -> nn.Module:
    """Three linear layers c_in -> c_hidden -> c_hidden -> c_out."""
    return _three_layers(lambda i, a, b: nn.Linear(a, b), (c_in, c_hidden, c_hidden, c_out), activation)


def residual_step(x: Tensor, mapping: Callable, skip: Callable, act: Callable) -> Tensor:
    """y = act(mapping(x) + skip(x))"""
    return act(mapping(x) + skip(x))


def resnet_trunk_functional(x: Tensor, params: Sequence[Tensor], has_initial: bool) -> Tensor:
    """The formula the kernels implement, on the parameters in the kernels' order: initial.weight / .bias when
    present, then per block f.0.weight, f.0.bias, f.2.*, f.4.*; ReLU everywhere."""
    params = list(params)
    h = x
    if has_initial:
        h = F.linear(h, params[0], params[1])
        params = params[2:]
    for b in range(len(params) // 6):
        w0, b0, w2, b2, w4, b4 = params[6 * b:6 * b + 6]
        h = residual_step(
            h, lambda t: F.linear(F.relu(F.linear(F.relu(F.linear(t, w0, b0)), w2, b2)), w4, b4), lambda t: t, F.relu)
    return h


# ---- the kernel route ---------------------------------------------------------------------------------------------------
def resnet_config(c_in: int, c_internal: int, c_hidden: int, n_blocks: int) -> _lib.ResNetConfigC:
    cfg = _lib.ResNetConfigC()
    cfg.c_in, cfg.c_internal, cfg.c_hidden, cfg.n_blocks = int(c_in), int(c_internal), int(c_hidden), int(n_blocks)
    return cfg


def plan(cfg: _lib.ResNetConfigC, rows: int) -> Tuple[int, int, List[int], int]:
    """(rc, row tile, lds bytes of the forward and delta kernels, weight-gradient row splits): a host-side answer"""
    lds = (ctypes.c_int32 * 2)()
    tile, splits = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = int(_lib.load().sbi_amd_resnet_plan(ctypes.byref(cfg), rows, ctypes.byref(tile), lds, ctypes.byref(splits)))
    return rc, int(tile.value), [int(v) for v in lds], int(splits.value)


def plan_reason(rc: int) -> str:
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def param_count(cfg: _lib.ResNetConfigC) -> Tuple[int, List[int]]:
    entries = 6 * max(int(cfg.n_blocks), 0) + (2 if cfg.c_in != cfg.c_internal else 0)
    offsets = (ctypes.c_int64 * max(entries, 1))()
    n = int(_lib.load().sbi_amd_resnet_param_count(ctypes.byref(cfg), offsets))
    return n, [int(o) for o in offsets][:entries]


def workspace_bytes(cfg: _lib.ResNetConfigC, rows: int, training: bool) -> int:
    return int(_lib.load().sbi_amd_resnet_workspace_bytes(ctypes.byref(cfg), rows, int(training)))


class _ResNetTrunkFn(torch.autograd.Function):
    """trunk = blocks(initial(x)) on the kernels; x (rows, c_in) contiguous fp32 on the device."""

    @staticmethod
    def forward(ctx, x: Tensor, cfg, *params: Tensor) -> Tensor:
        lib = _lib.load()
        rows = x.shape[0]
        training = any(ctx.needs_input_grad[2:])
        flat = flat_image(params)
        out = torch.empty(rows, int(cfg.c_internal), dtype=torch.float32, device=x.device)
        nbytes = workspace_bytes(cfg, rows, training)
        if nbytes < 0:
            _lib.check(nbytes, "resnet_workspace_bytes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_resnet_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), rows, out.data_ptr(),
                                              ws.data_ptr(), int(training), _lib.current_stream(x.device)),
                   "resnet_forward")
        ctx.cfg = cfg
        ctx.stash = ws if training else None
        ctx.save_for_backward(x, flat, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, flat, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        cfg = ctx.cfg
        if torch.is_grad_enabled():
            # double backward (create_graph=True): differentiate the written formula instead
            with torch.enable_grad():
                wanted = [t for t, n in zip(params, need[2:]) if n]
                trunk = resnet_trunk_functional(x, params, cfg.c_in != cfg.c_internal)
                got = iter(torch.autograd.grad(trunk, wanted, grad_out, create_graph=True, allow_unused=True))
            return (None, None, *[next(got) if n else None for n in need[2:]])
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        _lib.check(_lib.load().sbi_amd_resnet_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.shape[0],
                                                       grad_out.data_ptr(), grad_flat.data_ptr(),
                                                       ctx.stash.data_ptr(), _lib.current_stream(x.device)),
                   "resnet_backward")
        grads = [g if n else None for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (None, None, *grads)


# ---- the modules ------------------------------------------------------------------------------------------------------
class ResidualBLock(nn.Module):
    """One residual block: ``y = activation(f(x) + downsampling(residual(x)))``.

    Args:
        c_in: input channels.
        c_out: output channels, ``c_in`` when None.
        is_conv_block: image-like data (4D) instead of vectors (2D).
        construct_mapping: builds ``f`` as ``construct_mapping(c_in, c_out, **construct_mapping_kwargs)``.
        construct_mapping_kwargs: its keyword arguments.
        activation: constructor of the output activation.
        downsample: halve height and width on the skip path with a strided 3x3 convolution (images only).
        change_c_mode: how the skip path changes its channel count on images: "conv" (1x1 convolution) or "zeros"
            (zero channels are appended).  Vectors use a bias-free Linear.
    """

    def __init__(self, c_in: int, c_out: Optional[int], is_conv_block: bool, construct_mapping: Callable,
                 construct_mapping_kwargs: Optional[Dict], activation: Type[nn.Module], downsample: bool = False,
                 change_c_mode: str = "conv") -> None:
        super().__init__()
        if construct_mapping_kwargs is None:
            construct_mapping_kwargs = {}
        if c_out is None:
            c_out = c_in
        if c_in == c_out:
            self.residual = nn.Identity()
        elif not is_conv_block:
            self.residual = nn.Linear(c_in, c_out, bias=False)
        elif change_c_mode == "conv":
            self.residual = nn.Conv2d(c_in, c_out, kernel_size=1, stride=1, bias=False)
        elif change_c_mode == "zeros":
            if c_in > c_out:
                raise ValueError("c_in channels must be smaller than c_out.")
            self.residual = partial(zero_pad, c_out=c_out)
        else:
            raise ValueError(f"Invalid change_c_mode {change_c_mode}.")
        if is_conv_block and downsample:
            self.downsampling = nn.Conv2d(c_out, c_out, kernel_size=3, stride=2, bias=False, padding=1)
            construct_mapping_kwargs["downsample"] = downsample
        else:
            self.downsampling = nn.Identity()
        self.f = construct_mapping(c_in, c_out, **construct_mapping_kwargs)
        self.final_activation = activation()

    def forward(self, x: Tensor) -> Tensor:
        if x.ndim not in (2, 4):
            raise ValueError("Only 2D images or 1D vectors are supported.")
        return residual_step(x, self.f, lambda t: self.downsampling(self.residual(t)), self.final_activation)


def _head(c_in: int, c_hidden: int, c_out: int, activation: Type[nn.Module]) -> List[nn.Module]:
    return list(_three_layers(lambda i, a, b: nn.Linear(a, b), (c_in, c_hidden, c_hidden, c_out), activation))


class ResNetEmbedding2D(nn.Module):
    """sbi's ``ResNetEmbedding2D``: a residual network from images to a vector.  Eager route only.

    The network is a 7x7 stride-2 convolution and a max pool, then ``n_stages`` stages of residual blocks (the last
    block of every stage but the final one halves height and width and moves to the next stage's channel count), then
    an average pool and a three-layer fully connected head that is built on the FIRST forward, when its input size is
    known: until then ``final`` is None and the ``state_dict`` has no ``final.*`` entries.

    Args:
        c_in: input channels.
        c_out: dimension of the embedding.
        c_hidden_fc: hidden units of the head.
        n_stages: number of stages.
        blocks_per_stage: residual blocks per stage, [2, 2, 2, 2] when None.
        c_stages: channels per stage, [64, 128, 256, 512] when None.
        activation: constructor of the activation.
        change_c_mode: "conv" or "zeros", see ``ResidualBLock``.
        construct_mapping: builds a block's ``f``: ``construct_mapping(c_in, c_out, activation, **kwargs)``.
        construct_mapping_kwargs: its keyword arguments ({"c_hidden": 128} when None).  The caller's dict is written
            to (``activation``, ``downsample``), as in the reference.
        residual_block_kwargs: further keyword arguments of every ``ResidualBLock``.

    Input (batch, channels, height, width) or (batch, height, width); output (batch, c_out).
    """

    def __init__(self, c_in: int, c_out: int = 20, c_hidden_fc: int = 1000, n_stages: int = 4,
                 blocks_per_stage: Optional[List] = None, c_stages: Optional[List] = None,
                 activation: Type[nn.Module] = nn.ReLU, change_c_mode: str = "conv",
                 construct_mapping: Callable = construct_simple_conv_net,
                 construct_mapping_kwargs: Optional[Dict] = None,
                 residual_block_kwargs: Optional[Dict] = None) -> None:
        super().__init__()
        if construct_mapping_kwargs is None:
            construct_mapping_kwargs = {"c_hidden": 128}
        construct_mapping_kwargs["activation"] = activation
        if residual_block_kwargs is None:
            residual_block_kwargs = {}
        if blocks_per_stage is None:
            blocks_per_stage = [2, 2, 2, 2]
        if c_stages is None:
            c_stages = [64, 128, 256, 512]
        if len(blocks_per_stage) != n_stages:
            raise ValueError("The number of stages and the number of specified block must match.")
        if len(c_stages) != n_stages:
            raise ValueError("The number of stages and the number of specified channels must match.")
        self.c_hidden_fc, self.c_out, self.activation = c_hidden_fc, c_out, activation
        self.initial = nn.Sequential(nn.Conv2d(c_in, c_stages[0], kernel_size=7, stride=2, padding=3),
                                     nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        blocks = []
        for stage, count in enumerate(blocks_per_stage):
            for j in range(count):
                widen = j == count - 1 and stage != n_stages - 1
                construct_mapping_kwargs["downsample"] = widen
                blocks.append(ResidualBLock(
                    is_conv_block=True, c_in=c_stages[stage], c_out=c_stages[stage + 1] if widen else c_stages[stage],
                    downsample=widen, change_c_mode=change_c_mode, construct_mapping=construct_mapping,
                    construct_mapping_kwargs=construct_mapping_kwargs, activation=activation,
                    **residual_block_kwargs))
        self.blocks = nn.Sequential(*blocks)
        self.final = None

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        return False, "ResNetEmbedding2D runs eager (no convolutional kernels)"

    def forward(self, x: Tensor) -> Tensor:
        if x.ndim == 3:
            x = x.unsqueeze(1)
        if x.ndim != 4:
            raise ValueError("Only 4D input tensors are supported.")
        y = self.blocks(self.initial(x))
        if self.final is None:
            features = 1
            for n in y.shape[1:]:
                features *= int(n)
            self.final = nn.Sequential(nn.AvgPool2d(kernel_size=3, stride=1, padding=1), nn.Flatten(),
                                       *_head(features, self.c_hidden_fc, self.c_out, self.activation))
            self.final.to(device=y.device, dtype=y.dtype)
        return self.final(y)


class ResNetEmbedding1D(nn.Module):
    """sbi's ``ResNetEmbedding1D``: a residual network from vectors to a vector.

    ``initial`` (a Linear c_in -> c_internal, or Identity when they are equal), ``n_blocks`` residual blocks on
    c_internal features, and the three-layer head ``final`` with ``c_hidden_final`` hidden units.

    Args:
        c_in: input dimension.
        c_out: dimension of the embedding.
        construct_mapping: builds a block's ``f``: ``construct_mapping(c_in, c_out, activation, **kwargs)``.
        construct_mapping_kwargs: its keyword arguments ({"c_hidden": 128} when None).  The caller's dict is written
            to (``activation``), as in the reference.
        residual_block_kwargs: further keyword arguments of every ``ResidualBLock``.
        n_blocks: number of residual blocks.
        c_internal: width of the residual stream.
        c_hidden_final: hidden units of the head.
        activation: constructor of the activation.

    Input (batch, c_in); output (batch, c_out).  ``force_eager = True`` on an instance pins the eager route.
    """

    force_eager = False

    def __init__(self, c_in: int, c_out: int, construct_mapping: Callable = construct_simple_fc_net,
                 construct_mapping_kwargs: Union[Dict, None] = None,
                 residual_block_kwargs: Union[Dict, None] = None, n_blocks: int = 20, c_internal: int = 128,
                 c_hidden_final: int = 1000, activation: Type[nn.Module] = nn.ReLU) -> None:
        super().__init__()
        if construct_mapping_kwargs is None:
            construct_mapping_kwargs = {"c_hidden": 128}
        default_mapping = (construct_mapping is construct_simple_fc_net
                           and set(construct_mapping_kwargs) - {"activation"} == {"c_hidden"})
        construct_mapping_kwargs["activation"] = activation
        plain_blocks = not residual_block_kwargs
        if residual_block_kwargs is None:
            residual_block_kwargs = {}
        self.initial = nn.Identity() if c_in == c_internal else nn.Linear(c_in, c_internal)
        self.final = nn.Sequential(*_head(c_internal, c_hidden_final, c_out, activation))
        self.blocks = nn.Sequential(*[
            ResidualBLock(c_in=c_internal, c_out=c_internal, is_conv_block=False, construct_mapping=construct_mapping,
                          construct_mapping_kwargs=construct_mapping_kwargs, activation=activation,
                          **residual_block_kwargs)
            for _ in range(n_blocks)])
        # what the kernel route needs to know about how the trunk was built
        self._c_in, self._c_internal = int(c_in), int(c_internal)
        self._c_hidden = int(construct_mapping_kwargs["c_hidden"]) if default_mapping else 0
        self._static_reason = (
            "activation is not nn.ReLU" if activation is not nn.ReLU else
            "a custom construct_mapping (or kwargs beyond c_hidden) runs eager" if not default_mapping else
            "residual_block_kwargs run eager" if not plain_blocks else
            "n_blocks == 0 has no trunk to run" if n_blocks < 1 else "")

    # -- routing --
    def kernel_config(self) -> _lib.ResNetConfigC:
        return resnet_config(self._c_in, self._c_internal, self._c_hidden, len(self.blocks))

    def kernel_parameters(self) -> List[Tensor]:
        """The trunk's parameters in the kernels' order: initial.*, then per block f.0.*, f.2.*, f.4.*."""
        out = list(self.initial.parameters())
        for block in self.blocks:
            out += list(block.f.parameters())
        return out

    def kernel_route(self, x: Tensor) -> Tuple[bool, str]:
        if self.force_eager:
            return False, "force_eager is set"
        if self._static_reason:
            return False, self._static_reason
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        if x.ndim != 2 or x.shape[1] != self._c_in:
            return False, "input shape is not (batch, c_in)"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        params = self.kernel_parameters()
        if not params_on(params, x):
            return False, "parameters are not float32 on the input's device"
        cfg = self.kernel_config()
        rc = plan(cfg, x.shape[0])[0]
        if rc == 0 and sum(p.numel() for p in params) != param_count(cfg)[0]:
            return False, "the trunk's modules were replaced after construction"
        if rc != 0:
            return False, plan_reason(rc)
        training = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        nbytes = workspace_bytes(cfg, x.shape[0], training)
        if nbytes > MAX_WORKSPACE_BYTES:
            return False, (f"workspace of {nbytes} bytes passes MAX_WORKSPACE_BYTES = {MAX_WORKSPACE_BYTES} "
                           "(the stash of a call that needs gradients grows with rows * n_blocks)")
        limit = MAX_ROWS_TRAINING if training else MAX_ROWS_FORWARD
        if x.shape[0] >= limit:
            return False, (f"{'a call that needs gradients' if training else 'a forward-only call'} with "
                           f"{x.shape[0]} >= {limit} rows: eager torch measured faster there "
                           "(profiles/resnet_embed_bench.json)")
        return True, "kernel"

    def trunk(self, x: Tensor) -> Tensor:
        """blocks(initial(x)), (batch, c_internal): the part the kernel route replaces."""
        if x.ndim != 2:
            raise ValueError("Only 2D input tensors are supported.")
        if self.kernel_route(x)[0]:
            return _ResNetTrunkFn.apply(x.contiguous(), self.kernel_config(), *self.kernel_parameters())
        return self.blocks(self.initial(x))

    def forward(self, x: Tensor) -> Tensor:
        return self.final(self.trunk(x))
