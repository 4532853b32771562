"""fp64 restatement of sbi's ResNetEmbedding1D / ResNetEmbedding2D, written from the published definition (He et al.
2015 residual blocks as sbi arranges them), on a ``state_dict`` alone: no module of the package is used.

1D:  h = x Wi^T + bi (when ``initial.weight`` exists);  per block  h <- act(f(h) + h)  with
     f = Linear -> act -> Linear -> act -> Linear (``blocks.i.f.{0,2,4}``);  out = head(h), the head being
     Linear -> act -> Linear -> act -> Linear (``final.{0,2,4}``).
2D:  h = maxpool3s2p1(conv7s2p3(x));  per block  h <- act(f(h) + down(skip(h)))  with f three 3x3 convolutions (the first
     with stride 2 in a downsampling block), skip the identity, a bias-free 1x1 convolution (``residual.weight``) or
     appended zero channels, down the identity or a bias-free 3x3 stride-2 convolution (``downsampling.weight``);
     out = head(flatten(avgpool3s1p1(h))) (``final.{2,4,6}``).
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

KINK_MARGIN = 64 * 2.0**-24


def _act(kwargs: dict):
    name = kwargs.get("activation", "ReLU")
    return {"ReLU": torch.relu, "Tanh": torch.tanh}[name]


def _leaves(state_dict: Dict[str, Tensor]) -> Dict[str, Tensor]:
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in state_dict.items()}


def _n_blocks(sd) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def forward_1d(sd: Dict[str, Tensor], x: Tensor, kwargs: dict, pre: Optional[List[Tensor]] = None,
               operands: Optional[Dict[str, Tuple[Tensor, Tensor]]] = None) -> Tuple[Tensor, Tensor]:
    """(trunk, out) in the dtype of `sd`; `pre` collects every activation's input (rows first); `operands` collects per
    Linear (its name without ".weight") the pair (input, output)"""
    act = _act(kwargs)

    def a(t):
        if pre is not None:
            pre.append(t)
        return act(t)

    def lin(name, t):
        z = t @ sd[name + ".weight"].T + sd[name + ".bias"]
        if operands is not None:
            operands[name] = (t, z)
        return z

    h = x
    if "initial.weight" in sd:
        h = lin("initial", h)
    for i in range(_n_blocks(sd)):
        p = f"blocks.{i}.f."
        u = a(lin(p + "0", h))
        u = a(lin(p + "2", u))
        h = a(lin(p + "4", u) + h)
    trunk = h
    u = a(lin("final.0", h))
    u = a(lin("final.2", u))
    return trunk, lin("final.4", u)


def forward_2d(sd: Dict[str, Tensor], x: Tensor, kwargs: dict) -> Tensor:
    act = _act(kwargs)
    if x.ndim == 3:
        x = x[:, None]
    h = F.max_pool2d(F.conv2d(x, sd["initial.0.weight"], sd["initial.0.bias"], stride=2, padding=3), 3, 2, 1)
    for i in range(_n_blocks(sd)):
        p = f"blocks.{i}."
        down = p + "downsampling.weight" in sd
        u = act(F.conv2d(h, sd[p + "f.0.weight"], sd[p + "f.0.bias"], stride=2 if down else 1, padding=1))
        u = act(F.conv2d(u, sd[p + "f.2.weight"], sd[p + "f.2.bias"], padding=1))
        u = F.conv2d(u, sd[p + "f.4.weight"], sd[p + "f.4.bias"], padding=1)
        skip = h
        if p + "residual.weight" in sd:
            skip = F.conv2d(skip, sd[p + "residual.weight"])
        elif u.shape[1] != h.shape[1]:
            skip = torch.cat([skip, skip.new_zeros(h.shape[0], u.shape[1] - h.shape[1], *h.shape[2:])], dim=1)
        if down:
            skip = F.conv2d(skip, sd[p + "downsampling.weight"], stride=2, padding=1)
        h = act(u + skip)
    h = F.avg_pool2d(h, 3, 1, 1).flatten(1)
    u = act(h @ sd["final.2.weight"].T + sd["final.2.bias"])
    u = act(u @ sd["final.4.weight"].T + sd["final.4.bias"])
    return u @ sd["final.6.weight"].T + sd["final.6.bias"]


def is_2d(sd) -> bool:
    return "initial.0.weight" in sd


def reference(state_dict: Dict[str, Tensor], x: Tensor, wts: Tensor, kwargs: dict
              ) -> Tuple[Optional[Tensor], Tensor, Tensor]:
    """(trunk or None, out, flat gradient of sum(out * wts) in state_dict order), all fp64 on the host"""
    sd = _leaves({k: v.cpu() for k, v in state_dict.items()})
    xd = x.detach().double().cpu()
    if is_2d(sd):
        trunk, out = None, forward_2d(sd, xd, kwargs)
    else:
        trunk, out = forward_1d(sd, xd, kwargs)
    grads = torch.autograd.grad((out * wts.detach().double().cpu()).sum(), list(sd.values()), allow_unused=True)
    flat = torch.cat([(g if g is not None else torch.zeros_like(v)).reshape(-1) for g, v in zip(grads, sd.values())])
    return (None if trunk is None else trunk.detach()), out.detach(), flat


def reference_with_operands(state_dict: Dict[str, Tensor], x: Tensor, wts: Tensor, kwargs: dict
                            ) -> Tuple[Tensor, Tensor, Tensor, Dict[str, Tuple[Tensor, Tensor]]]:
    """`reference` of a 1D net, and per Linear (its name without ".weight") the fp64 pair (A, D): its input (rows, K) and
    the gradient of sum(out * wts) with respect to its output (rows, N).  Row r alone contributes the outer product
    D[r]^T A[r] to the weight's gradient and D[r] to the bias's."""
    sd = _leaves({k: v.cpu() for k, v in state_dict.items()})
    operands: Dict[str, Tuple[Tensor, Tensor]] = {}
    trunk, out = forward_1d(sd, x.detach().double().cpu(), kwargs, operands=operands)
    outputs = [z for _, z in operands.values()]
    grads = torch.autograd.grad((out * wts.detach().double().cpu()).sum(), list(sd.values()) + outputs,
                                allow_unused=True)
    grads = [torch.zeros_like(v) if g is None else g for g, v in zip(grads, list(sd.values()) + outputs)]
    flat = torch.cat([g.reshape(-1) for g in grads[:len(sd)]])
    pairs = {name: (a.detach(), d) for (name, (a, _)), d in zip(operands.items(), grads[len(sd):])}
    return trunk.detach(), out.detach(), flat, pairs


def near_kink_rows(state_dict: Dict[str, Tensor], x: Tensor, kwargs: dict) -> List[int]:
    """Rows of a 1D ReLU net with any ReLU input (both hidden ones and the output one of every block, the head's two)
    within 64 * 2^-24 * max|that layer's inputs| of 0, decided in fp64."""
    sd = {k: v.detach().double().cpu() for k, v in state_dict.items()}
    pre: List[Tensor] = []
    forward_1d(sd, x.detach().double().cpu(), kwargs, pre)
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for t in pre:
        near |= (t.abs() <= KINK_MARGIN * t.abs().max()).any(dim=1)
    return [int(i) for i in torch.nonzero(near).flatten()]


def flat_grad(module) -> Tensor:
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                      for p in module.parameters()])
