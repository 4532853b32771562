"""fp64 restatement of CausalCNNEmbedding's causal stack + average pool and of its parameter gradient, written from
the definition with explicit taps and an explicit backward pass (no conv1d, no autograd): the reference of the kernel
parity tests.  tests/test_causal_cnn_embedding_cpu.py checks it against autograd of the fp64 eager formula.

Layer l: u[b, o, t] = bias[o] + sum_{c, j} w[o, c, j] y[b, c, t - (k - 1 - j) d_l] with y = 0 left of t = 0, then
a = u if u > 0 else slope u.  pooled[b, o, p] = mean of a[b, o, p pool : (p + 1) pool]; the last T mod pool steps are
dropped.  The derivative of the activation at u <= 0 is slope.

The kink.  The gradient is discontinuous in u at 0: an fp32 route whose rounding puts a pre-activation on the other
side of 0 than fp64 does has taken the other one-sided derivative, and one such step moves the gradient by far more
than any rounding bound.  Both sides are right within S = |bias| + sum |w| |y|, the scale of the sum, times the
rounding of a dot product; `reference(..., positive=...)` therefore takes the side a route took (the signs of its own
layer outputs), and `kink_disagreements` says whether every step where that differs from fp64 lies within 32 * 2^-24 S
of the kink (the margin of tests/cnn_embedding_oracle.py)."""
import torch


def conv_params(state_dict, num_layers):
    """[(weight, bias)] of the causal convolutions out of a CausalCNNEmbedding state_dict, in fp64"""
    return [(state_dict[f"causal_cnns.{2 * l}.1.weight"].detach().double().cpu(),
             state_dict[f"causal_cnns.{2 * l}.1.bias"].detach().double().cpu()) for l in range(num_layers)]


def _padded(y, d, k):
    return torch.cat([torch.zeros(*y.shape[:2], d * (k - 1), dtype=y.dtype), y], dim=-1)


def forward(layers, x, dilations, pool, slope):
    """(pooled, [padded input of every layer], [pre-activation of every layer])"""
    y = x.detach().double().cpu()
    T = y.shape[-1]
    inputs, pre = [], []
    for (w, b), d in zip(layers, dilations):
        k = w.shape[-1]
        yp = _padded(y, d, k)
        u = b[None, :, None].expand(y.shape[0], -1, T).clone()
        for j in range(k):
            u += torch.einsum("oc,bct->bot", w[:, :, j], yp[..., j * d:j * d + T])
        inputs.append(yp)
        pre.append(u)
        y = torch.where(u > 0, u, slope * u)
    Tp = T // pool
    pooled = y[..., :Tp * pool].reshape(*y.shape[:2], Tp, pool).mean(dim=-1)
    return pooled, inputs, pre


def kink_disagreements(layers, x, dilations, slope, positive):
    """(steps where positive[l] differs from u > 0, those of them further than 32 * 2^-24 S from the kink)"""
    _, inputs, pre = forward(layers, x, dilations, 1, slope)
    differ = far = 0
    for (w, b), d, yp, u, pos in zip(layers, dilations, inputs, pre, positive):
        T = u.shape[-1]
        S = b.abs()[None, :, None].expand_as(u).clone()
        for j in range(w.shape[-1]):
            S += torch.einsum("oc,bct->bot", w[:, :, j].abs(), yp[..., j * d:j * d + T].abs())
        off = pos.cpu() != (u > 0)
        differ += int(off.sum())
        far += int((off & (u.abs() > 32 * 2.0**-24 * S)).sum())
    return differ, far


def reference(layers, x, wts, dilations, pool, slope, positive=None):
    """(pooled (B, C_last, T // pool), flat gradient of sum(wts * pooled) in the order weight 0, bias 0, weight 1, ...).
    `positive`: per layer a bool (B, C, T) that replaces u > 0 in the derivative of the activation (see "The kink")."""
    pooled, inputs, pre = forward(layers, x, dilations, pool, slope)
    if positive is None:
        positive = [u > 0 for u in pre]
    B, _, T = pre[-1].shape
    Tp = T // pool
    g = torch.zeros_like(pre[-1])
    g[..., :Tp * pool] = (wts.detach().double().cpu() / pool).repeat_interleave(pool, dim=-1)
    grads = []
    for (w, _), d, yp, u, pos in reversed(list(zip(layers, dilations, inputs, pre, positive))):
        k = w.shape[-1]
        gu = g * torch.where(pos.cpu(), torch.ones_like(u), torch.full_like(u, slope))
        dw = torch.stack([torch.einsum("bot,bct->oc", gu, yp[..., j * d:j * d + T]) for j in range(k)], dim=-1)
        grads.append((dw, gu.sum(dim=(0, 2))))
        gp = torch.zeros_like(yp)
        for j in range(k):
            gp[..., j * d:j * d + T] += torch.einsum("bot,oc->bct", gu, w[:, :, j])
        g = gp[..., d * (k - 1):]
    flat = torch.cat([t.reshape(-1) for dw, db in reversed(grads) for t in (dw, db)])
    return pooled, flat


def golden_net(cls, case):
    """the module of a recorded case (tools/make_golden_causal_cnn_embedding.py) with the recorded weights"""
    from torch import nn

    kw = dict(case["kwargs"])
    if case["activation"] is not None:
        kw["activation"] = getattr(nn, case["activation"][0])(**case["activation"][1])
    if case["aggregator"] is not None:
        _, channels, steps, out = case["aggregator"]
        kw["aggregator"] = nn.Sequential(nn.Conv1d(channels, 6, kernel_size=3, padding=1), nn.Tanh(), nn.Flatten(),
                                         nn.Linear(6 * steps, out))
    net = cls(**kw)
    net.load_state_dict(case["state_dict"], strict=True)
    return net
