"""fp64 restatement of the two embedding-net forward formulas (sbi/neural_nets/embedding_nets), with THIS project's
count definition: the count of batch element b is the number of its trials that are not entirely NaN.  Gradients come
by autograd in fp64.  Weights are a list [W0, b0, W1, b1, ...] in state_dict order."""
import torch


def fc_forward(params, x):
    h = x
    for w, b in zip(params[0::2], params[1::2]):
        h = torch.clamp(h @ w.T + b, min=0.0)
    return h


def perminv_forward(trial_params, head_params, x, mean):
    """x (B, T, D) with NaN padding -> (B, E)."""
    nan = torch.isnan(x)
    valid = ~nan.all(dim=-1)                                     # (B, T)
    count = valid.sum(dim=1, keepdim=True).to(x.dtype)           # (B, 1)
    clean = torch.where(nan, torch.zeros_like(x), x)
    emb = fc_forward(trial_params, clean)                        # (B, T, E_t)
    emb = torch.where(valid.unsqueeze(-1), emb, torch.zeros_like(emb))
    pooled = emb.sum(dim=1)
    if mean:
        pooled = pooled / count
    return fc_forward(head_params, torch.cat([pooled, count], dim=1))


def to64(params):
    return [p.detach().double().cpu().clone().requires_grad_(True) for p in params]


def fc_reference(params, x, wts, want_dx=False):
    """(out, [grad of every parameter], dx | None) of sum(out * wts) in fp64."""
    p64 = to64(params)
    x64 = x.detach().double().cpu().clone().requires_grad_(want_dx)
    out = fc_forward(p64, x64)
    grads = torch.autograd.grad((out * wts.double().cpu()).sum(), p64 + ([x64] if want_dx else []))
    return out.detach(), list(grads[:len(p64)]), (grads[-1] if want_dx else None)


def perminv_reference(trial_params, head_params, x, wts, mean):
    t64, h64 = to64(trial_params), to64(head_params)
    out = perminv_forward(t64, h64, x.detach().double().cpu(), mean)
    grads = torch.autograd.grad((out * wts.double().cpu()).sum(), t64 + h64)
    return out.detach(), list(grads)


def lds_bytes(in_dim, hidden, out_dim, L):
    """the documented image: weight rows padded to 16 with stride + 4, biases, L + 1 row tiles of 32 rows (16 rows
    when 32 would pass 160 KiB), 352 misc"""
    up = lambda n: (n + 15) // 16 * 16     # noqa: E731
    d = [up(in_dim)] + [up(hidden)] * (L - 1) + [up(out_dim)]
    image = sum(d[i + 1] * (d[i] + 4) + d[i + 1] for i in range(L)) + 352
    with_32 = 4 * (image + 32 * sum(w + 4 for w in d))
    return with_32 if with_32 <= 160 * 1024 else 4 * (image + 16 * sum(w + 4 for w in d))
