"""fp64 oracle of the Gaussian variational family and its four divergence optimisers, in plain torch.

It restates `LearnableGaussian` (loc, tril(scale_tril) or exp(log_scale)) and the per-dimension link of
include/sbi_amd_vi.h, is fed a GIVEN eps, writes the four surrogate losses the way
sbi/samplers/vi/vi_divergence_optimizers.py writes them, and lets autograd produce the reference gradient;
`clip_grad_norm_` + `torch.optim.Adam` + `ExponentialLR` produce the reference update.  The potential enters as its
values p_i and its theta-gradients r_i at the drawn points: p_i(theta) = p_i + r_i . (theta - theta_i) has exactly
those, which is all a first-order method sees.  `philox_normal` restates the kernels' eps stream on the host.
"""
import math

import numpy as np
import torch

F64 = torch.float64
TAG = 0x56494731


# ---- the eps stream ---------------------------------------------------------------------------------------------
def _philox4x32_10(c, k):
    """c: (N, 4) uint64 holding 32-bit words, k: (2,) python ints."""
    c = [c[:, i].copy() for i in range(4)]
    k0, k1 = int(k[0]), int(k[1])
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n1 = p1 & M
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        n3 = p0 & M
        c = [n0 & M, n1, n2 & M, n3]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1)


def philox_normal(seed, step, rows, D):
    """eps (len(rows), D) in fp64: Box-Muller on philox4x32_10(counter = (row lo, row hi, step, TAG + d // 4),
    key = (seed lo, seed hi)) as include/sbi_amd_vi.h states it."""
    rows = np.asarray(rows, dtype=np.uint64)
    out = np.zeros((len(rows), 4 * ((D + 3) // 4)))
    for j in range((D + 3) // 4):
        ctr = np.stack([rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), np.full_like(rows, step),
                        np.full_like(rows, TAG + j)], axis=1)
        o = _philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.float64)
        for h in range(2):
            u1 = (np.floor(o[:, 2 * h] / 256) + 1) / 16777216.0
            u2 = np.floor(o[:, 2 * h + 1] / 256) / 16777216.0
            rad = np.sqrt(-2 * np.log(u1))
            ang = np.float64(np.float32(6.283185307179586)) * u2
            out[:, 4 * j + 2 * h] = rad * np.cos(ang)
            out[:, 4 * j + 2 * h + 1] = rad * np.sin(ang)
    return torch.from_numpy(out[:, :D].copy())


# ---- the family -------------------------------------------------------------------------------------------------
def split_phi(phi, D, full):
    loc = phi[:D]
    if full:
        L = phi[D:].reshape(D, D).tril()
    else:
        L = torch.diag(phi[D:].exp())
    return loc, L


def link_forward(z, link):
    """theta and sum_d log|T'(z_d)| for the (4, D) table [kind | a | b | c] (None: identity), torch's formulas."""
    if link is None:
        return z, torch.zeros(z.shape[:-1], dtype=z.dtype)
    kind, a, b = link[0], link[1].to(F64), link[2].to(F64)
    tiny, eps = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).eps
    sig = torch.clamp(torch.sigmoid(z), min=tiny, max=1.0 - eps)
    sp = torch.nn.functional.softplus
    th = torch.where(kind == 0, a + b * z, torch.where(kind == 1, a + b * sig, torch.where(kind == 2, a + z.exp(),
                                                                                         a - z.exp())))
    ld = torch.where(kind == 0, b.abs().log().expand_as(z),
                     torch.where(kind == 1, -sp(-z) - sp(z) + b.abs().log(), z))
    return th, ld.sum(-1)


def base_log_prob(z, loc, L):
    D = z.shape[-1]
    e = torch.linalg.solve_triangular(L, (z - loc).T, upper=False).T
    return -0.5 * (e * e).sum(-1) - 0.5 * D * math.log(2 * math.pi) - torch.diagonal(L).log().sum()


def forward(phi, link, eps, D, full):
    """(z, theta, log q(theta)) with everything attached to `phi`."""
    loc, L = split_phi(phi, D, full)
    z = loc + eps @ L.T
    theta, ld = link_forward(z, link)
    return z, theta, base_log_prob(z, loc, L) - ld


def losses(method, phi, link, eps, p, r, D, full, K=1, alpha=0.5, unbiased=False, stick_the_landing=False, dreg=False):
    """(surrogate loss, displayed loss) of one optimiser step, as the reference writes them.  `r` None for fKL."""
    n = eps.shape[0]
    loc, L = split_phi(phi, D, full)
    if method == "fKL":
        with torch.no_grad():
            z = loc + eps @ L.T
            _, ld = link_forward(z, link)
        logq = base_log_prob(z, loc, L) - ld                  # theta (= z) detached, the parameters attached
        with torch.no_grad():
            lw = p - logq
            w = (lw - lw.max()).exp()
            w = w / w.sum()
        return -(w * logq).sum(), (w * (p - logq)).sum().detach()
    if dreg:
        stick_the_landing = True
    z = loc + eps @ L.T
    theta, ld = link_forward(z, link)
    if stick_the_landing:
        logq = base_log_prob(z, loc.detach(), L.detach()) - ld    # the surrogate q: detached parameters at theta
    else:
        logq = base_log_prob(z, loc, L) - ld
    pot = p + (r * (theta - theta.detach())).sum(-1)          # value p_i, theta-gradient r_i
    elbo = pot - logq
    if method == "rKL":
        loss = -elbo.mean()
        return loss, loss.detach()
    if method == "IW":
        el = elbo.reshape(n // K, K)
        w = torch.exp(el.detach() - torch.logsumexp(el.detach(), -1, keepdim=True))
        if dreg:
            w = w**2
        surrogate = -(w * el).sum(-1).mean(0)
        loss = -torch.mean(torch.exp(el) + 1e-20, -1).log().mean()
        return surrogate, loss.detach()
    assert method == "alpha"

    def importance(e):
        lw = (1 - alpha) * e
        mean_lw = torch.logsumexp(lw, 0) - math.log(n)
        w = (lw - mean_lw).exp()
        return (w**2 if dreg else w), mean_lw

    if unbiased:
        _, mean_lw = importance(elbo * (1 - alpha))
        return -torch.exp(mean_lw), (-mean_lw / (1 - alpha)).detach()
    w, mean_lw = importance(elbo.detach())
    return -torch.mean(w * elbo), (-mean_lw / (1 - alpha)).detach()


def gradient(method, phi32, link, eps32, p32, r32, D, full, **kw):
    """(grad (P,), displayed loss) in fp64 from fp32 inputs."""
    phi = phi32.detach().cpu().to(F64).requires_grad_(True)
    link = None if link is None else link.detach().cpu()
    r = None if r32 is None else r32.detach().cpu().to(F64)
    surrogate, loss = losses(method, phi, link, eps32.detach().cpu().to(F64), p32.detach().cpu().to(F64), r, D, full,
                             **kw)
    (g,) = torch.autograd.grad(surrogate, phi)
    return g, loss


def update(phi32, grad, clip_value, lr, gamma=1.0, sched_steps=0, betas=(0.9, 0.999)):
    """phi after clip_grad_norm_ + one Adam step from zero moments, the learning rate after `sched_steps` steps of
    ExponentialLR(gamma), in fp64."""
    param = torch.nn.Parameter(phi32.detach().cpu().to(F64).clone())
    opt = torch.optim.Adam([param], lr=lr, betas=betas)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
    for _ in range(sched_steps):
        opt.step()                      # (no gradient yet: a no-op that keeps the scheduler's call order legal)
        sched.step()
    param.grad = grad.clone()
    if clip_value > 0:
        torch.nn.utils.clip_grad_norm_([param], clip_value)
    opt.step()
    return param.detach()
