"""Eager-torch restatement of the L-C2ST trainer and evaluation (TEST INFRASTRUCTURE: only tests and tools import this).

Same row lists, same initial weights, same epoch orders and the rules of include/sbi_amd_lc2st.h, in fp32 or fp64:
the orders come from the Python `prp` of tests/shuffle_restatement.py keyed by the Philox restatement of
tests/mcmc_restatement.py; the optimiser is `torch.optim.Adam(weight_decay=...)`.  The early-stopping rule restates
skorch's `EarlyStopping` from its documentation (skorch is not installable here), as the header says.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.mcmc_restatement import philox4x32_10
from tests.shuffle_restatement import prp

STREAM_TAG = 0x4C433253


def epoch_key(seed: int, epoch: int, member_id: int) -> int:
    o = philox4x32_10((epoch, 0, member_id, STREAM_TAG), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return int(o[0]) | (int(o[1]) << 32)


def epoch_order(n_train: int, seed: int, epoch: int, member_id: int) -> np.ndarray:
    key = epoch_key(seed, epoch, member_id)
    return np.array([prp(i, n_train, key) for i in range(n_train)], dtype=np.int64)


def split_params(hyper, flat):
    out, o = [], 0
    for _, shape in hyper.param_shapes():
        n = int(np.prod(shape))
        out.append(flat[o:o + n].reshape(shape))
        o += n
    return out


def logits(hyper, flat, X):
    w1, b1, w2, b2, w3, b3 = split_params(hyper, flat)
    h = torch.relu(X @ w1.T + b1)
    h = torch.relu(h @ w2.T + b2)
    return (h @ w3.T + b3)[:, 0]


def member_batch(members, m, hyper, seed, epoch, batch, order=None):
    """(row indices into data, labels) of batch `batch` of epoch `epoch` of member slot m."""
    nt = int(members.n_train[m])
    if order is None:
        order = epoch_order(nt, seed, epoch, int(members.member_id[m]))
    pos = order[batch * hyper.batch_size: min((batch + 1) * hyper.batch_size, nt)]
    return members.rows[m, pos].astype(np.int64), members.labels[m, pos]


def member_valid(members, m):
    nt, nv = int(members.n_train[m]), int(members.n_valid[m])
    return members.rows[m, nt:nt + nv].astype(np.int64), members.labels[m, nt:nt + nv]


def loss_and_grad(hyper, flat, data, rows, labels, dtype):
    """mean BCE-with-logits over the rows and g = dloss/dp + weight_decay p (autograd)."""
    p = flat.detach().to(dtype).clone().requires_grad_(True)
    X = data[torch.as_tensor(rows)].to(dtype)
    y = torch.as_tensor(labels).to(dtype)
    loss = F.binary_cross_entropy_with_logits(logits(hyper, p, X), y)
    (g,) = torch.autograd.grad(loss, p)
    return loss.detach(), g + hyper.weight_decay * p.detach()


class EarlyStopper:
    """improved iff valid < best (1 - threshold); improved: best = valid, misses = 0; else misses += 1; stop when
    misses == patience or epoch == max_epochs."""

    def __init__(self, patience, max_epochs, threshold=1e-4):
        self.patience, self.max_epochs, self.threshold = patience, max_epochs, threshold
        self.best, self.misses, self.epoch, self.best_epoch, self.stopped = float("inf"), 0, 0, -1, False

    def update(self, valid: float) -> bool:
        """-> True when this epoch improved (the caller then keeps the parameters)."""
        improved = valid < self.best * (1.0 - self.threshold)
        if improved:
            self.best, self.misses, self.best_epoch = valid, 0, self.epoch
        else:
            self.misses += 1
        self.epoch += 1
        self.stopped = self.misses >= self.patience or self.epoch >= self.max_epochs
        return improved


def train_member(hyper, data, members, m, params0, seed, epochs, dtype, reorder=None):
    """Up to `epochs` epochs of member slot m from params0 -> dict(history (epochs, 2), params, best_params, ...).
    reorder: None, or a seed -- every batch's (and the validation set's) rows are then summed in another order, the same
    mathematics in a different floating-point order (what a kernel with its own reduction order is to this oracle)."""
    data = data.to(dtype)
    p = params0.detach().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=hyper.lr, betas=(hyper.beta1, hyper.beta2), eps=hyper.eps,
                           weight_decay=hyper.weight_decay)
    es = EarlyStopper(hyper.patience, hyper.max_epochs, hyper.threshold)
    nt = int(members.n_train[m])
    vrows, vlab = member_valid(members, m)
    rng = None if reorder is None else np.random.default_rng(reorder)
    if rng is not None:
        q = rng.permutation(len(vrows))
        vrows, vlab = vrows[q], vlab[q]
    Xv, yv = data[torch.as_tensor(vrows)], torch.as_tensor(vlab).to(dtype)
    hist = np.full((epochs, 2), np.nan)
    best_params = p.detach().clone()
    for e in range(epochs):
        if es.stopped:
            break
        order = epoch_order(nt, seed, e, int(members.member_id[m]))
        tsum = 0.0
        for b in range(-(-nt // hyper.batch_size)):
            rows, lab = member_batch(members, m, hyper, seed, e, b, order)
            if rng is not None:
                q = rng.permutation(len(rows))
                rows, lab = rows[q], lab[q]
            opt.zero_grad()
            loss = F.binary_cross_entropy_with_logits(logits(hyper, p, data[torch.as_tensor(rows)]),
                                                      torch.as_tensor(lab).to(dtype))
            loss.backward()
            opt.step()
            tsum += float(loss.detach()) * len(rows)
        with torch.no_grad():
            valid = float(F.binary_cross_entropy_with_logits(logits(hyper, p, Xv), yv))
        hist[e] = (tsum / nt, valid)
        if es.update(valid):
            best_params = p.detach().clone()
    return dict(history=hist, params=p.detach(), best_params=best_params, best_epoch=es.best_epoch, epoch=es.epoch,
                stopped=es.stopped)


def eval_proba(hyper, params, theta, x_o, group_size, dtype):
    """-> proba (groups, n), score (groups,): class-0 probability averaged over each group's members, then the score.
    theta (n, D) shared or (groups, n, D)."""
    params, theta, x_o = params.to(dtype), theta.to(dtype), x_o.to(dtype).reshape(1, -1)
    groups = params.shape[0] // group_size
    proba = []
    for g in range(groups):
        th = theta if theta.dim() == 2 else theta[g]
        X = torch.cat([th, x_o.expand(th.shape[0], -1)], dim=1)
        proba.append(torch.stack([1.0 - torch.sigmoid(logits(hyper, params[g * group_size + e], X))
                                  for e in range(group_size)]).mean(0))
    proba = torch.stack(proba)
    return proba, ((proba - 0.5) ** 2).mean(1)
