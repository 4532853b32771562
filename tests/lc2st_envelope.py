"""The case table of the L-C2ST envelope tests (tests/test_lc2st_envelope_cpu.py and test_lc2st_envelope_gpu.py): the
shapes, members, batch sizes and evaluation sizes at which csrc/lc2st_kernel.h changes tile, chunk or row-block
structure, the plan arithmetic of `lc_build_plan` restated from its rules, and the shared inputs and fp64 / fp32
references of every case (tests/lc2st_oracle.py), computed once and never modified.  Importable without a GPU; no test
functions here.

A shape is (D, Dx, H): theta features, x features, hidden width.  F = D + Dx.  The kernel pads F and H to 16
(Fp, Hp; FB, HB tiles), walks a batch in chunks of 32 rows, evaluates in row blocks of 512, and folds x_o into the first
bias so that the evaluation's first contraction is K1 = round_up(D, 16) wide.
"""
import functools

import numpy as np
import torch

from sbi_amd.diagnostics import lc2st as L
from tests import lc2st_oracle as O
from tests.test_lc2st_gpu import make_members

TILE, CHUNK, EVAL_ROWS = 16, 32, 512
SEED = 20240917

SHAPES = [
    ((1, 1, 1), "smallest of everything"),
    ((1, 1, 3), "small H, F = 2"),
    ((15, 1, 16), "F = 16 and H = 16 exactly one tile, D = 15"),
    ((16, 1, 17), "K1 = 16 exact; F = 17, H = 17: one live row / column in the second tile"),
    ((17, 15, 15), "F = 32, D = 17 gives K1 = 32"),
    ((1, 32, 33), "FB = 3, HB = 3, one live row / column in the third tile, D = 1"),
    ((32, 16, 48), "FB = 3, HB = 3 exact"),
    ((33, 16, 49), "FB = 4, HB = 4 by one"),
    ((63, 1, 112), "F = 64, D = 63, HB = 7 exact"),
    ((1, 63, 113), "F = 64, D = 1, HB = 8 by one"),
    ((48, 16, 128), "both envelope maxima, the LDS corner of the kernel's header comment"),
]
SHAPE_LIST = [s for s, _ in SHAPES]
MEMBER_SIZES = [(1, 1), (2, 32), (33, 33), (64, 64), (97, 31)]      # (n_train, n_valid)
DATA_ROWS = 150
GRAD_BATCH_SIZES = (1, 31, 32, 33, 64, 97, 200)
GRAD_EPOCHS = (0, 3)
TRAJECTORY_BATCH_SIZES = (32, 33)
EVAL_SIZES = (1, 31, 32, 33, 511, 512, 513, 1025)
EVAL_LAYOUTS = ((1, False), (1, True), (3, False), (3, True))        # (group_size, theta per group) over 3 members
FIRST_STEP_MEMBERS = (0, 2)            # (1, 1) and (33, 33): one epoch is one step at B = 64
FIRST_STEP_BATCH_SIZE = 64
FIRST_STEP_LEFT_OUT = set()            # (shape, member) whose gradient leaves <= 0.3 of the entries above 1e-6: none

# bounds of tests/test_lc2st_gpu.py::test_batch_grad_matches_fp64_autograd
LOSS_ABS = LOSS_REL = 1e-5
GRAD_REL, BLOCK_REL, BLOCK_FLOOR = 2e-4, 3e-4, 1e-3


def shape_id(s):
    return "D%d-Dx%d-H%d" % s


# ------------------------------------------------------------------------------ the plan of lc_build_plan, restated
def _round_up(v, m):
    return (v + m - 1) // m * m


def plan(shape):
    D, Dx, H = shape
    F = D + Dx
    Fp, Hp = _round_up(F, TILE), _round_up(H, TILE)
    return dict(D=D, Dx=Dx, H=H, F=F, Fp=Fp, Hp=Hp, FB=Fp // TILE, HB=Hp // TILE, K1=_round_up(D, TILE))


def batches(nt, B):
    """[(first position, rows)] of the batches of one epoch over nt training rows."""
    return [(p, min(B, nt - p)) for p in range(0, nt, B)]


def chunks(rows):
    """(chunks of one batch, rows of its last chunk)."""
    n = -(-rows // CHUNK)
    return n, rows - (n - 1) * CHUNK


def grad_batches(B):
    """Batch indices of the gradient test at batch size B: batch 0, every member's last batch, and one index past the
    end of every member (NaN loss, zero gradient)."""
    last = sorted({len(batches(nt, B)) - 1 for nt, _ in MEMBER_SIZES})
    return sorted({0, *last}) + [last[-1] + 1]


# ------------------------------------------------------------------------------------------------ inputs, built once
@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(data, members, params0) of a shape: R = 150 shared rows, the five members, initial weights of seeds 100 + m."""
    D, Dx, H = shape
    rng = np.random.default_rng(sum(shape) + 1000)
    data = torch.from_numpy(rng.standard_normal((DATA_ROWS, D + Dx)).astype(np.float32))
    members = make_members(DATA_ROWS, MEMBER_SIZES, D + Dx, rng, data)
    base = L.LC2STHyper(D=D, Dx=Dx, H=H)
    params0 = torch.stack([L.init_params(base, s) for s in members.init_seed])
    return data, members, params0


def hyper(shape, **kw):
    D, Dx, H = shape
    return L.LC2STHyper(D=D, Dx=Dx, H=H, **kw)


def block_metric(h, got, ref):
    """[(parameter name, max |got - ref| / max(|ref block|, 1e-3 |ref|))]: the per-block figure of the gradient test."""
    scale = ref.abs().max().item()
    return [(name, (a - b).abs().max().item() / max(b.abs().max().item(), BLOCK_FLOOR * scale))
            for (name, _), a, b in zip(h.param_shapes(), O.split_params(h, got), O.split_params(h, ref))]


@functools.lru_cache(maxsize=None)
def grad_references(shape):
    """{(B, which, epoch, batch, m): (rows, labels, loss64, grad64)} for every case of the gradient test: each member's
    batch 0 and last batch at epochs 0 and 3 (which = 0), and the validation rows as one batch (which = 1, at
    B = 200)."""
    data, members, params0 = inputs(shape)
    out = {}
    for B in GRAD_BATCH_SIZES:
        h = hyper(shape, batch_size=B)
        for epoch in GRAD_EPOCHS:
            for m, (nt, _) in enumerate(MEMBER_SIZES):
                order = O.epoch_order(nt, SEED, epoch, int(members.member_id[m]))
                for batch in sorted({0, len(batches(nt, B)) - 1}):     # the member's first and last batch
                    rows, lab = O.member_batch(members, m, h, SEED, epoch, batch, order)
                    out[(B, 0, epoch, batch, m)] = (rows, lab) + O.loss_and_grad(h, params0[m], data, rows, lab,
                                                                                 torch.float64)
    h = hyper(shape)
    for m in range(len(MEMBER_SIZES)):
        rows, lab = O.member_valid(members, m)
        out[(h.batch_size, 1, 0, 0, m)] = (rows, lab) + O.loss_and_grad(h, params0[m], data, rows, lab, torch.float64)
    return out


@functools.lru_cache(maxsize=None)
def eval_inputs(shape):
    """(params (3, P) = 2 x the initial weights of members 0..2, theta (3, 1025, D), x_o): every evaluation size takes
    the leading rows of the same theta, so the runs can be compared row by row."""
    _, _, params0 = inputs(shape)
    g = torch.Generator().manual_seed(3)
    D, Dx, _ = shape
    return params0[:3] * 2.0, torch.randn(3, max(EVAL_SIZES), D, generator=g), torch.randn(Dx, generator=g)


def eval_theta(shape, n, group_size, per_group):
    _, theta, _ = eval_inputs(shape)
    groups = 3 // group_size
    return theta[:groups, :n].contiguous() if per_group else theta[0, :n].contiguous()


@functools.lru_cache(maxsize=None)
def eval_references(shape):
    """{(n, group_size, per_group): (proba64, score64, proba32, score32)}."""
    params, _, x_o = eval_inputs(shape)
    h = hyper(shape)
    out = {}
    for n in EVAL_SIZES:
        for group_size, per_group in EVAL_LAYOUTS:
            th = eval_theta(shape, n, group_size, per_group)
            out[(n, group_size, per_group)] = (O.eval_proba(h, params, th, x_o, group_size, torch.float64) +
                                               O.eval_proba(h, params, th, x_o, group_size, torch.float32))
    return out


@functools.lru_cache(maxsize=None)
def trajectory_references(shape, B):
    """[(history64, worst |o32 - f64| as-is, worst over as-is and four re-orderings)] per member, three epochs."""
    data, members, params0 = inputs(shape)
    h = hyper(shape, batch_size=B, max_epochs=3)
    out = []
    for m in range(len(MEMBER_SIZES)):
        r64 = O.train_member(h, data, members, m, params0[m], SEED, 3, torch.float64)["history"]
        devs = [np.abs(O.train_member(h, data, members, m, params0[m], SEED, 3, torch.float32, reorder=r)["history"]
                       - r64).max() for r in (None, 1, 2, 3, 4)]
        out.append((r64, devs[0], max(devs)))
    return out


# ------------------------------------------------------------------------- the rows a kernel could drop unnoticed
def edge_entries(shape):
    """{name: (block index, index expression)}: the last live row and column of dW1 and dW2, the last entry of db1,
    db2 and dw3 -- what a wrong tile bound or guard would lose first."""
    return {"dW1 last row": (0, (-1, slice(None))), "dW1 last column": (0, (slice(None), -1)),
            "dW2 last row": (2, (-1, slice(None))), "dW2 last column": (2, (slice(None), -1)),
            "db1 last": (1, (-1,)), "db2 last": (3, (-1,)), "dw3 last": (4, (0, -1))}


@functools.lru_cache(maxsize=None)
def edge_observability(shape):
    """{name: (largest max|edge| / max|block| over the gradient cases, the case's key)} on the fp64 gradient of the
    loss alone (weight_decay = 0: the decay term would make every entry visible whatever the kernel sums)."""
    data, _, params0 = inputs(shape)
    h = hyper(shape, weight_decay=0.0)
    best = {name: (0.0, None) for name in edge_entries(shape)}
    for key, (rows, lab, _, _) in grad_references(shape).items():
        _, g = O.loss_and_grad(h, params0[key[4]], data, rows, lab, torch.float64)
        blocks = O.split_params(h, g)
        for name, (b, idx) in edge_entries(shape).items():
            top = blocks[b].abs().max().item()
            share = blocks[b][idx].abs().max().item() / top if top > 0 else 0.0
            if share > best[name][0]:
                best[name] = (share, key)
    return best
