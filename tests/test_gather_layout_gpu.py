"""The minibatch gather (csrc/shuffle.hip) over the shapes and alignments that decide how a row can be copied: widths
that allow 8-byte accesses, odd ones and one of each, bases that sit 4 bytes past an 8-byte boundary, windows that start
and end inside a wave's 64 rows, with and without a base index, and calls that ask for only one of the three outputs.

However the kernel lays a row over its lanes, none of it may show: the source rows are those of
tests/shuffle_restatement.py index for index, the gathered rows are `theta_all[idx]` / `x_all[idx]` bit for bit, and
every output sits between guard rows that must keep their fill."""

from functools import lru_cache

import pytest
import torch

from sbi_amd.utils.shuffle import ShuffledGather, epoch_key
from tests.shuffle_restatement import prp

pytestmark = pytest.mark.gpu

SEED, EPOCH, EXTRA = 7, 3, 7        # EXTRA: rows of theta_all / x_all beyond the n_perm that a base index selects from
GUARD = -123.0


def _windows(n):
    """(offset, count): from the start (several blocks and a partial last wave where n allows), from the middle, and
    ending at n_perm."""
    out = [(0, min(n, 2891))]
    if n - n // 3 - 1 > 0:
        out.append((n // 3, min(n - n // 3 - 1, 777)))
    out.append((n - min(n, 333), min(n, 333)))
    return out


@lru_cache(maxsize=None)
def _order(n, lo, cnt):
    return torch.tensor([prp(i, n, epoch_key(SEED, EPOCH)) for i in range(lo, lo + cnt)], dtype=torch.int64)


@lru_cache(maxsize=None)
def _base(n):
    return torch.randperm(n + EXTRA, generator=torch.Generator().manual_seed(n))[:n]


def _rows(n_rows, d, seed, misalign):
    """(n_rows, d) random fp32 rows on the device; `misalign`: the first element sits 4 bytes past an 8-byte boundary."""
    flat = torch.randn(n_rows * d + 1, generator=torch.Generator().manual_seed(seed)).cuda()
    t = flat[1:] if misalign else flat[:-1]
    assert t.data_ptr() % 8 == (4 if misalign else 0)
    return t.view(n_rows, d)


def _guarded(cnt, d, dtype=torch.float32, misalign=False):
    """An output of `cnt` rows between two guard rows (plus one leading element when misaligned)."""
    buf = torch.full(((cnt + 2) * d + 1,), GUARD, dtype=dtype).cuda()
    body = buf[1:] if misalign else buf[:-1]
    rows = body.view(cnt + 2, d)
    return buf, rows[1:cnt + 1]


def _guards_intact(buf, out):
    keep = torch.ones_like(buf, dtype=torch.bool)
    start = (out.data_ptr() - buf.data_ptr()) // buf.element_size()
    keep[start:start + out.numel()] = False
    return bool((buf[keep] == GUARD).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("da,db", [(1, 1), (3, 2), (10, 10), (17, 5)])
@pytest.mark.parametrize("n", [1, 2, 65, 1000, 100_000])
def test_gather_matches_restatement_and_plain_indexing(n, da, db, misalign):
    th_all, x_all = _rows(n + EXTRA, da, 1, misalign), _rows(n + EXTRA, db, 2, misalign)
    th_cpu, x_cpu = th_all.cpu(), x_all.cpu()
    for with_base in (False, True):
        base = _base(n) if with_base else None
        # (without a base index the order runs over every row of the tensors: hand over the first n_perm of them)
        sg = (ShuffledGather(th_all, x_all, base.cuda(), seed=SEED) if with_base else
              ShuffledGather(th_all[:n], x_all[:n], None, seed=SEED))
        assert sg.n == n and sg.theta_all.data_ptr() == th_all.data_ptr() and sg.x_all.data_ptr() == x_all.data_ptr()
        for lo, cnt in _windows(n):
            want = _order(n, lo, cnt) if base is None else base[_order(n, lo, cnt)]
            # all three outputs in one launch
            ba, a = _guarded(cnt, da, misalign=misalign)
            bb, b = _guarded(cnt, db, misalign=misalign)
            bi, i = _guarded(cnt, 1, torch.int64)
            sg._call(EPOCH, lo, cnt, a, b, i.view(-1))
            assert torch.equal(i.view(-1).cpu(), want), (lo, cnt, with_base)
            assert torch.equal(_bits(a).cpu(), _bits(th_cpu[want])) and torch.equal(_bits(b).cpu(), _bits(x_cpu[want]))
            assert _guards_intact(ba, a) and _guards_intact(bb, b) and _guards_intact(bi, i)
            # the index alone, theta alone, x alone
            assert torch.equal(sg.indices(EPOCH, lo, cnt).cpu(), want)
            ba, a = _guarded(cnt, da, misalign=not misalign)      # (the output's alignment alone decides, too)
            sg._call(EPOCH, lo, cnt, a, None, None)
            assert torch.equal(_bits(a).cpu(), _bits(th_cpu[want])) and _guards_intact(ba, a)
            bb, b = _guarded(cnt, db, misalign=misalign)
            sg._call(EPOCH, lo, cnt, None, b, None)
            assert torch.equal(_bits(b).cpu(), _bits(x_cpu[want])) and _guards_intact(bb, b)
            # the public entry points
            a, b = sg.batch(EPOCH, lo, cnt)
            assert torch.equal(_bits(a).cpu(), _bits(th_cpu[want])) and torch.equal(_bits(b).cpu(), _bits(x_cpu[want]))
