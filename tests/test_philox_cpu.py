"""The host Philox4x32-10 of tests/mcmc_restatement.py against the published Random123 known-answer vectors
(Random123's kat_vectors, the three `philox4x32 10` lines), and the layout of the uniforms built from it.  The GPU
tests hold the in-kernel generator (csrc/philox.h) to this one, so these vectors pin both."""

import numpy as np
import pytest
import torch

from tests.mcmc_restatement import philox4x32_10, tick_uniforms, torch_tick, u01, restatement_state

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox4x32_10_known_answers(counter, key, want):
    got = tuple(int(w) for w in philox4x32_10(counter, key))
    assert got == want, [hex(g) for g in got]


def test_philox_is_vectorised_over_counters():
    ctr = [np.array([c[q] for c, _, _ in KAT], dtype=np.uint64) for q in range(4)]
    key = [np.array([k[q] for _, k, _ in KAT], dtype=np.uint64) for q in range(2)]
    got = np.stack(philox4x32_10(ctr, key), axis=1)
    assert got.tolist() == [list(w) for _, _, w in KAT]


def test_u01_keeps_the_top_24_bits():
    r = np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
    got = u01(r)
    assert got.dtype == np.float32
    assert got.tolist() == [0.0, 0.0, 2.0**-24, 0.5, 1.0 - 2.0**-24]


def test_tick_uniforms_layout():
    """Block 0 -> u[0..3]; lane d & 3 of block 1 + (d >> 2) -> column 4 + d; counter words (tick lo, tick hi, chain,
    block), key words (seed lo, seed hi)."""
    seed, tick, C, D = 0x9E3779B97F4A7C15, 2**32 + 5, 7, 9
    u = tick_uniforms(seed, tick, C, D)
    assert u.shape == (C, 4 + D) and u.dtype == torch.float32
    assert bool(((u >= 0) & (u < 1)).all())
    for c in (0, 3, 6):
        key = (0x7F4A7C15, 0x9E3779B9)
        b0 = philox4x32_10((5, 1, c, 0), key)
        assert u[c, :4].tolist() == [float(u01(w)) for w in b0]
        for d in range(D):
            w = philox4x32_10((5, 1, c, 1 + (d >> 2)), key)[d & 3]
            assert u[c, 4 + d].item() == float(u01(w)), (c, d)
    # another chain, tick or seed is another stream
    assert not torch.equal(u[0], u[1])
    assert not torch.equal(u, tick_uniforms(seed, tick + 1, C, D))
    assert not torch.equal(u, tick_uniforms(seed ^ (1 << 40), tick, C, D))
    assert not torch.equal(u, tick_uniforms(seed, tick ^ (1 << 40), C, D))


def _scalar_order(u_row, D):
    """The Fisher-Yates of csrc/mcmc_tick.h for one chain, float32 product."""
    o = list(range(D))
    for d in range(D - 1, 0, -1):
        k = min(int(np.float32(u_row[4 + d]) * np.float32(d + 1)), d)
        o[d], o[k] = o[k], o[d]
    return o


@pytest.mark.parametrize("D", [1, 2, 5, 9])
def test_restatement_shuffle_equals_the_scalar_fisher_yates(D):
    """A chain that accepts in its last dimension gets a fresh order: the tensorised swap loop against the scalar one,
    with uniforms at the edges of the index computation (0, just below 1, k / (d + 1) and its neighbours)."""
    C = 64
    g = torch.Generator().manual_seed(D)
    u = torch.rand(C, 4 + D, generator=g)
    edge = torch.tensor([0.0, 1.0 - 2.0**-24, 0.5, 1.0 / 3.0, 2.0 / 3.0, 0.25, 0.75, 0.2, 0.4, 0.6, 0.8])
    u[: edge.numel(), 4:] = edge[:, None]
    u[edge.numel() : 2 * edge.numel(), 4:] = torch.nextafter(edge, torch.tensor(0.0)).clamp(min=0.0)[:, None]
    st = restatement_state(torch.zeros(C, D), torch.arange(D).repeat(C, 1), 1.0, 2)
    st.update(state=torch.full((C,), 3), i=torch.full((C,), D - 1))           # SAMPLE_SLICE in the last dimension
    torch_tick(st, torch.zeros(C), u, 2, 0, 3.0e38)                            # log p = logu = 0: accepted
    assert bool((st["t"] == 1).all()) and bool((st["state"] == 0).all())
    assert st["order"].tolist() == [_scalar_order(u[c].numpy(), D) for c in range(C)]
