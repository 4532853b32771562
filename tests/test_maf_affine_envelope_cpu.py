"""The host plan of the affine MAF kernels (csrc/maf_affine.hip: `aff_build_plan`, `aff_plan_for_rows`) through the
host-only `sbi_amd_maf_affine_plan_waves`, against the Python restatement in tests/maf_affine_envelope.py.  No device.

The workgroup widths tests/test_maf_affine_envelope_gpu.py claims (config = D, C, H, NB, T):

  paired kernels (log_prob, sample, training pass): widths follow the row count alone, every config of the envelope
  fits at 8 waves (the corner D16 C32 H64 NB4 takes 138 272 bytes of the 163 840)
      D5 C3 H32 NB1     8161 rows -> 2     16321 -> 4     32641 -> 8
      D10 C10 H50 NB2   32641 -> 8    (sbi's defaults, 13 hidden K-steps)
      D16 C32 H64 NB4   32641 -> 8
      D5 C3 H32 NB0     32641 -> 8
  trials kernel (its scratch also holds 8 flow states per wave), thetas -> waves
      D3 C4 H24 NB2 T3  8161 -> 2     16321 -> 4     32641 -> 8
      D16 C32 H64 NB4   32641 -> 4    (LDS-forced, as the next three)
      D14 C10 H64 NB4   32641 -> 5
      D8 C32 H64 NB4    32641 -> 6
      D4 C32 H64 NB4    32641 -> 7
  1, 2 and 3 waves at 32641 thetas and E_LDS are unreachable inside the envelope.
"""
import itertools

import pytest

from sbi_amd import _lib
from tests import maf_affine_envelope as env

GRID_D = (1, 2, 4, 5, 8, 10, 13, 14, 15, 16)
GRID_C = (1, 3, 10, 15, 16, 17, 32)
GRID_H = (3, 17, 32, 48, 49, 52, 53, 64)
GRID_NB = (0, 1, 2, 4)
GRID_N = (1, 8160, 8161, 16320, 16321, 32640, 32641)


def query(cfg, n, trials=False, epsilon=1e-3):
    D, C, H, NB, T = cfg
    return _lib.load().sbi_amd_maf_affine_plan_waves(_lib.MAFAffineConfigC(D, C, H, T, NB, epsilon), n, int(trials))


def test_restatement_and_query_agree_on_the_grid_and_the_reachable_widths_are_as_stated():
    by_rows = {1: 1, 8160: 1, 8161: 2, 16320: 2, 16321: 4, 32640: 4, 32641: 8}
    reached = {False: set(), True: set()}
    for D, C, H, NB in itertools.product(GRID_D, GRID_C, GRID_H, GRID_NB):
        cfg = (D, C, H, NB, 2)
        for n, trials in itertools.product(GRID_N, (False, True)):
            got = query(cfg, n, trials)
            assert got == env.waves(cfg, n, trials), (cfg, n, trials, got)
            if not trials:
                assert got == by_rows[n], (cfg, n, got)      # the LDS limit never narrows a paired launch
            else:
                assert 1 <= got <= by_rows[n], (cfg, n, got)
            if n == 32641:
                reached[trials].add(got)
    assert reached[False] == {8}
    assert reached[True] == {4, 5, 6, 7, 8}
    # the largest footprint: the corner, in both kernels' scratch layouts
    assert env.lds_bytes(env.CORNER, 8) == 138272 <= env.LDS_LIMIT_BYTES
    assert env.lds_bytes(env.CORNER, 4, trials=True) <= env.LDS_LIMIT_BYTES < env.lds_bytes(env.CORNER, 5, trials=True)
    worst = max(env.lds_bytes((D, C, H, NB, 2), 8) for D, C, H, NB in
                itertools.product(range(1, 17), (1, 16, 17, 32), range(1, 65), range(5)))
    assert worst == env.lds_bytes(env.CORNER, 8)


def test_widths_the_gpu_tests_claim():
    for cfg, n, nw in env.WIDE:
        assert query(cfg, n) == nw == env.waves(cfg, n), (cfg, n)
        assert query(cfg, env.ONE_WAVE_ROWS) == 1
    for cfg, n, nw in env.TRIALS_WIDE + env.TRIALS_FORCED:
        assert query(cfg, n, trials=True) == nw == env.waves(cfg, n, trials=True), (cfg, n)
        assert query(cfg, n) == 8 or n < 32641          # the paired reference of the same thetas is not narrowed
        assert query(cfg, env.ONE_WAVE_ROWS, trials=True) == 1
    assert sorted(nw for _, _, nw in env.TRIALS_FORCED) == [4, 5, 6, 7]
    # the other configs the issue names
    named = {(14, 32, 64, 4, 2): 4, (16, 32, 50, 4, 2): 5, (16, 32, 64, 2, 2): 6, (16, 32, 64, 1, 2): 7}
    for cfg, nw in named.items():
        assert query(cfg, 32641, trials=True) == nw, cfg
    # the shape edges (one dimension at a time from the small config) and the row edges run at one wave
    for D in (1, 4, 5, 13, 15, 16):
        assert query((D, 3, 32, 1, 2), 333) == 1
    for n in (1, 15, 16, 17, 127, 128, 129, 511, 512, 513, 3000, 10**6):
        assert query(env.SMALL, n) == (1 if n <= 8160 else 8)


def test_refusals_keep_their_codes_and_come_from_the_query_too():
    D, C, H, NB, T = env.SMALL
    for trials in (False, True):
        for cfg in ((17, C, H, NB, T), (D, 33, H, NB, T), (D, C, 65, NB, T), (D, C, H, NB, 17), (D, C, H, 5, T)):
            assert query(cfg, 333, trials) == _lib.E_UNSUPPORTED == env.waves(cfg, 333, trials), cfg
        for cfg in ((0, C, H, NB, T), (D, 0, H, NB, T), (D, C, 0, NB, T), (D, C, H, NB, 0), (D, C, H, -1, T)):
            assert query(cfg, 333, trials) == _lib.E_BADARG == env.waves(cfg, 333, trials), cfg
        for eps in (-1e-3, float("nan")):
            assert query(env.SMALL, 333, trials, epsilon=eps) == _lib.E_BADARG == env.waves(env.SMALL, 333, trials, eps)
        assert query(env.SMALL, 333, trials, epsilon=0.0) == 1
        for n in (0, -5):
            assert query(env.SMALL, n, trials) == _lib.E_BADARG == env.waves(env.SMALL, n, trials)
        assert _lib.load().sbi_amd_maf_affine_plan_waves(None, 100, int(trials)) == _lib.E_BADARG


def test_python_surface_answers_and_raises():
    from sbi_amd.neural_nets.estimators.maf_affine_flow import MAFAffineHyper, MAFAffineNet
    import torch

    def net(cfg):
        D, C, H, NB, T = cfg
        hyper = MAFAffineHyper(D=D, C=C, hidden_features=H, num_transforms=T, num_blocks=NB)
        return MAFAffineNet(hyper, torch.zeros(2 * D + 2 * C), True, True)

    small = net(env.SMALL)
    assert [small.plan_waves(n) for n in (1, 8160, 8161, 16321, 32641)] == [1, 1, 2, 4, 8]
    corner = net(env.CORNER)
    assert corner.plan_waves(32641) == 8 and corner.plan_waves(32641, trials=True) == 4
    with pytest.raises(RuntimeError):
        net((5, 3, 65, 1, 2)).plan_waves(333)
