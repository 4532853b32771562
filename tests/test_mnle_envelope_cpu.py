"""The references of the MNLE envelope tests (tests/mnle_envelope.py) on their own, without a GPU: the rows that
tests/test_mnle_envelope_gpu.py leaves out of a comparison are chosen from the two restatements alone, and their number
is capped HERE, so the GPU tests cannot hide a failure behind their exclusions; and the flat parameter layout of the
library against the Python side at every configuration, the distinct-width ones included."""
import pytest
import torch

from tests.mnle_envelope import (CONFIGS, LARGE_CONFIGS, LARGE_ROWS, NEW_CONFIGS, POOL_ROWS, TRAINABLE_NEW, hyper_of,
                                 row_gradients, sample_reference, smooth_rows)

TRAIN_CASES = [(name, False) for name in TRAINABLE_NEW] + [(name, True) for name in LARGE_CONFIGS]
SAMPLE_CASES = ([(name, log_x, False) for name in NEW_CONFIGS for log_x in (False, True)]
                + [(name, True, True) for name in LARGE_CONFIGS])


@pytest.mark.parametrize("name, large", TRAIN_CASES, ids=[f"{n}-{'large' if l else 'pool'}" for n, l in TRAIN_CASES])
def test_training_exclusions_stay_below_one_percent_of_the_pool(name, large):
    rows, left_out = smooth_rows(name, large)
    n = LARGE_ROWS if large else POOL_ROWS
    print(f"{name}: {left_out} of {n} rows left out for a ReLU branch that differs between fp32 and fp64")
    assert rows.numel() + left_out == n
    assert left_out <= n // 100
    _, g64 = row_gradients(name, large)
    assert (g64[rows].abs().max(1).values > 0).all()          # no kept row has a zero reference gradient


def test_floor_has_no_reference_gradient():
    """Why `floor` is a forward-only configuration: d loss / d theta of both restatements is identically zero."""
    g32, g64 = row_gradients("floor")
    assert g64.shape == (POOL_ROWS, 1) and (g64 == 0).all() and (g32 == 0).all()


@pytest.mark.parametrize("name, log_x, large", SAMPLE_CASES,
                         ids=[f"{n}-{'log' if lx else 'linear'}-{'large' if l else 'pool'}" for n, lx, l in SAMPLE_CASES])
def test_sampling_exclusions_stay_below_one_percent_of_the_draws(name, log_x, large):
    keep = sample_reference(name, log_x, large)[-1]
    n = LARGE_ROWS if large else POOL_ROWS
    left_out = int((~keep).sum())
    print(f"{name}: {left_out} of {n} draws within 1e-6 of a cumulative boundary")
    assert keep.shape == (n,) and left_out <= n // 100


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hyper_layout_matches_the_library(name):
    """tests/test_mnle_host_cpu.py::test_hyper_layout_matches_the_library at every configuration (host-only entry
    points: no GPU needed)."""
    from sbi_amd import _lib

    lib = _lib.load()
    h = hyper_of(name)
    cfg = h.c_config()
    assert h.in_envelope()
    assert lib.sbi_amd_mnle_param_count(cfg) == h.param_count()
    off = 0
    for i, (_, o, n_in) in enumerate(h.linears()):
        assert lib.sbi_amd_mnle_param_offset(cfg, i, 0) == off, i
        assert lib.sbi_amd_mnle_param_offset(cfg, i, 1) == off + o * n_in, i
        off += o * n_in + o
    assert off == h.param_count()
    assert lib.sbi_amd_mnle_param_offset(cfg, len(h.linears()), 0) == _lib.E_BADARG
