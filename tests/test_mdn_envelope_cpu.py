"""What tests/test_mdn_envelope_gpu.py relies on, checked without a GPU: the restatement of the host side's plan in
tests/mdn_envelope.py against the library's host-only size queries at every configuration and row edge; every named
row count and configuration on the path it is listed for (1, 2 or 4 waves, 13 or 16 K-steps, its number of
weight-gradient chunks, the capped broadcast grid on a second trip), so that a later change to the plan fails HERE
instead of silently emptying the GPU tests; and the conditions on the references alone (finite fp32 / fp64 references,
non-zero gradients, the left-out cap of the sampling draws, the share of raw diagonal entries above softplus's
threshold, the weights at the ends of the component selection)."""
import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.mdn import MDNHyper
from tests.mdn_envelope import (BCAST_CONFIGS, BCAST_LOG_PROB_ROWS, BCAST_SAMPLE_ROWS, CHUNK_ROWS, CONFIGS,
                                LDS_LIMIT_BYTES, POOL_ROWS, ROWS, SELECT_CONFIGS, SOFTPLUS_CONFIGS, WAVE_CONFIGS,
                                WAVE_ROWS, XROWS_CASES, bcast_grid_and_trips,
                                bcast_lds_bytes, bcast_subset, ksh, large_pool, mdn_pair_cpu, nchunks,
                                paired_lds_bytes, plan, ref_log_prob, ref_pick, sample_draws, softplus_fraction,
                                softplus_pair_cpu, softplus_theta, training_reference, training_weights, waves,
                                workspace_floats)

ALL_CONFIGS = {**CONFIGS, "softplus-mid": SOFTPLUS_CONFIGS["mid"]}
ROW_EDGES = sorted(set(ROWS + WAVE_ROWS + CHUNK_ROWS + [n for n, _ in XROWS_CASES]
                       + [0, 511, 1024, 1536, 1537, BCAST_LOG_PROB_ROWS, BCAST_SAMPLE_ROWS]))


@pytest.mark.parametrize("name", list(ALL_CONFIGS))
def test_plan_restatement_matches_the_library(name):
    cfg = ALL_CONFIGS[name]
    lib = _lib.load()
    h = MDNHyper(*cfg)
    c = h.c_config()
    P = plan(*cfg)
    assert lib.sbi_amd_mdn_param_count(c) == P["n_params"] == h.param_count()
    assert lib.sbi_amd_mdn_packed_floats(c) == P["img_floats"]
    for n in ROW_EDGES:
        assert lib.sbi_amd_mdn_train_workspace_floats(c, n) == workspace_floats(cfg, n), n


def test_configurations_sit_on_the_edges_they_are_listed_for():
    assert {name: ksh(c) for name, c in CONFIGS.items()} == dict(corner=16, floor=13, ksh13=13, ksh16=16, wideC=13,
                                                                 oneK=13, thinH=13, defaults=13)
    assert ksh((1, 1, 52, 1)) == 13 and ksh((1, 1, 53, 1)) == 16          # the switch itself
    corner, floor = plan(*CONFIGS["corner"]), plan(*CONFIGS["floor"])
    assert (corner["KS1"], corner["ld1"], corner["R"], corner["RP"]) == (16, 66, 153, 160)
    assert (floor["U"], floor["R"], floor["n_params"]) == (0, 3, 10)
    p = plan(*CONFIGS["ksh13"])
    assert p["R"] == 15 and p["K"] * p["D"] == 16
    p = plan(*CONFIGS["ksh16"])
    assert p["R"] == 21 and p["KS1"] == 2 and p["C"] == 5
    p = plan(*CONFIGS["wideC"])
    assert (p["C"], p["KS1"], p["K"] * p["D"], p["K"] * p["U"]) == (63, 16, 33, 165)
    p = plan(*CONFIGS["oneK"])
    assert (p["K"], p["K"] * p["D"], p["K"] * p["U"]) == (1, 16, 120)
    assert CONFIGS["thinH"][2:] == (1, 16)
    for cfg in ALL_CONFIGS.values():                                       # the one-observation kernels always fit
        assert bcast_lds_bytes(cfg) <= LDS_LIMIT_BYTES


def test_row_counts_land_on_their_wave_counts_chunks_and_trips():
    for name in WAVE_CONFIGS:
        assert [waves(CONFIGS[name], n) for n in WAVE_ROWS] == [1, 2, 2, 4], name
    # the corner at 4 waves: the launch nearest the LDS limit that the plan ever makes (about 150 KiB of 160)
    assert waves(CONFIGS["corner"], 16321) == 4
    assert 144 * 1024 < paired_lds_bytes(CONFIGS["corner"], 4) <= LDS_LIMIT_BYTES
    assert all(paired_lds_bytes(c, 4) <= paired_lds_bytes(CONFIGS["corner"], 4) for c in ALL_CONFIGS.values())
    small = ROWS + CHUNK_ROWS + [n for n, _ in XROWS_CASES]
    assert all(waves(c, n) == 1 for c in ALL_CONFIGS.values() for n in small)
    assert [nchunks(n) for n in CHUNK_ROWS] == [1, 1, 1, 2, 3]
    assert [nchunks(n) for n in ROWS] == [1, 1, 1] and [nchunks(n) for n in WAVE_ROWS] == [16, 16, 32, 32]
    assert [nchunks(n) for n, _ in XROWS_CASES] == [1, 1, 1, 2, 2]
    assert all(1 < r < n or r > n for n, r in XROWS_CASES)
    assert any(r > n for n, r in XROWS_CASES) and any(1 < r < n and n > 512 for n, r in XROWS_CASES)
    # the one-observation kernels: the grid is capped and the workgroups go round a second time
    assert bcast_grid_and_trips(32768, False) == (512, 1) and bcast_grid_and_trips(131072, True) == (512, 1)
    assert bcast_grid_and_trips(BCAST_LOG_PROB_ROWS, False) == (512, 2)
    assert bcast_grid_and_trips(BCAST_SAMPLE_ROWS, True) == (512, 2)
    assert BCAST_LOG_PROB_ROWS % 16 == 1 and BCAST_SAMPLE_ROWS % 64 == 1      # a last partial tile of one row
    rows = bcast_subset(BCAST_LOG_PROB_ROWS, False)
    assert set(range(0, 16)) | set(range(32752, 32785)) == set(rows.tolist())
    rows = bcast_subset(BCAST_SAMPLE_ROWS, True)
    assert set(range(0, 64)) | set(range(131008, 131137)) == set(rows.tolist())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_references_are_finite_and_have_gradients(name):
    cfg = CONFIGS[name]
    o32, o64, _, theta, x = mdn_pair_cpu(*cfg)
    for what, th in (("in-distribution", theta), ("stress", 3.0 * theta), ("far tail", 10.0 * theta)):
        for xx in (x, x[:1]):
            r32, r64 = ref_log_prob(o32, th, xx), ref_log_prob(o64, th, xx)
            assert torch.isfinite(r32).all() and torch.isfinite(r64).all(), what
            print(f"{name} {what} x_rows={xx.shape[0]}: |o32-f64|={(r32.double() - r64).abs().max():.3e} "
                  f"max|ref|={r64.abs().max():.1f}")
    for xx in (x, x[:1]):
        for o in (o32, o64):
            losses, g, gth = training_reference(o, theta, xx, training_weights(POOL_ROWS))
            assert torch.isfinite(losses).all() and torch.isfinite(g).all() and torch.isfinite(gth).all()
            assert g.abs().max() > 0 and gth.abs().max() > 0
    for o in (o32, o64):              # the uniform-weight case
        _, g, gth = training_reference(o, theta, x, torch.full((POOL_ROWS,), 1.0 / POOL_ROWS))
        assert torch.isfinite(g).all() and g.abs().max() > 0 and gth.abs().max() > 0


def _left_out(o64, n, D, K, x):
    return int((~ref_pick(o64, sample_draws(n, D, K)[2], x)[1]).sum())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_sampling_draws_stay_off_the_cumulative_boundaries(name):
    """The cap `left_out <= n // 100` of tests/test_mdn_gpu.py at every row count the GPU tests draw uniforms for."""
    D, C, H, K = CONFIGS[name]
    _, o64, _, _, x = mdn_pair_cpu(D, C, H, K)
    for n in ROWS:
        for xx in (x[:n], x[:1]):
            assert _left_out(o64, n, D, K, xx) <= n // 100, (n, xx.shape[0])
    for n, r in XROWS_CASES:
        assert _left_out(o64, n, D, K, x[:r][torch.arange(n) % r]) <= n // 100, (n, r)
    if name in WAVE_CONFIGS or name == "corner":
        for n in ([16321] if name == "corner" else WAVE_ROWS):
            assert _left_out(o64, n, D, K, large_pool(name, n)[1]) <= n // 100, n
    if name in BCAST_CONFIGS:
        rows = bcast_subset(BCAST_SAMPLE_ROWS, True)
        u = sample_draws(BCAST_SAMPLE_ROWS, D, K)[2][rows]
        assert int((~ref_pick(o64, u, x[7:8])[1]).sum()) <= rows.numel() // 100


@pytest.mark.parametrize("name", SELECT_CONFIGS)
def test_selection_ends_are_decided_by_the_weights(name):
    """u = 0 selects component 0 when its weight is positive, u = nextafter(1, 0) the last one when that one's weight
    is above fp32's resolution of 1: both by a wide margin on the rows the GPU test uses."""
    D, C, H, K = CONFIGS[name]
    _, o64, _, _, x = mdn_pair_cpu(D, C, H, K)
    with torch.no_grad():
        cum = o64.cumulative_weights(x[:81].double())
    assert (cum[:, 0] > 1e-3).all()
    if K > 1:
        assert (cum[:, K - 2] < 1.0 - 1e-3).all()


@pytest.mark.parametrize("name", list(SOFTPLUS_CONFIGS))
def test_softplus_shift_straddles_the_threshold(name):
    frac = softplus_fraction(name)
    print(f"{name}: {100 * frac:.1f} % of the shifted components' raw diagonal entries exceed 20")
    assert 0.2 <= frac <= 0.8
    D, C, H, K = SOFTPLUS_CONFIGS[name]
    o32, o64, est, theta, x = softplus_pair_cpu(name)
    off = {key: (o, cnt) for key, o, cnt, _ in est.net._slices()}["_unconstrained_diagonal_layer.bias"]
    for one_x in (False, True):
        xx = x[:1] if one_x else x[:333]
        th = softplus_theta(name, 333, one_x)
        for o in (o32, o64):
            assert torch.isfinite(ref_log_prob(o, th, xx)).all()
            assert torch.isfinite(ref_log_prob(o, theta[:333], xx)).all()
        _, g, gth = training_reference(o64, th, xx, training_weights(333))
        assert torch.isfinite(g).all() and torch.isfinite(gth).all()
        # the shifted components take responsibility on these rows: their raw-diagonal gradient (the `sg` factor of
        # the kernel's pass B) is a visible part of the reference gradient
        shifted = g[off[0]: off[0] + off[1]].reshape(K, D)[1::2].abs().max().item()
        print(f"{name} one_x={one_x}: max |d/d raw diagonal bias| of the shifted components {shifted:.3e}, "
              f"max |gradient| {g.abs().max():.3e}")
        assert shifted >= 1e-3 * g.abs().max().item()
