"""Partial-gradient write-out of the wave-specialised backward kernel (csrc/nsf_train_kernel.h).

At every transform boundary each grad wave stores its weight-gradient accumulators to the workgroup's partial slab.
The static-layout instantiation (the default configuration) does that with straight-line stores at compile-time
offsets (wo_static), every other instantiation with the guarded element-by-element code (write_tile / write_thin /
write_bias).  A mis-addressed or missing store is one wrong gradient entry, so the tests below compare the whole flat
gradient with the fp64 oracle (tolerance rule of tests/test_nsf_train_gpu.py), hold the entries of the edge tiles to
it block by block, and check that no slab word depends on what an earlier step left in the workspace.

Row counts are the smallest that reach this kernel: just above the cooperative kernels' training limit, which is
asked of the host routing code (sbi_amd_nsf_image_kind), not written down here."""

import pytest
import torch

from tests.helpers import hip_training_pass, matched_pair, oracle_training_grad

pytestmark = pytest.mark.gpu


def _coop_training_limit():
    """Largest row count whose training pass the host routes to the cooperative kernels (default configuration)."""
    from sbi_amd import _lib
    from sbi_amd.neural_nets.estimators.nsf_flow import NSFHyper

    lib, c = _lib.load(), NSFHyper(D=10, C=10).c_config()
    assert lib.sbi_amd_nsf_image_kind(c, 1, 1) == 1 and lib.sbi_amd_nsf_image_kind(c, 1 << 20, 1) == 0
    lo, hi = 1, 1 << 20          # kind(lo) == 1, kind(hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.sbi_amd_nsf_image_kind(c, mid, 1) == 1:
            lo = mid
        else:
            hi = mid
    return lo


def _throughput_routed(est, n):
    from sbi_amd import _lib

    return _lib.load().sbi_amd_nsf_image_kind(est.net.hyper.c_config(), n, 1) == 0


def _check_against_oracle(cfg, n, selections=None):
    """Per-row losses and flat gradient of one n-row training pass vs the fp64 oracle: tests/test_nsf_train_gpu.py's
    rule -- 2e-4 of the largest entry overall, and per parameter block 2e-4 of the block's largest entry (floored at
    1e-3 of the overall one) -- and the same per-block rule on every (name, indices) of `selections(est)`."""
    oracle, est, theta, x = matched_pair(n=n, **cfg)
    assert theta.shape[0] == n and _throughput_routed(est, n)
    loss_ref, gref, _, _ = oracle_training_grad(oracle, est, theta, x)
    losses, got, _, _ = hip_training_pass(est, theta, x)      # (NaN-filled workspace)
    assert torch.isfinite(got).all() and torch.isfinite(losses).all()
    got = got.double()
    assert (losses.double() - loss_ref).abs().max() <= 1e-5 + 1e-5 * loss_ref.abs().max()
    scale = gref.abs().max().item()
    rel = (got - gref).abs().max().item() / scale
    print(f"{cfg} n={n}: grad max|ref|={scale:.3e} rel err={rel:.3e}")
    assert rel <= 2e-4, f"flat gradient mismatch: rel {rel}"
    blocks = [(key, torch.arange(off, off + cnt)) for key, off, cnt, _ in est.net._slices()]
    worst = (0.0, "")
    for name, idx in blocks + (selections(est) if selections else []):
        a, b = got[idx], gref[idx]
        tol = 2e-4 * max(b.abs().max().item(), 1e-3 * scale) + 1e-7
        err = (a - b).abs().max().item()
        worst = max(worst, (err / tol, name))
        assert err <= tol, (name, err, tol)
    print(f"  tightest block: {worst[1]} at {worst[0]:.3f} of its tolerance")


def _edge_selections(est):
    """The entries that the edge tiles of the write-out store, per transform (default configuration: 50 hidden
    features = three full 16-feature tiles + features 48, 49 + the bias column; 29 spline parameters per dim = one
    full parameter tile + 13 of the second)."""
    h = est.net.hyper
    P = 3 * h.num_bins - 1
    sel = []
    for key, off, cnt, shape in est.net._slices():
        idx = torch.arange(off, off + cnt)
        if "linear_layers" in key and key.endswith("weight"):
            m = idx.reshape(shape)
            sel.append((key + "[48:50, :]", m[48:50].reshape(-1)))
            sel.append((key + "[:, 48:50]", m[:, 48:50].reshape(-1)))
        elif "linear_layers" in key and key.endswith("bias"):
            sel.append((key, idx))
        elif key.endswith("final_layer.weight") or key.endswith("final_layer.bias"):
            m = idx.reshape(shape[0] // P, P, -1)
            for d in range(m.shape[0]):
                sel.append((f"{key} dim {d}, parameters 16..{P - 1}", m[d, 16:].reshape(-1)))
        elif "transform_net" not in key:          # LULinear: lower / upper triangle, diagonal, bias
            sel.append((key, idx))
    assert len(sel) == h.num_transforms * (4 * 3 + 2 * (h.D // 2) + 4)
    return sel


def test_default_config_ragged_just_above_the_cooperative_limit():
    # fewer tiles than workgroups: most workgroups write their slabs from zero accumulators
    _check_against_oracle(dict(D=10, C=10), _coop_training_limit() + 11)


def test_default_config_two_tiles_one_tile_and_ragged_last_tile():
    # 260 tiles on 256 persistent workgroups: four walk two tiles, the others one; the last tile has 5 rows
    _check_against_oracle(dict(D=10, C=10), 64 * (256 + 3) + 5, _edge_selections)


@pytest.mark.parametrize("cfg", [
    dict(D=10, C=10, hidden_features=64, num_transforms=2),   # bias gradients through write_bias
    dict(D=4, C=4, num_bins=8, num_transforms=2),             # two parameter tiles per dim, 23 live parameters
    dict(D=5, C=3, num_transforms=2),                         # 3 / 2 transformed dims: the split last chunk and a full one
    dict(D=4, C=7, num_transforms=2),                         # 2 transformed dims
], ids=["hidden64", "bins8", "odd-dims", "even-dims"])
def test_dynamic_plan_guarded_paths(cfg):
    _check_against_oracle(cfg, _coop_training_limit() + 11)


def test_gradient_does_not_depend_on_the_previous_steps_workspace():
    """Step on batch A, then on batch B; a fresh stepper (NaN-filled workspace) steps on B only from the same state.
    A slab word that the write-out no longer stores would carry batch A's value in the first and NaN in the second."""
    from sbi_amd.inference.trainers.fused import FusedTrainStep

    n = _coop_training_limit() + 11
    _, est1, theta, x = matched_pair(D=10, C=10, n=2 * n)
    _, est2, _, _ = matched_pair(D=10, C=10, n=2 * n)
    assert _throughput_routed(est1, n)
    theta, x = theta.cuda(), x.cuda()
    tA, xA, tB, xB = theta[:n].contiguous(), x[:n].contiguous(), theta[n:].contiguous(), x[n:].contiguous()

    first = FusedTrainStep(est1, distributed=False)
    first.step(tA, xA)
    snap = first.snapshot()
    first.loss_and_grad(tB, xB)
    g_first = first.grad.clone()
    first.apply()

    fresh = FusedTrainStep(est2, distributed=False)
    fresh.restore(snap)
    fresh._workspace(n).fill_(float("nan"))
    fresh.loss_and_grad(tB, xB)
    g_fresh = fresh.grad.clone()
    fresh.apply()
    torch.cuda.synchronize()

    assert torch.isfinite(g_fresh).all()
    assert torch.equal(g_first.view(torch.int32), g_fresh.view(torch.int32))
    assert torch.equal(est1.net.flat_params.data.view(torch.int32), est2.net.flat_params.data.view(torch.int32))
