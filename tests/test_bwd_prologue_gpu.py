"""The conditioner-input tile Bs of the wave-specialised backward kernel (csrc/nsf_train_kernel.h), and the rest of
the row waves' tile prologue.

Bs ([z_id ; context ; 1 ; 0 ...]: the B operand of d W0 and of every block's d Wc) is built per tile in the prologue,
which is pure critical path.  Its zero padding is written once per launch; a tile rewrites only the column groups
that can hold something else, which depends on in0 of BOTH mask parities (odd theta dims: they differ, and the column
that holds the 1 under one parity must be rewritten under the other).  A workgroup that walks two tiles builds the
second tile's rows over the first's.  The tests also pin what the prologue's neighbours may not change: the dead dim
slot of an odd last chunk (static and dynamic plan) and the input gradient at transform 0, asked for or not.

So: the whole flat gradient against the fp64 oracle (tolerance rule of tests/test_nsf_train_gpu.py: 2e-4 of the largest
entry overall, and per parameter block 2e-4 of the block's largest entry, floored at 1e-3 of the overall one), the
consumers of Bs -- the initial layer's and both context layers' weight and bias blocks -- named and held one by one,
the parameter gradient with grad_theta requested against not requested bit for bit, grad_theta itself against the
oracle (that file's rule for this call: 3e-4 of the largest entry), and a fresh NaN-filled workspace against a reused
one.  Row counts: just above the cooperative kernels' training limit, asked of the host routing, and 259 tiles + 5
rows, where four workgroups walk two tiles."""

from functools import lru_cache

import pytest
import torch

from tests.helpers import hip_training_pass, matched_pair, oracle_training_grad

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
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


def _rows(tag):
    return {"limit+11": _coop_training_limit() + 11, "two-tiles": 64 * (256 + 3) + 5}[tag]


CASES = {
    "default-ragged": (dict(D=10, C=10), "limit+11"),
    "default-two-tiles": (dict(D=10, C=10), "two-tiles"),      # Bs of a second tile over the first's rows
    "odd-dims": (dict(D=5, C=3, num_transforms=2), "limit+11"),   # dynamic plan; in0 = 5 / 6: the 1 moves between parities
    "even-dims": (dict(D=4, C=7, num_transforms=2), "limit+11"),
    "hidden64": (dict(D=10, C=10, hidden_features=64, num_transforms=2), "limit+11"),
}


@lru_cache(maxsize=None)
def _passes(case):
    """One case, computed once: the fp64 oracle's losses / gradients, and the HIP training pass with grad_theta
    requested (NaN-filled workspace) and not requested."""
    from sbi_amd.neural_nets.estimators.nsf_flow import loss_fwd_bwd, train_workspace

    cfg, rows = CASES[case]
    n = _rows(rows)
    oracle, est, theta, x = matched_pair(n=n, **cfg)
    assert theta.shape[0] == n and _throughput_routed(est, n)
    loss_ref, gref, gth_ref, _ = oracle_training_grad(oracle, est, theta, x)
    losses, got, gth, _ = hip_training_pass(est, theta, x)
    grad2 = torch.full_like(est.net.flat_params.data, float("nan"))
    ws = train_workspace(est.net, n, "cuda")
    ws.fill_(float("nan"))
    losses2, none = loss_fwd_bwd(est.net, theta.cuda().contiguous(), x.cuda().contiguous(), None, 1.0 / n, grad2,
                                 want_grad_theta=False, workspace=ws)
    torch.cuda.synchronize()
    assert none is None
    return dict(est=est, n=n, loss_ref=loss_ref, gref=gref, gth_ref=gth_ref, losses=losses, got=got, gth=gth,
                losses_no_gth=losses2.cpu(), got_no_gth=grad2.cpu())


def _bs_consumers(est):
    """(name, indices) of the parameter blocks whose gradient has Bs as its B operand."""
    h = est.net.hyper
    sel = [(key, torch.arange(off, off + cnt)) for key, off, cnt, _ in est.net._slices()
           if "initial_layer" in key or "context_layer" in key]
    assert len(sel) == h.num_transforms * (2 + 2 * h.num_blocks), [k for k, _ in sel]
    return sel


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_matches_the_oracle_block_by_block(case):
    r = _passes(case)
    est, got, gref, loss_ref = r["est"], r["got"].double(), r["gref"], r["loss_ref"]
    assert torch.isfinite(r["got"]).all() and torch.isfinite(r["losses"]).all()
    assert (r["losses"].double() - loss_ref).abs().max() <= 1e-5 + 1e-5 * loss_ref.abs().max()
    scale = gref.abs().max().item()
    rel = (got - gref).abs().max().item() / scale
    print(f"{case} n={r['n']}: grad max|ref|={scale:.3e} rel err={rel:.3e}")
    assert rel <= 2e-4, f"flat gradient mismatch: rel {rel}"
    blocks = [(key, torch.arange(off, off + cnt)) for key, off, cnt, _ in est.net._slices()]
    worst = (0.0, "")
    for name, idx in blocks + _bs_consumers(est):
        a, b = got[idx], gref[idx]
        tol = 2e-4 * max(b.abs().max().item(), 1e-3 * scale) + 1e-7
        err = (a - b).abs().max().item()
        worst = max(worst, (err / tol, name))
        assert err <= tol, (name, err, tol)
    print(f"  tightest block: {worst[1]} at {worst[0]:.3f} of its tolerance")


@pytest.mark.parametrize("case", list(CASES))
def test_grad_theta_requested_or_not(case):
    """Whether the caller asks for grad_theta decides only what transform 0 does with its input gradient: the parameter
    gradient and the losses must not notice, and a requested grad_theta must be the oracle's."""
    r = _passes(case)
    assert torch.isfinite(r["got_no_gth"]).all()
    assert torch.equal(r["got_no_gth"].view(torch.int32), r["got"].view(torch.int32))
    assert torch.equal(r["losses_no_gth"].view(torch.int32), r["losses"].view(torch.int32))
    gth, ref = r["gth"].double(), r["gth_ref"]
    assert torch.isfinite(r["gth"]).all()
    err, scale = (gth - ref).abs().max().item(), ref.abs().max().item()
    print(f"{case}: grad_theta max|ref|={scale:.3e} rel err={err / scale:.3e}")
    assert err <= 3e-4 * scale


def test_gradient_does_not_depend_on_the_previous_steps_workspace():
    """Step on batch A, then on batch B; a fresh stepper (NaN-filled workspace) steps on B only from the same state.
    Two tiles per workgroup for some: a Bs column that a tile no longer rewrites but should, or anything else that
    leaks from the previous tile or step, would differ between the two."""
    from sbi_amd.inference.trainers.fused import FusedTrainStep

    n = _rows("two-tiles")
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
