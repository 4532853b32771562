"""The thin remainder of the 50-wide hidden layers at the benchmarked size.

sbi's default hidden_features = 50 fills 4 m-tiles of 16 features, the 4th with only features 48 and 49.  The static-
layout backward kernel (the default configuration at 65 536 rows) computes their weight-gradient entries on 4x4x1 MFMAs
instead of padded 16x16 tiles.  A mistake there is confined to 2 of 50 features, which the
whole-vector tolerances of tests/test_parity_full_size_gpu.py would hide: this test holds the entries such a mistake
touches to the fp64 oracle on their own, with the same yardsticks that test applies per parameter block."""

import pytest
import torch

from tests.helpers import matched_pair
from tests.test_parity_full_size_gpu import CHUNK, KNOT_ULPS, N, _bench_data

pytestmark = pytest.mark.gpu

THIN = slice(48, 50)   # the real features of m-tile 3


def _selections(est):
    """(name, flat indices) of every entry the thin remainder feeds, per transform."""
    sel = []
    for key, off, cnt, shape in est.net._slices():
        idx = torch.arange(off, off + cnt)
        if key.endswith("linear_layers.0.weight") or key.endswith("linear_layers.1.weight"):
            m = idx.reshape(shape)
            sel.append((key + "[48:50, :]", m[THIN].reshape(-1)))
            sel.append((key + "[:, 48:50]", m[:, THIN].reshape(-1)))
        elif key.endswith("linear_layers.0.bias") or key.endswith("linear_layers.1.bias"):
            sel.append((key, idx))
        elif key.endswith("final_layer.bias"):
            sel.append((key + " (bias column of d Wf)", idx))
        elif key.endswith("final_layer.weight"):
            sel.append((key + "[:, 48:50]", idx.reshape(shape)[:, THIN].reshape(-1)))
        elif key.endswith("initial_layer.weight") or key.endswith("context_layer.weight"):
            sel.append((key + "[48:50, :]", idx.reshape(shape)[THIN].reshape(-1)))
        elif key.endswith("initial_layer.bias") or key.endswith("context_layer.bias"):
            sel.append((key + "[48:50]", idx[THIN]))
    return sel


def test_thin_remainder_entries_match_autograd_65536():
    from sbi_amd.neural_nets.estimators.nsf_flow import loss_fwd_bwd, train_workspace
    from tests.helpers import spline_knot_distances

    oracle, est, _, _ = matched_pair(D=10, C=10)
    theta, x = _bench_data(seed=2)

    def oracle_pass(double, keep=None):
        oracle.zero_grad()
        dt = torch.float64 if double else torch.float32
        oracle.double() if double else oracle.float()
        gth = []
        for i in range(0, N, CHUNK):
            th = theta[i : i + CHUNK].to(dt).requires_grad_(True)
            l = oracle.loss(th, x[i : i + CHUNK].to(dt))
            w = torch.ones(l.shape[0], dtype=dt) if keep is None else keep[i : i + CHUNK].to(dt)
            ((l * w).sum() / N).backward()
            gth.append(th.grad * N)
        named = dict(oracle.named_parameters())
        flat = torch.zeros(est.net.flat_params.numel(), dtype=dt)
        for key, off, n_, _ in est.net._slices():
            flat[off : off + n_] = named["net." + key].grad.reshape(-1)
        oracle.float()
        return flat, torch.cat(gth)

    def hip_pass(keep=None):
        grad = torch.empty_like(est.net.flat_params.data)
        ws = train_workspace(est.net, N, "cuda")
        ws.fill_(float("nan"))
        rw = None if keep is None else (keep / N).cuda().contiguous()
        _, gth = loss_fwd_bwd(est.net, theta.cuda(), x.cuda(), rw, 1.0 / N, grad, want_grad_theta=True, workspace=ws)
        torch.cuda.synchronize()
        return grad.cpu(), gth.cpu() * N

    # ---- the input gradient, row by row (every row of the batch goes through features 48, 49 of every layer)
    _, gth64 = oracle_pass(True)
    _, gth_h = hip_pass()
    assert torch.isfinite(gth_h).all()
    row_err = (gth_h.double() - gth64).abs().max(dim=1).values / gth64.abs().max().item()
    outliers = (row_err > 1e-3).nonzero().flatten()
    assert outliers.numel() <= 8, "more knot-straddling rows than one-ulp knot differences can explain"
    if outliers.numel():      # the rows set aside must really straddle a knot (see test_parity_full_size_gpu.py)
        near = spline_knot_distances(oracle, theta[outliers], x[outliers]).min(dim=1).values
        assert (near <= KNOT_ULPS).all(), (outliers.tolist(), near.tolist())
    typical = row_err[row_err <= 1e-3].max().item()
    print(f"d loss / d theta: {outliers.numel()} knot-straddling rows, every other row within {typical:.3e}")
    assert typical <= 5e-4

    # ---- the parameter-gradient entries the thin remainder feeds, without the knot-straddling rows
    keep = torch.ones(N)
    keep[outliers] = 0.0
    g64, _ = oracle_pass(True, keep)
    g32, _ = oracle_pass(False, keep)
    g_h, _ = hip_pass(keep)
    assert torch.isfinite(g_h).all()
    scale = g64.abs().max().item()
    worst = []
    for name, idx in _selections(est):
        ref = g64[idx]
        den = max(ref.abs().max().item(), 1e-3 * scale)
        eh = (g_h[idx].double() - ref).abs().max().item() / den
        eo = (g32[idx].double() - ref).abs().max().item() / den
        worst.append((eh, name, eo, den / scale))
        # the per-block yardsticks of the full-size test, on these entries alone: within 5e-5 of the global maximum,
        # and within 5e-4 of their own maximum -- or no further from fp64 than twice the eager fp32 oracle is
        assert eh * den / scale <= 5e-5, (name, eh, den / scale)
        assert eh <= max(5e-4, 2.0 * eo), (name, eh, eo)
    worst.sort(reverse=True)
    for eh, name, eo, mag in worst[:5]:
        print(f"{name}: hip vs f64 {eh:.3e} (fp32 oracle {eo:.3e}), entries' max = {mag:.2e} of the global max")
