"""The training forward with two 16-row tiles per wave (nsf_flow_kernel, TW = 2).

At the default configuration the fused step's forward kernel gives each wave of an 8-wave workgroup two tiles (256 rows
per workgroup) when that halves the rounds of workgroups (nsf_flow_two_tiles): 32 769 ... 65 536 rows and 98 305 ...
131 072 rows among others.  The row counts below leave tile B of the last workgroup partly or wholly empty:

  32 769 = 128 workgroups + 1 row   (the last workgroup: one row in tile A of wave 0, every tile B empty)
  65 519 = 256 workgroups - 17 rows (in the last workgroup tile B of wave 6 has 15 rows, wave 7's is empty)
  98 344 = 384 workgroups + 40 rows (the last: tile A of waves 0 - 2 live, 8 rows in the third; no tile B)

The per-row loss and the flat gradient of the fused step are held to the fp64 oracle with the yardsticks of
tests/test_parity_full_size_gpu.py, and a permutation of the rows must permute the per-row losses bit for bit:
a row gives the same result in tile A or tile B, in any wave and any workgroup."""

import pytest
import torch

from tests.helpers import matched_pair, row_parity

pytestmark = pytest.mark.gpu

SIZES = [32769, 65536 - 17, 98304 + 40]
CHUNK = 16384
KNOT_ULPS = 2.0     # as in tests/test_parity_full_size_gpu.py


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(n, 10, generator=g) * (0.1**0.5)
    x = theta + (0.1**0.5) * torch.randn(n, 10, generator=g)
    return theta, x


def _oracle_pass(oracle, est, theta, x, keep=None):
    """fp64 autograd through the oracle: (per-row loss, flat grad of sum_n keep_n loss_n / N, per-row d loss / d theta)"""
    n = theta.shape[0]
    oracle.double()
    oracle.zero_grad()
    losses, gth = [], []
    for i in range(0, n, CHUNK):
        th = theta[i : i + CHUNK].double().requires_grad_(True)
        l = oracle.loss(th, x[i : i + CHUNK].double())
        w = torch.ones(l.shape[0], dtype=torch.float64) if keep is None else keep[i : i + CHUNK].double()
        ((l * w).sum() / n).backward()
        losses.append(l.detach())
        gth.append(th.grad * n)
    named = dict(oracle.named_parameters())
    flat = torch.zeros(est.net.flat_params.numel(), dtype=torch.float64)
    for key, off, cnt, _ in est.net._slices():
        flat[off : off + cnt] = named["net." + key].grad.reshape(-1)
    oracle.float()
    return torch.cat(losses), flat, torch.cat(gth)


def _oracle_log_prob32(oracle, theta, x):
    with torch.no_grad():
        return torch.cat([oracle.log_prob(theta[i : i + CHUNK], x[i : i + CHUNK])[0]
                          for i in range(0, theta.shape[0], CHUNK)])


def _hip_pass(est, theta, x, keep=None):
    from sbi_amd.neural_nets.estimators.nsf_flow import loss_fwd_bwd, train_workspace

    n = theta.shape[0]
    grad = torch.empty_like(est.net.flat_params.data)
    ws = train_workspace(est.net, n, "cuda")
    ws.fill_(float("nan"))
    rw = None if keep is None else (keep / n).cuda().contiguous()
    losses, gth = loss_fwd_bwd(est.net, theta.cuda().contiguous(), x.cuda().contiguous(), rw, 1.0 / n, grad,
                               want_grad_theta=True, workspace=ws)
    torch.cuda.synchronize()
    return losses.cpu(), grad.cpu(), gth.cpu() * n


@pytest.mark.parametrize("n", SIZES)
def test_ragged_two_tile_loss_and_gradient_match_oracle(n):
    from tests.helpers import spline_knot_distances

    oracle, est, _, _ = matched_pair(D=10, C=10)
    theta, x = _data(n, seed=n)
    loss_h, g_h, gth_h = _hip_pass(est, theta, x)
    assert loss_h.shape == (n,)
    assert torch.isfinite(loss_h).all() and torch.isfinite(g_h).all() and torch.isfinite(gth_h).all()

    # per-row loss against the fp32 and fp64 oracle (the yardsticks of the full-size log_prob / training tests)
    loss32 = -_oracle_log_prob32(oracle, theta, x)
    e_l = (loss_h - loss32).abs().max().item()
    assert e_l <= 1e-5 + 1e-5 * loss32.abs().max().item(), e_l
    loss64, g64, gth64 = _oracle_pass(oracle, est, theta, x)
    rp64, ro64 = row_parity(loss_h, loss64), row_parity(loss32, loss64)
    print(f"n={n}: loss |hip-o32|={e_l:.3e}; vs f64 worst {rp64['worst_scaled']:.2f} x bound, beyond "
          f"{rp64['exceed_frac']:.3%} (o32: {ro64['worst_scaled']:.2f}, {ro64['exceed_frac']:.3%})")
    assert rp64["exceed_frac"] <= 0.01 and rp64["worst_scaled"] <= 4.0, rp64

    # the gradient: knot-straddling rows (two-valued derivative) set aside after checking that they are such rows
    row_err = (gth_h.double() - gth64).abs().max(dim=1).values / gth64.abs().max().item()
    outliers = (row_err > 1e-3).nonzero().flatten()
    assert outliers.numel() <= 8, "more knot-straddling rows than one-ulp knot differences can explain"
    if outliers.numel():
        near = spline_knot_distances(oracle, theta[outliers], x[outliers]).min(dim=1).values
        assert (near <= KNOT_ULPS).all(), (outliers.tolist(), near.tolist())
    assert row_err[row_err <= 1e-3].max().item() <= 5e-4
    keep = torch.ones(n)
    keep[outliers] = 0.0
    _, g64k, _ = _oracle_pass(oracle, est, theta, x, keep)
    _, g_hk, _ = _hip_pass(est, theta, x, keep)
    scale = g64.abs().max().item()
    e_keep = (g_hk.double() - g64k).abs().max().item() / scale
    print(f"n={n}: grad vs f64 {e_keep:.3e} of max|grad| ({outliers.numel()} knot-straddling rows set aside)")
    assert e_keep <= 5e-5, e_keep


@pytest.mark.parametrize("n", SIZES)
def test_ragged_log_prob_matches_oracle(n):
    oracle, est, _, _ = matched_pair(D=10, C=10)
    theta, x = _data(n, seed=n + 1)
    ref = _oracle_log_prob32(oracle, theta, x)
    got = est.log_prob(theta.cuda(), x.cuda())[0].cpu()
    assert torch.isfinite(got).all()
    e_o = (got - ref).abs().max().item()
    assert e_o <= 1e-5 + 1e-5 * ref.abs().max().item(), e_o
    rp = row_parity(got, ref)
    assert rp["exceed_frac"] <= 0.01 and rp["worst_scaled"] <= 4.0, rp


@pytest.mark.parametrize("n", [65536, 98304 + 40])
def test_permuted_rows_give_permuted_results_bit_for_bit(n):
    """Rows move between tile A and tile B, waves and workgroups: the fused step's per-row loss and log_prob follow
    them exactly."""
    _, est, _, _ = matched_pair(D=10, C=10)
    theta, x = _data(n, seed=7)
    g = torch.Generator().manual_seed(11)
    p = torch.randperm(n, generator=g)
    l0, _, _ = _hip_pass(est, theta, x)
    l1, _, _ = _hip_pass(est, theta[p], x[p])
    assert torch.equal(l1, l0[p])
    lp0 = est.log_prob(theta.cuda(), x.cuda())[0].cpu()
    lp1 = est.log_prob(theta[p].cuda(), x[p].cuda())[0].cpu()
    assert torch.equal(lp1, lp0[p])
