"""GPU parity of the maf_rqs / zuko_nsf kernels (csrc/maf_kernel.h, variants 0 and 1) over what the host code can
launch, not only the one-wave corner tests/test_maf_gpu.py and tests/test_zuko_gpu.py reach:

  (a) workgroup widths 2, 4, 8 at the thresholds of `maf_plan_for_rows`' halving loop (8161, 16321, 32641 rows),
  (b) the widths 3, 5, 6, 7 (and 1, 2) the LDS limit forces at 32641 rows, with C = 32, D = 16, NB = 4, NB = 0 and
      final layers of two and three full 16-m-tile pieces,
  (c) bit-identity of every per-row output of a wide launch with the same rows evaluated in one-wave launches,
  (d) the three condition-broadcast branches (x_rows == n, == 1, row % x_rows),
  (e) the row edges of the training pass (512-row chunks of four 128-row sub-chunks, the 4-way + tail reduction),
  (f) hidden widths on both sides of the KSH 13 / 16 switch and below one 16-tile,
  (g) clean E_LDS refusals past the real envelope.

Every test first asserts, through the host-only `sbi_amd_maf_plan_waves`, the workgroup width (or the refusal) it
claims to cover.  The kernels are called through the C ABI with outputs and workspace pre-filled with NaN.  T = 2
throughout (the fp64 oracle stays cheap); tolerances are the ones tests/test_maf_gpu.py and tests/test_zuko_gpu.py apply
to the same quantities."""
import functools

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.maf_flow import maf_packed_weights
from tests.parity_log import record
from tests.test_maf_gpu import maf_pair
from tests.test_maf_gpu import oracle_flat_grad as maf_flat_grad
from tests.test_zuko_gpu import oracle_flat_grad as zuko_flat_grad
from tests.test_zuko_gpu import zuko_pair

pytestmark = pytest.mark.gpu

NAN = float("nan")
ONE_WAVE_ROWS = 8160          # 510 x 16: the largest launch the halving loop leaves at one wave per workgroup
SMALL = (5, 3, 32, 8, 1)      # (D, C, H, K, NB): KSH == 16, one 16-tile of outputs per dim pair, ragged everywhere


def _id(case):
    return "v{}-D{}-C{}-H{}-K{}-NB{}".format(*case)


# ------------------------------------------------------------------------------------------------- pairs and calls
@functools.lru_cache(maxsize=None)
def pair(variant, D, C, H, K, NB, n_data=1000):
    """(oracle, HIP estimator, theta, x) on identical perturbed weights, built once per module."""
    if variant == 0:
        return maf_pair(D=D, C=C, n=n_data, hidden_features=H, num_transforms=2, num_bins=K, num_blocks=NB)
    return zuko_pair(D=D, C=C, n=n_data, hidden_features=[H] * (NB + 1), num_transforms=2, num_bins=K)


def waves(net, n):
    return _lib.load().sbi_amd_maf_plan_waves(net.hyper.c_config(), n)


def _call(net, name, *args):
    dev = net.flat_params.device
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(net.hyper.c_config(), *args, _lib.current_stream(dev))
    return rc


def hip_log_prob(net, theta, x, fill=NAN, check=True):
    n, D = theta.shape
    logp, noise = torch.full((n,), fill, device="cuda"), torch.full((n, D), fill, device="cuda")
    rc = _call(net, "sbi_amd_maf_log_prob", _lib.ptr(maf_packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(theta),
               _lib.ptr(x), n, x.shape[0], _lib.ptr(logp), _lib.ptr(noise))
    if check:
        _lib.check(rc, "maf_log_prob")
    torch.cuda.synchronize()
    return (logp.cpu(), noise.cpu()) if check else (rc, logp.cpu(), noise.cpu())


def hip_sample(net, noise, x, fill=NAN, check=True):
    n, D = noise.shape
    theta, ld = torch.full((n, D), fill, device="cuda"), torch.full((n,), fill, device="cuda")
    rc = _call(net, "sbi_amd_maf_sample", _lib.ptr(maf_packed_weights(net)), _lib.ptr(net.zstats), _lib.ptr(noise),
               _lib.ptr(x), n, x.shape[0], _lib.ptr(theta), _lib.ptr(ld))
    if check:
        _lib.check(rc, "maf_sample")
    torch.cuda.synchronize()
    return (theta.cpu(), ld.cpu()) if check else (rc, theta.cpu(), ld.cpu())


def hip_train(net, theta, x, w, fill=NAN, check=True):
    """(losses, flat parameter gradient, grad_theta) of sum_n w_n loss_n; everything the call writes starts as NaN."""
    n, D = theta.shape
    loss, gth = torch.full((n,), fill, device="cuda"), torch.full((n, D), fill, device="cuda")
    grad = torch.full_like(net.flat_params.data, fill)
    ws = torch.full((net.train_workspace_floats(n),), NAN, device="cuda")
    rc = _call(net, "sbi_amd_maf_loss_fwd_bwd", _lib.ptr(maf_packed_weights(net)), _lib.ptr(net.zstats),
               _lib.ptr(net.kernel_masks()), _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(w), 0.0,
               _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(gth), _lib.ptr(ws))
    if check:
        _lib.check(rc, "maf_loss_fwd_bwd")
    torch.cuda.synchronize()
    return (loss.cpu(), grad.cpu(), gth.cpu()) if check else (rc, loss.cpu(), grad.cpu(), gth.cpu())


def row_weights(n):
    return torch.linspace(0.5, 1.5, n) / n


def noise_for(n, D):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(5))


# ------------------------------------------------------------------------------------------------- fp64 references
def oracle_training(variant, oracle, est, theta, x, w, chunk=8192):
    """fp64 autograd of sum_n w_n loss_n: (losses, flat parameter gradient with the masks applied, d / d theta)."""
    n = theta.shape[0]
    oracle.double().zero_grad()
    th = theta.double().clone().requires_grad_(True)
    xx, ww = x.double(), w.double()
    losses = []
    for i in range(0, n, chunk):
        l = oracle.loss(th[i : i + chunk], xx[i : i + chunk])
        (l * ww[i : i + chunk]).sum().backward()
        losses.append(l.detach())
    gref = (maf_flat_grad if variant == 0 else zuko_flat_grad)(oracle, est, torch.float64)
    oracle.float()
    return torch.cat(losses), gref, th.grad.clone()


def check_log_prob(oracle, theta, x, got, key, tag):
    with torch.no_grad():
        ref = oracle.log_prob(theta, x)[0]
        ref64 = oracle.double().log_prob(theta.double(), x.double())[0]
        oracle.float()
    assert torch.isfinite(got).all()
    e_hip, e_ref = (got.double() - ref64).abs().max().item(), (ref.double() - ref64).abs().max().item()
    record(key + "_log_prob", tag, max_abs_hip_vs_oracle32=(got - ref).abs().max().item(), max_abs_hip_vs_f64=e_hip,
           max_abs_oracle32_vs_f64=e_ref, max_abs_ref=ref.abs().max().item())
    print(f"{tag} log_prob: |hip-o32|={(got - ref).abs().max():.3e} |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} "
          f"max|ref|={ref.abs().max():.1f}")
    assert (got - ref).abs().max() <= 1e-5 + 1e-5 * ref.abs().max()      # in-distribution rows
    assert e_hip <= 2.0 * e_ref + 1e-5


def check_sample(oracle, noise, x, got, got_ld, key, tag):
    with torch.no_grad():
        ref, ref_ld = oracle.sample_from_noise(noise, x)
        ref64, ref_ld64 = oracle.double().sample_from_noise(noise.double(), x.double())
        oracle.float()
    assert torch.isfinite(got).all() and torch.isfinite(got_ld).all()
    e_hip, e_ref = (got.double() - ref64).abs().max().item(), (ref.double() - ref64).abs().max().item()
    l_hip, l_ref = (got_ld.double() - ref_ld64).abs().max().item(), (ref_ld.double() - ref_ld64).abs().max().item()
    record(key + "_sample", tag, max_abs_hip_vs_f64=e_hip, max_abs_oracle32_vs_f64=e_ref,
           max_abs_logabsdet_hip_vs_f64=l_hip, max_abs_logabsdet_oracle32_vs_f64=l_ref)
    print(f"{tag} sample: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} logabsdet {l_hip:.3e} / {l_ref:.3e}")
    assert e_hip <= 2.0 * e_ref + 1e-5
    assert l_hip <= 2.0 * l_ref + 2e-5


def check_masked_zero(variant, est, got):
    if variant == 1:
        assert (got[est.net.mask_flat.cpu() == 0] == 0).all()
        return
    h = est.net.hyper
    for (key, off, cnt, shape), (_, _, kind) in zip(est.net._slices(), h.layer_entries() * h.num_transforms):
        if kind in (0, 2, 3):
            assert (got[off : off + cnt].reshape(shape)[h.mask(kind) == 0] == 0).all(), key


def check_training(variant, est, got, ref, key, tag, small, grad_only=False, rows=None):
    """`got` / `ref`: (losses, flat gradient, grad_theta).  `small` (n <= 3000): 2e-4 on the whole gradient and 3e-4
    per parameter block; otherwise the 1e-3 of the 65536-row test (knot-straddling rows bound it from below).
    `grad_only`: the rows are not in-distribution pairs, only the parameter gradient has a bar.
    `rows`: grad_theta, a per-row output, is held to its bar on these rows only (the caller looks at the others)."""
    (losses, grad, gth), (loss_ref, gref, gth_ref) = got, ref
    if rows is not None:
        gth, gth_ref = gth[rows], gth_ref[rows]
    grad = grad.double()
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all() and torch.isfinite(gth).all()
    e_l = (losses.double() - loss_ref).abs().max().item()
    scale = gref.abs().max().item()
    rel = (grad - gref).abs().max().item() / scale
    worst, worst_key = 0.0, ""
    for k, off, cnt, _ in est.net._slices():
        a, b = grad[off : off + cnt], gref[off : off + cnt]
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale)
        if e > worst:
            worst, worst_key = e, k
    e_th = (gth.double() - gth_ref).abs().max().item() / gth_ref.abs().max().item()
    record(key + "_train", tag, max_abs_loss_err_vs_f64=e_l, max_abs_loss=loss_ref.abs().max().item(),
           rel_grad_err_vs_f64=rel, worst_block_rel_err=worst, rel_grad_theta_err=e_th)
    print(f"{tag} train: loss err {e_l:.3e} (max {loss_ref.abs().max():.1f}) grad rel {rel:.3e} worst block {worst:.3e} "
          f"({worst_key}) d/dtheta rel {e_th:.3e}")
    assert grad_only or e_l <= 1e-5 + 1e-5 * loss_ref.abs().max().item()
    if small:
        assert worst <= 3e-4, f"{worst_key}: {worst:.3e}"
        assert rel <= 2e-4
    else:
        assert rel <= 1e-3
    assert grad_only or e_th <= 3e-4
    check_masked_zero(variant, est, grad)


def knot_distances(variant, oracle, theta, x):
    """Per row: the distance of the closest forward spline input to a knot of its spline (the tail bounds +-B count),
    evaluated in fp64 through the oracle, in units of the fp32 spacing at B (tests/helpers.py::spline_knot_distances
    does the same for the coupling flow)."""
    import numpy as np
    import torch.nn.functional as F

    captured = []
    if variant == 0:
        import oracle.maf_oracle as mod

        name, real = "unconstrained_rational_quadratic_spline", mod.unconstrained_rational_quadratic_spline

        def spy(inputs, uw, uh, ud, inverse=False, tail_bound=1.0, min_bin_width=1e-3, **kw):
            K = uw.shape[-1]
            w = min_bin_width + (1 - min_bin_width * K) * F.softmax(uw, dim=-1)
            knots = 2 * tail_bound * torch.cumsum(w, dim=-1)[..., :-1] - tail_bound
            d = torch.minimum((inputs[..., None] - knots).abs().min(dim=-1).values, (inputs.abs() - tail_bound).abs())
            captured.append((d / float(np.spacing(np.float32(tail_bound)))).detach())
            return real(inputs, uw, uh, ud, inverse=inverse, tail_bound=tail_bound, min_bin_width=min_bin_width, **kw)
    else:
        import oracle.zuko_oracle as mod

        name, real = "rqs_forward", mod.rqs_forward

        def spy(inputs, horizontal, vertical, derivatives):
            d = (inputs[..., None] - horizontal).abs().min(dim=-1).values
            captured.append((d / float(np.spacing(np.float32(horizontal.max().item())))).detach())
            return real(inputs, horizontal, vertical, derivatives)

    setattr(mod, name, spy)
    try:
        oracle.double()
        with torch.no_grad():
            oracle.log_prob(theta.double(), x.double())
    finally:
        setattr(mod, name, real)
        oracle.float()
    return torch.cat([c.reshape(theta.shape[0], -1) for c in captured], dim=1).min(dim=1).values


def relu_distances(oracle, theta, x):
    """zuko's hyper-nets are ReLU MLPs: d log p / d theta is two-valued as well where a hidden pre-activation is 0.
    Per row: the smallest |pre-activation| of the oracle in fp64, in units of the rounding error bound of its fp32
    evaluation, depth * (fan_in + 1) * 2^-24 * (|W| |h| + |b|) (an fp32 dot product of fan_in terms plus the bias; the
    inputs of the layer at `depth` carry the same relative error from each layer before it)."""
    from torch import nn

    from oracle.zuko_oracle import MaskedMLP

    captured, hooks = [], []

    def make(depth):
        def hook(mod, inp, out):
            w = (mod.mask * mod.weight).abs()
            bound = depth * (w.shape[1] + 1) * 2.0**-24 * (inp[0].abs() @ w.t() + mod.bias.abs())
            captured.append((out.abs() / bound).min(dim=-1).values.detach())
        return hook

    for mlp in oracle.modules():
        if isinstance(mlp, MaskedMLP):
            linears = [m for m in mlp if isinstance(m, nn.Linear)]
            hooks += [lin.register_forward_hook(make(depth)) for depth, lin in enumerate(linears[:-1], 1)]
    try:
        oracle.double()
        with torch.no_grad():
            oracle.log_prob(theta.double(), x.double())
    finally:
        for h in hooks:
            h.remove()
        oracle.float()
    return torch.stack(captured, dim=1).min(dim=1).values


RELU_WINDOW = 2.0      # x the bound above: the first layer's input (z-scored theta, the previous transform's output) is
                       # itself an fp32 result


def knot_window(case):
    """How far (in fp32 spacings at the tail bound B) from a knot an fp32 evaluation can still pick the other bin:
    knot k is 2 B cumsum_k(widths) - B, and a K-term fp32 running sum of widths that add up to 1 carries at most
    (K - 1) 2^-24 of absolute error, i.e. 2 B (K - 1) 2^-24 on the knot; the spline input itself (the previous
    transform's output, |.| <= B in the spline's domain) carries the few spacings by which an fp32 evaluation of a
    transform differs from fp64 (the eager fp32 oracle's own error, `max_abs_oracle32_vs_f64` of the sample records:
    <= 2e-6), 8 spacings allowed."""
    import numpy as np

    B = 3.0 if case[0] == 0 else 5.0
    return 2 * B * (case[4] - 1) * 2.0**-24 / float(np.spacing(np.float32(B))) + 8.0


def check_grad_theta_rows_off_the_bar_straddle_a_knot(case, oracle, theta, x, gth, gth_ref, key, tag):
    """The RQ spline is C1: at a knot d log p / d theta is two-valued (tests/test_parity_full_size_gpu.py), so among
    tens of thousands of rows a few disagree with fp64 about a bin and miss every bar.  Each such row must be shown,
    in fp64, to sit within `knot_window` of a knot (or, zuko, to have a ReLU pre-activation within rounding of 0:
    `relu_distances`) -- a row that is merely wrong fails here -- and there may be only a handful (8, as in the
    full-size test).  Returns those rows.

    Measured at 32641 rows (profiles/parity_maf_envelope.json, `*_knot_rows`): no such row in 12 of the 20 wide cases,
    one in each of the others -- six knot rows (d / d theta off by 0.012 .. 0.25 of the maximum, 0.4 .. 2.6 spacings from
    a knot; e.g. v0 D14 C32 H32 K16 NB2: row 690, 0.59 spacings, 0.20) and two zuko ReLU rows (v1 D10 C10 H50 K10 NB1:
    row 7572, 1.5e-3, 0.015 rounding bounds from a kink, 696 spacings from any knot; v1 D16 C32 H64 K8 NB2: row 31821,
    6.2e-4, 0.0017 bounds).  Ordinary rows sit hundreds to thousands of either unit away."""
    err = (gth.double() - gth_ref).abs().amax(dim=1) / gth_ref.abs().max()
    out = torch.nonzero(err > 3e-4).flatten()
    near = knot_distances(case[0], oracle, theta[out], x[out]) if out.numel() else torch.zeros(0)
    relu = relu_distances(oracle, theta[out], x[out]) if out.numel() and case[0] == 1 else torch.full_like(near, 1e30)
    record(key + "_knot_rows", tag, rows=int(out.numel()), worst_rel_grad_theta_err=err.max().item(),
           knot_distance_fp32_spacings=[float(v) for v in near.tolist()], window=knot_window(case),
           relu_distance_rounding_bounds=[float(v) for v in relu.tolist()])
    print(f"{tag} grad_theta rows beyond 3e-4: {out.tolist()} rel err {err[out].tolist()} knot distance (fp32 spacings "
          f"at B) {near.tolist()} window {knot_window(case):.1f} relu distance (rounding bounds) {relu.tolist()}")
    assert out.numel() <= 8
    assert ((near <= knot_window(case)) | (relu <= RELU_WINDOW)).all()
    return out


# ------------------------------------------------------------------------------------------ (a), (b), (c): wide launches
# (case, rows, waves per workgroup the plan must answer).  (a): the halving thresholds on the small KSH == 16 config of
# each variant, and zuko's default hidden width (KSH == 13) at eight waves.
WIDE = [((v,) + SMALL, n, nw) for v in (0, 1) for n, nw in ((8161, 2), (16321, 4), (32641, 8))]
WIDE += [((1, 10, 10, 50, 10, 1), 32641, 8)]
# (b): widths the 160 KiB LDS limit forces at 32641 rows (the weight image leaves room for that many waves' scratch).
# D14 K16: 42 final-layer m-tiles = two full pieces + 10; D16 K8: exactly two full pieces; D16 K16: three.
WIDE += [(c, 32641, nw) for c, nw in (
    ((0, 14, 32, 32, 16, 2), 3), ((0, 16, 32, 50, 8, 1), 5), ((0, 4, 32, 50, 16, 4), 6), ((0, 16, 32, 32, 8, 2), 7),
    ((0, 16, 32, 32, 16, 1), 2), ((0, 16, 4, 64, 8, 2), 1),            # one wave: the largest fitting neighbour of (g)
    ((0, 5, 3, 32, 8, 0), 8),                                           # NB = 0
    ((1, 14, 32, 32, 16, 1), 3), ((1, 16, 32, 50, 8, 1), 5), ((1, 4, 32, 50, 16, 4), 6), ((1, 8, 32, 32, 16, 1), 7),
    ((1, 16, 32, 64, 8, 2), 1), ((1, 5, 3, 32, 8, 0), 8))]
WIDE_IDS = [f"{_id(c)}-n{n}-w{nw}" for c, n, nw in WIDE]


@functools.lru_cache(maxsize=None)
def wide_run(case, n):
    """Every per-row output and the parameter gradient of ONE launch each over all n rows."""
    oracle, est, theta, x = pair(*case, n_data=n)
    noise, w = noise_for(n, case[1]), row_weights(n)
    th_d, x_d = theta.cuda(), x.cuda()
    logp, z = hip_log_prob(est.net, th_d, x_d)
    samples, ld = hip_sample(est.net, noise.cuda(), x_d)
    back = hip_log_prob(est.net, samples.cuda(), x_d)[1]
    losses, grad, gth = hip_train(est.net, th_d, x_d, w.cuda())
    return dict(noise=noise, w=w, logp=logp, z=z, samples=samples, ld=ld, back=back, losses=losses, grad=grad, gth=gth)


def boundary_rows(n, nw):
    """First and last 512 rows plus the 32 rows straddling two workgroup boundaries (a workgroup owns 16 nw rows)."""
    wg = 16 * nw
    groups = (n + wg - 1) // wg
    parts = [torch.arange(0, 512), torch.arange(n - 512, n)]
    parts += [torch.arange(b - 16, b + 16) for b in (wg * (groups // 3), wg * (2 * groups // 3))]
    return torch.unique(torch.cat(parts))


@pytest.mark.parametrize("case,n,nw", WIDE, ids=WIDE_IDS)
def test_wide_launch_matches_the_fp64_oracle(case, n, nw):
    """log_prob, sample and the training pass at the stated workgroup width against the oracle.  Per-row outputs are
    compared on `boundary_rows` (test_wide_launch_is_bit_identical_to_one_wave_launches licenses the subsample), the
    parameter gradient, a sum over all rows, in full.  d loss / d theta is held to its 3e-4 on `boundary_rows`; over
    all rows, every row beyond it must be a verified knot-straddling row."""
    oracle, est, theta, x = pair(*case, n_data=n)
    assert waves(est.net, n) == nw
    run = wide_run(case, n)
    idx, tag = boundary_rows(n, nw), f"{_id(case)} n{n} w{nw}"
    for k in ("logp", "z", "samples", "ld", "losses", "gth", "grad"):
        assert torch.isfinite(run[k]).all(), k
    check_log_prob(oracle, theta[idx], x[idx], run["logp"][idx], "maf_envelope_wide", tag)
    check_sample(oracle, run["noise"][idx], x[idx], run["samples"][idx], run["ld"][idx], "maf_envelope_wide", tag)
    assert (run["back"] - run["noise"]).abs().max() <= 2e-4          # round trip on the device, every row
    ref = oracle_training(case[0], oracle, est, theta, x, run["w"])
    check_training(case[0], est, (run["losses"], run["grad"], run["gth"]), ref, "maf_envelope_wide", tag, small=False,
                   rows=idx)
    check_grad_theta_rows_off_the_bar_straddle_a_knot(case, oracle, theta, x, run["gth"], ref[2], "maf_envelope_wide", tag)


@pytest.mark.parametrize("case,n,nw", WIDE, ids=WIDE_IDS)
def test_wide_launch_is_bit_identical_to_one_wave_launches(case, n, nw):
    """One wave owns 16 rows whatever the workgroup width: log-probs, noise, samples, logabsdet, per-row losses and
    grad_theta rows of the wide launch equal, bit for bit, the same rows evaluated in launches of <= 8160 rows (one
    wave per workgroup) with the same per-row weights."""
    oracle, est, theta, x = pair(*case, n_data=n)
    assert waves(est.net, n) == nw
    run = wide_run(case, n)
    for s in range(0, n, ONE_WAVE_ROWS):
        e = min(n, s + ONE_WAVE_ROWS)
        assert waves(est.net, e - s) == 1
        th_d, x_d = theta[s:e].cuda().contiguous(), x[s:e].cuda().contiguous()
        logp, z = hip_log_prob(est.net, th_d, x_d)
        samples, ld = hip_sample(est.net, run["noise"][s:e].cuda().contiguous(), x_d)
        losses, _, gth = hip_train(est.net, th_d, x_d, run["w"][s:e].cuda().contiguous())
        for name, got in (("logp", logp), ("z", z), ("samples", samples), ("ld", ld), ("losses", losses), ("gth", gth)):
            assert torch.equal(run[name][s:e], got), f"{name} rows {s}..{e}"


# ------------------------------------------------------------------------------------------ (d): condition broadcast
@pytest.mark.parametrize("n,x_rows", [(333, 1), (333, 7), (8161, 100), (8161, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("variant", [0, 1])
def test_condition_broadcast_equals_the_expanded_condition(variant, n, x_rows):
    """x_rows == 1 and row % x_rows (n % x_rows != 0) against x_rows == n on x[i % x_rows]: bit-identical log_prob,
    noise, samples, logabsdet, losses, grad_theta and parameter gradient; the latter also against fp64 autograd on the
    expanded x.  The short condition is the head of an n-row buffer of OTHER rows, so an index that ignores x_rows
    reads defined, different data.  (8161 rows from one x row is the DirectPosterior.sample launch.)

    Rows whose grad_theta misses fp64 must be verified knot-straddling rows; where there is one (v0, 8161 rows from one
    x row: row 269, 0.39 fp32 spacings from a knot, d / d theta off by 0.114 of the maximum, parameter gradient by
    1.05e-3) the parameter gradient is compared with that row's weight set to 0 on both sides."""
    case = (variant,) + SMALL
    oracle, est, theta, x = pair(*case, n_data=max(n, 1000))
    assert waves(est.net, n) == (2 if n == 8161 else 1)
    theta, x_buf = theta[:n].cuda().contiguous(), x[:n].flip(0).cuda().contiguous()
    x_short = x_buf[:x_rows]
    x_exp = x_short[torch.arange(n, device="cuda") % x_rows].contiguous()
    noise, w = noise_for(n, case[1]).cuda(), row_weights(n).cuda()
    for name, a, b in zip(("logp", "noise"), hip_log_prob(est.net, theta, x_short), hip_log_prob(est.net, theta, x_exp)):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    for name, a, b in zip(("samples", "logabsdet"), hip_sample(est.net, noise, x_short), hip_sample(est.net, noise, x_exp)):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    got, exp = hip_train(est.net, theta, x_short, w), hip_train(est.net, theta, x_exp, w)
    for name, a, b in zip(("losses", "grad", "grad_theta"), got, exp):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    ref = oracle_training(variant, oracle, est, theta.cpu(), x_exp.cpu(), w.cpu())
    tag = f"{_id(case)} n{n} x_rows{x_rows}"
    straddling = check_grad_theta_rows_off_the_bar_straddle_a_knot(case, oracle, theta.cpu(), x_exp.cpu(), got[2], ref[2],
                                                                   "maf_envelope_broadcast", tag)
    if straddling.numel():
        # a row that straddles a knot carries weight ~1 / n: at 8161 rows that alone can exceed the 1e-3 which the
        # 65536-row test allows for such rows.  Compare the gradient of the other rows (weight 0 on both sides).
        w = w.clone()
        w[straddling.cuda()] = 0.0
        got = hip_train(est.net, theta, x_short, w)
        ref = oracle_training(variant, oracle, est, theta.cpu(), x_exp.cpu(), w.cpu())
    check_training(variant, est, got, ref, "maf_envelope_broadcast", tag, small=n <= 3000, grad_only=True)


# ------------------------------------------------------------------------------------------ (e): row edges
ROW_EDGES = [1, 15, 16, 17, 127, 128, 129, 511, 512, 513, 3000]      # 3000 rows: six chunks, 4-way loop + tail of two


@pytest.mark.parametrize("n", ROW_EDGES)
@pytest.mark.parametrize("variant", [0, 1])
def test_row_edges_of_the_training_pass(variant, n):
    """Wave-tile, sub-chunk (128) and chunk (512) boundaries +-1 row, one row, and a chunk count that runs both loops of
    the reduction: losses, the full parameter gradient and grad_theta against fp64 autograd, masked entries exactly
    zero, two calls bit-identical; log_prob and sample at the same row counts."""
    case = (variant,) + SMALL
    oracle, est, theta, x = pair(*case, n_data=3000)
    assert waves(est.net, n) == 1
    theta, x, w, noise = theta[:n], x[:n], row_weights(n), noise_for(n, case[1])
    tag = f"{_id(case)} n{n}"
    th_d, x_d, w_d = theta.cuda().contiguous(), x.cuda().contiguous(), w.cuda()
    got = hip_train(est.net, th_d, x_d, w_d)
    check_training(variant, est, got, oracle_training(variant, oracle, est, theta, x, w), "maf_envelope_rows", tag,
                   small=True)
    for name, a, b in zip(("losses", "grad", "grad_theta"), got, hip_train(est.net, th_d, x_d, w_d)):
        assert torch.equal(a, b), name
    check_log_prob(oracle, theta, x, hip_log_prob(est.net, th_d, x_d)[0], "maf_envelope_rows", tag)
    samples, ld = hip_sample(est.net, noise.cuda(), x_d)
    check_sample(oracle, noise, x, samples, ld, "maf_envelope_rows", tag)


# ------------------------------------------------------------------------------------------ (f): hidden widths
@pytest.mark.parametrize("H", [3, 17, 48, 49, 52, 53, 63])
@pytest.mark.parametrize("variant", [0, 1])
def test_hidden_width_edges(variant, H):
    """Both sides of the KSH switch (13 K-steps for H in 49..52, 16 otherwise), widths that are no multiple of 4 and a
    width below one 16-tile: log_prob, sample and the training pass at 333 rows."""
    case = (variant, 5, 3, H, 8, 1)
    oracle, est, theta, x = pair(*case)
    n = 333
    assert waves(est.net, n) == 1
    theta, x, w, noise = theta[:n], x[:n], row_weights(n), noise_for(n, case[1])
    tag = f"{_id(case)} n{n}"
    th_d, x_d = theta.cuda().contiguous(), x.cuda().contiguous()
    logp, z = hip_log_prob(est.net, th_d, x_d)
    check_log_prob(oracle, theta, x, logp, "maf_envelope_hidden", tag)
    samples, ld = hip_sample(est.net, noise.cuda(), x_d)
    check_sample(oracle, noise, x, samples, ld, "maf_envelope_hidden", tag)
    assert (hip_log_prob(est.net, samples.cuda(), x_d)[1] - noise).abs().max() <= 2e-4
    got = hip_train(est.net, th_d, x_d, w.cuda())
    check_training(variant, est, got, oracle_training(variant, oracle, est, theta, x, w), "maf_envelope_hidden", tag,
                   small=True)


# ------------------------------------------------------------------------------------------ (g): refusals
# the header's nominal corner; one block past the one-wave configs of (b); D = 14, H = 50, K = 16, NB = 1
REFUSED = [(v, 16, 32, 64, 16, 4) for v in (0, 1)] + [(0, 16, 4, 64, 8, 3), (1, 16, 32, 64, 8, 3), (0, 14, 10, 50, 16, 1)]


@pytest.mark.parametrize("case", REFUSED, ids=_id)
def test_configs_past_the_lds_envelope_are_refused_without_a_launch(case):
    """E_LDS from the query and from all three entry points at every row count, outputs untouched (no launch), and the
    Python surface raises `_lib`'s E_LDS message.  (The largest fitting neighbours run, at one wave, in (b).)"""
    oracle, est, theta, x = pair(*case)
    net, D = est.net, case[1]
    for n in (1, 333, 8161, 32641):
        assert waves(net, n) == _lib.E_LDS
    n, fill = 333, 7.5
    th_d, x_d = theta[:n].cuda().contiguous(), x[:n].cuda().contiguous()
    for out in (hip_log_prob(net, th_d, x_d, fill=fill, check=False),
                hip_sample(net, noise_for(n, D).cuda(), x_d, fill=fill, check=False),
                hip_train(net, th_d, x_d, row_weights(n).cuda(), fill=fill, check=False)):
        assert out[0] == _lib.E_LDS
        for t in out[1:]:
            assert (t == fill).all()
    with pytest.raises(RuntimeError, match="more than 160 KiB of LDS"):
        net.plan_waves(n)
    with pytest.raises(RuntimeError, match="more than 160 KiB of LDS"):
        est.log_prob(th_d, x_d)
    with pytest.raises(RuntimeError, match="more than 160 KiB of LDS"):
        est.sample_from_noise(noise_for(n, D).cuda(), x_d)
    with pytest.raises(RuntimeError, match="more than 160 KiB of LDS"):
        est.loss(th_d, x_d).mean().backward()
    torch.cuda.synchronize()
