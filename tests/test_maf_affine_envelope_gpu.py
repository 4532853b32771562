"""GPU parity of the affine MAF kernels (csrc/maf_affine_kernel.h, host side csrc/maf_affine.hip) over what the host
code can launch, not only the one-wave launches of tests/test_maf_affine_gpu.py and its neighbours:

  (a) workgroup widths 2, 4, 8 at the thresholds of `aff_plan_for_rows`' halving loop (8161, 16321, 32641 rows), at
      eight waves also sbi's defaults (13 hidden K-steps), the envelope's corner and NB = 0, against fp64,
  (b) bit-identity of every per-row output of a wide launch with the same rows evaluated in one-wave launches,
  (c) the three condition-broadcast branches (x_rows == n, == 1, row % x_rows) and the refusal of grad_x with them,
  (d) the row edges of the training pass (wave tile, 128-row sub-chunk, 512-row chunk, the 4-way + tail reduction),
  (e) shape edges at one wave: H, D, C, NB and T one at a time from D5 C3 H32 NB1 T2,
  (f) the iid-trials kernel at widths 2, 4, 8 and at the widths 4, 5, 6, 7 the LDS limit forces on it, over the edges
      of its 8-trial blocks,
  (g) refusals through the query and all four launching entry points, before any launch.

Every test first asserts, through the host-only `sbi_amd_maf_affine_plan_waves`, the workgroup width it claims
(tests/test_maf_affine_envelope_cpu.py pins the same table without a device).  The kernels are called through the C
ABI on the packed image, every pointer from a live tensor of exactly the stated size, outputs and workspace
pre-filled with NaN.  T = 2 unless a case says otherwise.  The affine transform is smooth: no row is exempt from any
bar.  Tolerances are those of tests/test_maf_affine_gpu.py; for the parameter gradient of launches of more than 3000
rows, whose fp32 sums nobody had measured, the bar is max(2e-4, 2 x the eager fp32 oracle's own distance from fp64
on the same rows and weights) of the largest entry, both figures recorded per case.

Measured on the MI355X (profiles/parity_maf_affine_envelope.json): over the launches of 8161 .. 32641 rows the kernels'
parameter gradient is 0.7e-7 .. 1.6e-7 of the largest entry from fp64 and the fp32 oracle's 1.1e-7 .. 7.2e-7, so the
bar is 2e-4 in every case; grad_theta and grad_x stay below 6e-7 on every row of every case."""
import functools

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.maf_affine_flow import maf_affine_packed_weights
from tests import maf_affine_envelope as env
from tests.maf_affine_envelope import ONE_WAVE_ROWS, SMALL, cfg_id
from tests.parity_log import record
from tests.test_maf_affine_gpu import maf_pair, oracle_flat_grad

pytestmark = pytest.mark.gpu

NAN = float("nan")
KEY = "maf_affine_envelope_"


# ------------------------------------------------------------------------------------------------- pairs and calls
@functools.lru_cache(maxsize=None)
def pair(cfg, n_data=1000, perturb=0.05):
    """(oracle, HIP estimator, theta, x) on identical perturbed weights, built once per module."""
    D, C, H, NB, T = cfg
    return maf_pair(D=D, C=C, n=n_data, perturb=perturb, hidden_features=H, num_transforms=T, num_blocks=NB)


def waves(net, n, trials=False):
    return _lib.load().sbi_amd_maf_affine_plan_waves(net.hyper.c_config(), n, int(trials))


def _call(net, cfg_c, name, *args):
    dev = net.flat_params.device
    with torch.cuda.device(dev):
        return getattr(_lib.load(), name)(cfg_c if cfg_c is not None else net.hyper.c_config(), *args,
                                          _lib.current_stream(dev))


def _finish(rc, what, check, outs):
    if check:
        _lib.check(rc, what)
    torch.cuda.synchronize()
    outs = tuple(None if t is None else t.cpu() for t in outs)
    return outs if check else (rc,) + outs


def hip_log_prob(net, theta, x, fill=NAN, check=True, cfg_c=None):
    n, D = theta.shape
    logp, noise = torch.full((n,), fill, device="cuda"), torch.full((n, D), fill, device="cuda")
    rc = _call(net, cfg_c, "sbi_amd_maf_affine_log_prob", _lib.ptr(maf_affine_packed_weights(net)), _lib.ptr(net.zstats),
               _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(logp), _lib.ptr(noise))
    return _finish(rc, "maf_affine_log_prob", check, (logp, noise))


def hip_sample(net, noise, x, fill=NAN, check=True, cfg_c=None):
    n, D = noise.shape
    theta, ld = torch.full((n, D), fill, device="cuda"), torch.full((n,), fill, device="cuda")
    rc = _call(net, cfg_c, "sbi_amd_maf_affine_sample", _lib.ptr(maf_affine_packed_weights(net)), _lib.ptr(net.zstats),
               _lib.ptr(noise), _lib.ptr(x), n, x.shape[0], _lib.ptr(theta), _lib.ptr(ld))
    return _finish(rc, "maf_affine_sample", check, (theta, ld))


def hip_train(net, theta, x, w, uniform=0.0, want_gx=True, fill=NAN, check=True, cfg_c=None):
    """(losses, flat parameter gradient, grad_theta, grad_x) of sum_n w_n loss_n (`w` None: the uniform weight);
    everything the call writes starts as NaN.  grad_x always has the (n, C) the header states."""
    n, D = theta.shape
    loss, gth = torch.full((n,), fill, device="cuda"), torch.full((n, D), fill, device="cuda")
    gx = torch.full((n, net.hyper.C), fill, device="cuda") if want_gx else None
    grad = torch.full_like(net.flat_params.data, fill)
    ws = torch.full((net.train_workspace_floats(n),), NAN, device="cuda")
    rc = _call(net, cfg_c, "sbi_amd_maf_affine_loss_fwd_bwd", _lib.ptr(maf_affine_packed_weights(net)),
               _lib.ptr(net.zstats), _lib.ptr(theta), _lib.ptr(x), n, x.shape[0], _lib.ptr(w), float(uniform),
               _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(gth), _lib.ptr(gx), _lib.ptr(ws))
    return _finish(rc, "maf_affine_loss_fwd_bwd", check, (loss, grad, gth, gx))


def hip_trials(net, x_trials, theta, fill=NAN, check=True, cfg_c=None):
    """out[c] = sum_i log q(x_trials[i] | theta[c]): x_trials (num_trials, D) flow inputs, theta (num_theta, C)."""
    out = torch.full((theta.shape[0],), fill, device="cuda")
    rc = _call(net, cfg_c, "sbi_amd_maf_affine_log_prob_trials", _lib.ptr(maf_affine_packed_weights(net)),
               _lib.ptr(net.zstats), _lib.ptr(x_trials), x_trials.shape[0], _lib.ptr(theta), theta.shape[0],
               _lib.ptr(out))
    return _finish(rc, "maf_affine_log_prob_trials", check, (out,))


def row_weights(n):
    return torch.linspace(0.5, 1.5, n) / n


def noise_for(n, D):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(5))


def dev(*tensors):
    return tuple(t.cuda().contiguous() for t in tensors)


# ------------------------------------------------------------------------------------------------- references
def oracle_training(oracle, est, theta, x, w, dtype=torch.float64, chunk=8192):
    """Autograd of sum_n w_n loss_n in `dtype`: (losses, flat parameter gradient with the masks applied, d / d theta,
    d / d x), returned as fp64.  The oracle comes back in fp32."""
    n = theta.shape[0]
    oracle.to(dtype).zero_grad()
    th = theta.to(dtype).clone().requires_grad_(True)
    xx = x.to(dtype).clone().requires_grad_(True)
    ww = w.to(dtype)
    losses = []
    for i in range(0, n, chunk):
        l = oracle.loss(th[i : i + chunk], xx[i : i + chunk])
        (l * ww[i : i + chunk]).sum().backward()
        losses.append(l.detach())
    gref = oracle_flat_grad(oracle, est, dtype).double()
    oracle.zero_grad()
    oracle.float()
    return torch.cat(losses).double(), gref, th.grad.double(), xx.grad.double()


def check_log_prob(oracle, theta, x, got, got_z, key, tag):
    with torch.no_grad():
        ref, ref_z = oracle.log_prob(theta, x)[0], oracle.inverse_transform(theta, x)
        ref64 = oracle.double().log_prob(theta.double(), x.double())[0]
        ref_z64 = oracle.inverse_transform(theta.double(), x.double())
        oracle.float()
    assert torch.isfinite(got).all() and torch.isfinite(got_z).all()
    e_hip, e_ref = (got.double() - ref64).abs().max().item(), (ref.double() - ref64).abs().max().item()
    z_hip, z_ref = (got_z.double() - ref_z64).abs().max().item(), (ref_z.double() - ref_z64).abs().max().item()
    d32, z32 = (got - ref).abs().max().item(), (got_z - ref_z).abs().max().item()
    record(KEY + key + "_log_prob", tag, max_abs_hip_vs_oracle32=d32, max_abs_hip_vs_f64=e_hip,
           max_abs_oracle32_vs_f64=e_ref, max_abs_ref=ref.abs().max().item(), noise_max_abs_hip_vs_oracle32=z32,
           noise_max_abs_hip_vs_f64=z_hip, noise_max_abs_oracle32_vs_f64=z_ref, noise_max_abs_ref=ref_z.abs().max().item())
    print(f"{tag} log_prob: |hip-o32|={d32:.3e} |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} max|ref|={ref.abs().max():.1f}"
          f" noise |hip-o32|={z32:.3e} |hip-f64|={z_hip:.3e} |o32-f64|={z_ref:.3e} max|ref|={ref_z.abs().max():.1f}")
    assert d32 <= 1e-5 + 1e-5 * ref.abs().max().item()                  # in-distribution rows
    assert z32 <= 1e-5 + 1e-5 * ref_z.abs().max().item()
    assert e_hip <= 2.0 * e_ref + 1e-5
    assert z_hip <= 2.0 * z_ref + 1e-5


def check_sample(oracle, noise, x, got, got_ld, key, tag):
    with torch.no_grad():
        ref, ref_ld = oracle.sample_from_noise(noise, x)
        ref64, ref_ld64 = oracle.double().sample_from_noise(noise.double(), x.double())
        oracle.float()
    assert torch.isfinite(got).all() and torch.isfinite(got_ld).all()
    e_hip, e_ref = (got.double() - ref64).abs().max().item(), (ref.double() - ref64).abs().max().item()
    l_hip, l_ref = (got_ld.double() - ref_ld64).abs().max().item(), (ref_ld.double() - ref_ld64).abs().max().item()
    d32, l32 = (got - ref).abs().max().item(), (got_ld - ref_ld).abs().max().item()
    record(KEY + key + "_sample", tag, max_abs_hip_vs_oracle32=d32, max_abs_hip_vs_f64=e_hip, max_abs_oracle32_vs_f64=e_ref,
           max_abs_ref=ref.abs().max().item(), max_abs_logabsdet_hip_vs_oracle32=l32, max_abs_logabsdet_hip_vs_f64=l_hip,
           max_abs_logabsdet_oracle32_vs_f64=l_ref, max_abs_logabsdet_ref=ref_ld.abs().max().item())
    print(f"{tag} sample: |hip-o32|={d32:.3e} |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} max|ref|={ref.abs().max():.1f} "
          f"logabsdet |hip-o32|={l32:.3e} |hip-f64|={l_hip:.3e} |o32-f64|={l_ref:.3e} max|ref|={ref_ld.abs().max():.1f}")
    assert d32 <= 1e-5 + 1e-5 * ref.abs().max().item()                  # in-distribution rows
    assert l32 <= 1e-5 + 1e-5 * ref_ld.abs().max().item()
    assert e_hip <= 2.0 * e_ref + 1e-5
    assert l_hip <= 2.0 * l_ref + 2e-5


def check_masked_zero(est, got):
    h = est.net.hyper
    for (key, off, cnt, shape), (_, _, kind) in zip(est.net._slices(), h.layer_entries() * h.num_transforms):
        if kind in (0, 2, 3):
            assert (got[off : off + cnt].reshape(shape)[h.mask(kind) == 0] == 0).all(), key


def check_training(oracle, est, got, theta, x, w, key, tag, grad_only=False):
    """`got`: (losses, flat gradient, grad_theta, grad_x | None) of the kernels for these rows and weights.  Losses,
    grad_theta and grad_x are held to their bars on EVERY row; the parameter gradient to 2e-4 overall and 3e-4 per
    block up to 3000 rows, beyond that to max(2e-4, 2 x the fp32 oracle's own distance from fp64).
    `grad_only`: the rows are not in-distribution pairs, only the parameter gradient has a bar."""
    n = theta.shape[0]
    losses, grad, gth, gx = got
    loss_ref, gref, gth_ref, gx_ref = oracle_training(oracle, est, theta, x, w)
    grad = grad.double()
    for t in got:
        assert t is None or torch.isfinite(t).all()
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
    e_x = -1.0 if gx is None else (gx.double() - gx_ref).abs().max().item() / gx_ref.abs().max().item()
    numbers = dict(rows=n, max_abs_loss_err_vs_f64=e_l, max_abs_loss=loss_ref.abs().max().item(), rel_grad_err_vs_f64=rel,
                   worst_block_rel_err=worst, rel_grad_theta_err=e_th, rel_grad_x_err=e_x)
    rel32 = None
    if n > 3000:
        g32 = oracle_training(oracle, est, theta, x, w, dtype=torch.float32)[1]
        rel32 = (g32 - gref).abs().max().item() / scale
        numbers.update(rel_grad_err_oracle32_vs_f64=rel32, rel_grad_bar=max(2e-4, 2.0 * rel32))
    record(KEY + key + "_train", tag, **numbers)
    print(f"{tag} train: loss err {e_l:.3e} (max {loss_ref.abs().max():.1f}) grad rel {rel:.3e} (fp32 oracle: {rel32}) "
          f"worst block {worst:.3e} ({worst_key}) d/dtheta rel {e_th:.3e} d/dx rel {e_x:.3e}")
    if not grad_only:
        assert e_l <= 1e-5 + 1e-5 * loss_ref.abs().max().item()
        assert e_th <= 3e-4 and e_x <= 3e-4
    if n <= 3000:
        assert worst <= 3e-4, f"{worst_key}: {worst:.3e}"
        assert rel <= 2e-4
    else:
        assert rel <= max(2e-4, 2.0 * rel32)
    check_masked_zero(est, grad)


# ------------------------------------------------------------------------------------------ (a), (b): wide launches
WIDE_IDS = [f"{cfg_id(c)}-n{n}-w{nw}" for c, n, nw in env.WIDE]


@functools.lru_cache(maxsize=None)
def wide_run(cfg, n):
    """Every per-row output and the parameter gradient of ONE launch each over all n rows."""
    oracle, est, theta, x = pair(cfg, n_data=n)
    noise, w = noise_for(n, cfg[0]), row_weights(n)
    th_d, x_d = dev(theta, x)
    logp, z = hip_log_prob(est.net, th_d, x_d)
    samples, ld = hip_sample(est.net, noise.cuda(), x_d)
    back = hip_log_prob(est.net, samples.cuda(), x_d)[1]
    losses, grad, gth, gx = hip_train(est.net, th_d, x_d, w.cuda())
    return dict(noise=noise, w=w, logp=logp, z=z, samples=samples, ld=ld, back=back, losses=losses, grad=grad, gth=gth,
                gx=gx)


def boundary_rows(n, nw):
    """First and last 512 rows plus the 32 rows straddling two workgroup boundaries (a workgroup owns 16 nw rows)."""
    wg = 16 * nw
    groups = (n + wg - 1) // wg
    parts = [torch.arange(0, 512), torch.arange(n - 512, n)]
    parts += [torch.arange(b - 16, b + 16) for b in (wg * (groups // 3), wg * (2 * groups // 3))]
    return torch.unique(torch.cat(parts))


@pytest.mark.parametrize("cfg,n,nw", env.WIDE, ids=WIDE_IDS)
def test_wide_launch_matches_the_fp64_oracle(cfg, n, nw):
    """log_prob + noise, sample + logabsdet, the device round trip and the training pass (row weights, grad_theta,
    grad_x) at the stated workgroup width.  log-probs, noise, samples and logabsdet are compared on `boundary_rows`
    (test_wide_launch_is_bit_identical_to_one_wave_launches licenses the subsample); the losses, grad_theta and grad_x
    on every row, the parameter gradient, a sum over all rows, in full."""
    oracle, est, theta, x = pair(cfg, n_data=n)
    assert waves(est.net, n) == nw
    run = wide_run(cfg, n)
    idx, tag = boundary_rows(n, nw), f"{cfg_id(cfg)} n{n} w{nw}"
    for k in ("logp", "z", "samples", "ld", "back", "losses", "gth", "gx", "grad"):
        assert torch.isfinite(run[k]).all(), k
    check_log_prob(oracle, theta[idx], x[idx], run["logp"][idx], run["z"][idx], "wide", tag)
    check_sample(oracle, run["noise"][idx], x[idx], run["samples"][idx], run["ld"][idx], "wide", tag)
    e_rt = (run["back"] - run["noise"]).abs().max().item()
    record(KEY + "wide_round_trip", tag, max_abs_round_trip=e_rt)
    assert e_rt <= 2e-4                                                   # round trip on the device, every row
    check_training(oracle, est, (run["losses"], run["grad"], run["gth"], run["gx"]), theta, x, run["w"], "wide", tag)


@pytest.mark.parametrize("cfg,n,nw", env.WIDE, ids=WIDE_IDS)
def test_wide_launch_is_bit_identical_to_one_wave_launches(cfg, n, nw):
    """One wave owns 16 rows and its own scratch whatever the workgroup width: log-probs, noise, samples, logabsdet,
    per-row losses, grad_theta and grad_x of the wide launch equal, bit for bit, the same rows evaluated in launches
    of <= 8160 rows (one wave per workgroup) with the same per-row weights."""
    oracle, est, theta, x = pair(cfg, n_data=n)
    assert waves(est.net, n) == nw
    run = wide_run(cfg, n)
    for s in range(0, n, ONE_WAVE_ROWS):
        e = min(n, s + ONE_WAVE_ROWS)
        assert waves(est.net, e - s) == 1
        th_d, x_d, noise_d, w_d = dev(theta[s:e], x[s:e], run["noise"][s:e], run["w"][s:e])
        logp, z = hip_log_prob(est.net, th_d, x_d)
        samples, ld = hip_sample(est.net, noise_d, x_d)
        losses, _, gth, gx = hip_train(est.net, th_d, x_d, w_d)
        for name, got in (("logp", logp), ("z", z), ("samples", samples), ("ld", ld), ("losses", losses), ("gth", gth),
                          ("gx", gx)):
            assert torch.isfinite(got).all() and torch.equal(run[name][s:e], got), f"{name} rows {s}..{e}"


# ------------------------------------------------------------------------------------------ (c): condition broadcast
@pytest.mark.parametrize("n,x_rows", [(333, 1), (333, 7), (8161, 100), (8161, 1)], ids=lambda v: str(v))
def test_condition_broadcast_equals_the_expanded_condition(n, x_rows):
    """x_rows == 1 and row % x_rows (n % x_rows != 0) against x_rows == n on x[i % x_rows]: bit-identical log_prob,
    noise, samples, logabsdet, losses, grad_theta and parameter gradient; the latter also against fp64 autograd on the
    expanded x.  The short condition is the head of an n-row buffer of OTHER rows, so an index that ignores x_rows
    reads defined, different data.  grad_x needs one condition row per theta row: with a short condition the call
    answers E_BADARG and writes neither grad_x nor the parameter gradient."""
    oracle, est, theta, x = pair(SMALL, n_data=max(n, 1000))
    assert waves(est.net, n) == (2 if n == 8161 else 1)
    theta, x_buf = dev(theta[:n], x[:n].flip(0))
    x_short = x_buf[:x_rows]
    x_exp = x_short[torch.arange(n, device="cuda") % x_rows].contiguous()
    assert not torch.equal(x_exp, x_buf)
    noise, w = dev(noise_for(n, SMALL[0]), row_weights(n))
    for name, a, b in zip(("logp", "noise"), hip_log_prob(est.net, theta, x_short), hip_log_prob(est.net, theta, x_exp)):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    for name, a, b in zip(("samples", "logabsdet"), hip_sample(est.net, noise, x_short), hip_sample(est.net, noise, x_exp)):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    got = hip_train(est.net, theta, x_short, w, want_gx=False)
    exp = hip_train(est.net, theta, x_exp, w)
    for name, a, b in zip(("losses", "grad", "grad_theta"), got, exp):
        assert torch.isfinite(b).all() and torch.equal(a, b), name
    check_training(oracle, est, got, theta.cpu(), x_exp.cpu(), w.cpu(), "broadcast", f"{cfg_id(SMALL)} n{n} x_rows{x_rows}",
                   grad_only=True)
    # grad_x with a short condition: refused before any launch
    n_c, fill = SMALL[1], 7.5
    loss, gth, gx = (torch.full(s, fill, device="cuda") for s in ((n,), (n, SMALL[0]), (n, n_c)))
    grad = torch.full_like(est.net.flat_params.data, fill)
    ws = torch.full((est.net.train_workspace_floats(n),), fill, device="cuda")
    rc = _call(est.net, None, "sbi_amd_maf_affine_loss_fwd_bwd", _lib.ptr(maf_affine_packed_weights(est.net)),
               _lib.ptr(est.net.zstats), _lib.ptr(theta), _lib.ptr(x_short), n, x_rows, _lib.ptr(w), 0.0, _lib.ptr(loss),
               _lib.ptr(grad), _lib.ptr(gth), _lib.ptr(gx), _lib.ptr(ws))
    torch.cuda.synchronize()
    assert rc == _lib.E_BADARG
    for name, t in (("loss", loss), ("grad", grad), ("grad_theta", gth), ("grad_x", gx), ("workspace", ws)):
        assert (t == fill).all(), name


# ------------------------------------------------------------------------------------------ (d): row edges
ROW_EDGES = [1, 15, 16, 17, 127, 128, 129, 511, 512, 513, 3000]      # 3000 rows: six chunks, 4-way loop + tail of two


@pytest.mark.parametrize("n", ROW_EDGES)
def test_row_edges_of_the_training_pass(n):
    """Wave-tile, sub-chunk (128) and chunk (512) boundaries +-1 row, one row, and a chunk count that runs both loops of
    the reduction: losses, the full parameter gradient, grad_theta and grad_x against fp64 autograd, masked entries
    exactly zero, two calls bit-identical, the uniform weight bit-identical to the same weight per row; log_prob and
    sample at the same row counts."""
    oracle, est, theta, x = pair(SMALL, n_data=3000)
    assert waves(est.net, n) == 1
    theta, x, w, noise = theta[:n], x[:n], row_weights(n), noise_for(n, SMALL[0])
    tag = f"{cfg_id(SMALL)} n{n}"
    th_d, x_d, w_d = dev(theta, x, w)
    got = hip_train(est.net, th_d, x_d, w_d)
    check_training(oracle, est, got, theta, x, w, "rows", tag)
    for name, a, b in zip(("losses", "grad", "grad_theta", "grad_x"), got, hip_train(est.net, th_d, x_d, w_d)):
        assert torch.equal(a, b), name
    uni = hip_train(est.net, th_d, x_d, None, uniform=1.0 / n)
    per_row = hip_train(est.net, th_d, x_d, torch.full((n,), 1.0 / n, device="cuda"))
    for name, a, b in zip(("losses", "grad", "grad_theta", "grad_x"), uni, per_row):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    check_log_prob(oracle, theta, x, *hip_log_prob(est.net, th_d, x_d), "rows", tag)
    samples, ld = hip_sample(est.net, noise.cuda(), x_d)
    check_sample(oracle, noise, x, samples, ld, "rows", tag)


# ------------------------------------------------------------------------------------------ (e): shape edges
# One dimension at a time from the small config.  H: both sides of the KSH switch (13 K-steps for 49..52), remainders of
# 4, below one 16-tile, the full width.  D: the register boundaries of the (u, s) fragments (4 r + g) and an empty
# initial mask (1).  C: both sides of 16 (4 / 8 context K-steps, the two m-tiles of the grad_x write-out).  T = 1:
# is_last and t == 0 in one backward launch; T = 16: the gz ping-pong, eight times round.
_D, _C, _H, _NB, _T = SMALL
SHAPES = [(_D, _C, H, _NB, _T) for H in (3, 17, 48, 49, 52, 53, 63, 64)]
SHAPES += [(D, _C, _H, _NB, _T) for D in (1, 4, 5, 13, 15, 16)]
SHAPES += [(_D, C, _H, _NB, _T) for C in (1, 15, 16, 17, 31, 32)]
SHAPES += [(_D, _C, _H, NB, _T) for NB in (0, 4)] + [(_D, _C, _H, _NB, T) for T in (1, 16)]


@pytest.mark.parametrize("cfg", SHAPES, ids=cfg_id)
def test_shape_edges_at_one_wave(cfg):
    """log_prob, sample, the device round trip and the training pass with grad_theta and grad_x at 333 rows.  T = 16
    runs on the oracle's default perturbation (0.05), which was not lowered: its log-probs stay in the in-distribution
    regime there (max |log p| 28.9, the fp32 oracle 6.4e-6 from fp64).  Sixteen perturbed transforms do amplify the
    sampling direction (samples up to 875, the fp32 oracle 4.6e-4 from fp64); its bars scale with the oracle's own
    error and the largest sample, and the device round trip still returns the noise to 2e-4."""
    oracle, est, theta, x = pair(cfg)
    n = 333
    assert waves(est.net, n) == 1
    theta, x, w, noise = theta[:n], x[:n], row_weights(n), noise_for(n, cfg[0])
    tag = f"{cfg_id(cfg)} n{n}"
    th_d, x_d = dev(theta, x)
    check_log_prob(oracle, theta, x, *hip_log_prob(est.net, th_d, x_d), "shape", tag)
    samples, ld = hip_sample(est.net, noise.cuda(), x_d)
    check_sample(oracle, noise, x, samples, ld, "shape", tag)
    e_rt = (hip_log_prob(est.net, samples.cuda(), x_d)[1] - noise).abs().max().item()
    record(KEY + "shape_round_trip", tag, max_abs_round_trip=e_rt)
    assert e_rt <= 2e-4
    check_training(oracle, est, hip_train(est.net, th_d, x_d, w.cuda()), theta, x, w, "shape", tag)


# ------------------------------------------------------------------------------------------ (f): trials kernel
# (config, thetas, waves, numbers of trials): the full trial grid (one trial, a block less one, a block, a block and a
# tail of one, two blocks, two blocks and one) at two waves; elsewhere one full block and a tail of one
TRIALS = [(c, n, nw, (1, 7, 8, 9, 16, 17) if n == 8161 else (9,)) for c, n, nw in env.TRIALS_WIDE + env.TRIALS_FORCED]
TRIALS = [(c, n, nw, k) for c, n, nw, ks in TRIALS for k in ks]


@functools.lru_cache(maxsize=None)
def trial_inputs(cfg, n):
    """17 trials (the flow's inputs) and n thetas (its condition), drawn as in tests/test_maf_affine_gpu.py."""
    g = torch.Generator().manual_seed(17000 + n)
    return torch.randn(17, cfg[0], generator=g) * 0.4, torch.randn(n, cfg[1], generator=g) * 0.5


@functools.lru_cache(maxsize=None)
def paired_terms(cfg, n):
    """log q(x_i | theta_c) for the trials a case of TRIALS uses (all 17 at 8161 thetas, the first 9 elsewhere) and n
    thetas from the PAIRED kernel in launches of <= 8160 rows (one wave): (trials, n)."""
    _, est, _, _ = pair(cfg)
    x_trials, theta = trial_inputs(cfg, n)
    k = max(k for c, m, _, k in TRIALS if (c, m) == (cfg, n))
    out = torch.empty(k, n)
    for s in range(0, n, ONE_WAVE_ROWS):
        e = min(n, s + ONE_WAVE_ROWS)
        assert waves(est.net, e - s) == 1
        th_d = theta[s:e].cuda().contiguous()
        for i in range(k):
            out[i, s:e] = hip_log_prob(est.net, x_trials[i : i + 1].expand(e - s, -1).cuda().contiguous(), th_d)[0]
    return out


@pytest.mark.parametrize("cfg,n,nw,num_trials", TRIALS, ids=[f"{cfg_id(c)}-n{n}-w{nw}-trials{k}" for c, n, nw, k in TRIALS])
def test_trials_kernel_is_the_paired_kernel_summed_in_trial_order(cfg, n, nw, num_trials):
    """The contract of the header at every workgroup width the trials kernel can take: bit-identical to the paired
    kernel's per-trial log-probs added in trial order in fp32.  On `boundary_rows` also against the fp64 oracle, to
    num_trials x the bars of a single log-prob."""
    oracle, est, _, _ = pair(cfg)
    assert waves(est.net, n, trials=True) == nw
    x_trials, theta = trial_inputs(cfg, n)
    x_trials = x_trials[:num_trials]
    got = hip_trials(est.net, *dev(x_trials, theta))[0]
    terms = paired_terms(cfg, n)
    want = terms[0].clone()
    for i in range(1, num_trials):
        want = want + terms[i]
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    idx = boundary_rows(n, nw)
    th = theta[idx]
    sum32, sum64 = torch.zeros(idx.numel()), torch.zeros(idx.numel(), dtype=torch.float64)
    e_term, max_term = 0.0, 0.0
    with torch.no_grad():
        for i in range(num_trials):
            xi = x_trials[i : i + 1].expand(idx.numel(), -1)
            r32 = oracle.log_prob(xi, th)[0]
            r64 = oracle.double().log_prob(xi.double(), th.double())[0]
            oracle.float()
            sum32, sum64 = sum32 + r32, sum64 + r64
            e_term, max_term = max(e_term, (r32.double() - r64).abs().max().item()), max(max_term, r32.abs().max().item())
    e_hip, d32 = (got[idx].double() - sum64).abs().max().item(), (got[idx] - sum32).abs().max().item()
    tag = f"{cfg_id(cfg)} n{n} w{nw} trials{num_trials}"
    record(KEY + "trials", tag, max_abs_hip_vs_f64=e_hip, max_abs_hip_vs_oracle32=d32, max_abs_term_oracle32_vs_f64=e_term,
           max_abs_term=max_term)
    print(f"{tag}: |hip-f64|={e_hip:.3e} |hip-o32|={d32:.3e} per term |o32-f64|={e_term:.3e} max|term|={max_term:.1f}")
    assert e_hip <= num_trials * (2.0 * e_term + 1e-5)
    assert d32 <= num_trials * (1e-5 + 1e-5 * max_term)                   # every term is in-distribution


# ------------------------------------------------------------------------------------------ (g): refusals
# (field, refused value, nearest valid value, code)
REFUSED = [("D", 17, 16, _lib.E_UNSUPPORTED), ("C", 33, 32, _lib.E_UNSUPPORTED), ("H", 65, 64, _lib.E_UNSUPPORTED),
           ("T", 17, 16, _lib.E_UNSUPPORTED), ("NB", 5, 4, _lib.E_UNSUPPORTED), ("D", 0, 1, _lib.E_BADARG),
           ("epsilon", -1e-3, 1e-3, _lib.E_BADARG), ("epsilon", NAN, 1e-3, _lib.E_BADARG)]


@pytest.mark.parametrize("field,bad,near,code", REFUSED, ids=[f"{f}={b}" for f, b, _, _ in REFUSED])
def test_configs_outside_the_envelope_are_refused_without_a_launch(field, bad, near, code):
    """The query and log_prob, sample, loss_fwd_bwd and log_prob_trials answer the code for a config built directly as
    the C struct, and leave outputs pre-filled with 7.5 as they were.  Every buffer (and the packed image) is sized
    for the nearest valid config, so nothing here could launch out of bounds."""
    fields = dict(zip(("D", "C", "H", "NB", "T"), SMALL))
    if field != "epsilon":
        fields[field] = near
    valid = tuple(fields[k] for k in ("D", "C", "H", "NB", "T"))
    oracle, est, theta, x = pair(valid)
    net = est.net
    fields["epsilon"] = 1e-3
    fields[field] = bad
    cfg_c = _lib.MAFAffineConfigC(fields["D"], fields["C"], fields["H"], fields["T"], fields["NB"], fields["epsilon"])
    lib = _lib.load()
    n, fill = 333, 7.5
    for rows in (1, n, 8161, 32641):
        for trials in (0, 1):
            assert lib.sbi_amd_maf_affine_plan_waves(cfg_c, rows, trials) == code
    assert waves(net, n) == 1 and waves(net, n, trials=True) == 1
    th_d, x_d = dev(theta[:n], x[:n])
    for out in (hip_log_prob(net, th_d, x_d, fill=fill, check=False, cfg_c=cfg_c),
                hip_sample(net, noise_for(n, valid[0]).cuda(), x_d, fill=fill, check=False, cfg_c=cfg_c),
                hip_train(net, th_d, x_d, row_weights(n).cuda(), fill=fill, check=False, cfg_c=cfg_c),
                hip_trials(net, th_d[:9].contiguous(), x_d, fill=fill, check=False, cfg_c=cfg_c)):
        assert out[0] == code
        for t in out[1:]:
            assert (t == fill).all()
