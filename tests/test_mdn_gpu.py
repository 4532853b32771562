"""GPU parity of the mixture-density-network kernels (csrc/mdn_kernel.h) through the C ABI against the eager
restatement (tests/mdn_oracle.py) on identical weights and inputs, and against recorded outputs of the real sbi
classes (tests/golden/mdn_reference.pt): mixture components, log_prob, loss, sample, the fused training pass, the
one-observation kernels, the autograd bridge and the fused step, end-to-end NPE, the ABI's refusals.
Tolerances as for the maf_rqs path (tests/test_maf_gpu.py): 1e-5 norm-wise and "no further from fp64 than the fp32
restatement is (x2)"; gradients 2e-4 of their max norm, 3e-4 per parameter block and for d loss / d theta."""
import copy
import functools
import os
import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.mdn import (mdn_components_call, mdn_log_prob_call, mdn_loss_fwd_bwd,
                                                mdn_packed_weights, mdn_sample_call)
from sbi_amd.neural_nets.net_builders.mdn import build_mdn
from tests.mdn_envelope import errs as _errs
from tests.mdn_envelope import mdn_pair_gpu
from tests.mdn_envelope import packed_factors as _packed_factors
from tests.parity_log import record

pytestmark = pytest.mark.gpu

# (D, C, H, K): defaults (H padded) | no upper head | one component | envelope corner | mid-size
CONFIGS = [(10, 10, 50, 10), (1, 3, 50, 10), (2, 2, 8, 1), (16, 12, 64, 16), (3, 5, 32, 4)]
ROWS = [333, 1, 17]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mdn_reference.pt")


def _id(c):
    return "D%d-C%d-H%d-K%d" % c


def mdn_pair(D, C, H, K):
    """(fp32 restatement, fp64 restatement, HIP estimator, theta, x): identical perturbed weights and z-scoring
    (built once in tests/mdn_envelope.py and shared with the envelope tests)."""
    return mdn_pair_gpu(D, C, H, K)


@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_components_log_prob_loss_and_sample_match_the_restatement(cfg, n, one_x):
    o32, o64, est, theta_d, x_d = mdn_pair(*cfg)
    D, C, H, K = cfg
    net = est.net
    x = x_d[:1] if one_x else x_d[:n]
    tag = f"{_id(cfg)} n{n} {'one_x' if one_x else 'paired'}"
    # -- components (the condition rows only)
    with torch.no_grad():
        lg32, mu32, A32 = o32.components(x)
        lg64, mu64, A64 = o64.components(x.double())
    lg, mu, fac = mdn_components_call(net, x.cuda())
    rec = {}
    for name, got, r32, r64 in (("logits", lg, lg32, lg64), ("means", mu, mu32, mu64),
                                ("factors", fac, _packed_factors(A32, D), _packed_factors(A64, D))):
        e_hip, e_ref = _errs(got, r32, r64)
        rec[name + "_hip_vs_f64"], rec[name + "_o32_vs_f64"] = e_hip, e_ref
        print(f"{name}: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
        assert torch.isfinite(got).all() and e_hip <= 2.0 * e_ref + 1e-5, name
    # -- log_prob / loss: in-distribution rows and 3-sigma stress rows
    for what, theta in (("in-distribution", theta_d[:n]), ("stress", 3.0 * theta_d[1000 - n:])):
        with torch.no_grad():
            ref = o32.log_prob(theta[:, None], x)[:, 0] if one_x else o32.log_prob(theta, x)
            ref64 = (o64.log_prob(theta.double()[:, None], x.double())[:, 0] if one_x
                     else o64.log_prob(theta.double(), x.double()))
        got = mdn_log_prob_call(net, theta.cuda().contiguous(), x.cuda()).cpu()
        e_hip, e_ref = _errs(got, ref, ref64)
        rec[what + "_hip_vs_o32"] = (got - ref).abs().max().item()
        rec[what + "_hip_vs_f64"], rec[what + "_o32_vs_f64"] = e_hip, e_ref
        rec[what + "_max_abs_ref"] = ref.abs().max().item()
        print(f"{what}: |hip-o32|={(got - ref).abs().max():.3e} |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} "
              f"max|ref|={ref.abs().max():.1f}")
        assert torch.isfinite(got).all()
        if what == "in-distribution":
            assert (got - ref).abs().max() <= 1e-5 + 1e-5 * ref.abs().max()
            if not one_x:       # loss = -log_prob through the estimator surface, (B,) without a sample dimension
                loss = est.loss(theta.cuda(), x.cuda()).cpu()
                assert loss.shape == (n,) and torch.equal(loss, -got)
        assert e_hip <= 2.0 * e_ref + 1e-5
    # -- sample for GIVEN components and normal draws
    g = torch.Generator().manual_seed(5 + n)
    comp = torch.randint(0, K, (n,), generator=g)
    zeta = torch.randn(n, D, generator=g)
    with torch.no_grad():
        ref = o32.sample_given(comp, zeta, x)
        ref64 = o64.sample_given(comp, zeta.double(), x.double())
    got = mdn_sample_call(net, zeta.cuda(), x.cuda(), comp=comp.to(torch.int32).cuda())
    e_hip, e_ref = _errs(got, ref, ref64)
    rec["sample_hip_vs_f64"], rec["sample_o32_vs_f64"] = e_hip, e_ref
    print(f"sample: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
    record("mdn_parity", tag, **rec)
    assert torch.isfinite(got).all() and e_hip <= 2.0 * e_ref + 1e-5


@pytest.mark.parametrize("case", ["d3", "d1"])
def test_matches_the_recorded_outputs_of_the_reference_classes(case):
    """Real MultivariateGaussianMDN / MixtureDensityEstimator / MoG outputs (tools/make_golden_mdn.py)."""
    c = torch.load(GOLDEN)[case]
    D, B = c["D"], c["theta"].shape[0]
    est = build_mdn(c["theta"], c["x"], hidden_features=c["H"], num_components=c["K"])
    est.load_state_dict(c["state_dict"], strict=True)
    est = est.cuda()

    def close(got, ref, what):
        err = (got.cpu() - ref).abs().max().item()
        record("mdn_golden", f"{case} {what}", max_abs_err=err, max_abs_ref=ref.abs().max().item())
        print(f"{what}: {err:.3e} (max |ref| {ref.abs().max():.2f})")
        assert err <= 1e-5 + 1e-5 * ref.abs().max().item(), what

    mog = est.get_uncorrected_mog(c["x"].cuda())
    close(mog.logits, c["logits"], "logits")
    close(mog.means, c["means"], "means")
    close(mog.precision_factors, c["precision_factors"], "precision_factors")
    close(mog.precisions, c["precisions"], "precisions")
    lp = est.log_prob(c["theta"].cuda(), c["x"].cuda())
    assert lp.shape == (B,)
    close(lp, c["log_prob"], "log_prob")
    lps = est.log_prob(c["theta_s"].cuda(), c["x"].cuda())
    assert lps.shape == (5, B)
    close(lps, c["log_prob_s"], "log_prob with a sample dimension")
    close(est.loss(c["theta"].cuda(), c["x"].cuda()), c["loss"], "loss")
    # sample: the reference drew choices (B, 7) and z (B, 7, D, 1) and returned (7, B, D); rows sample-major here
    comp = c["choices"].t().reshape(-1)
    zeta = c["z"][..., 0].transpose(0, 1).reshape(-1, D).contiguous()
    got = est.sample_given(zeta.cuda(), c["x"].cuda(), comp=comp.cuda()).reshape(7, B, D)
    close(got, c["samples"], "sample")
    # parameter gradient of the mean loss through the autograd bridge
    est.zero_grad()
    est.loss(c["theta"].cuda(), c["x"].cuda()).mean().backward()
    got = est.net.flat_params.grad.cpu()
    ref = torch.cat([c["grad"]["net." + key].reshape(-1) for key, _, _, _ in est.net._slices()])
    rel = (got - ref).abs().max().item() / ref.abs().max().item()
    record("mdn_golden", f"{case} grad", rel_grad_err=rel)
    assert rel <= 2e-4


@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_sample_picks_the_component_by_the_cumulative_weights(cfg, one_x):
    o32, o64, est, theta_d, x_d = mdn_pair(*cfg)
    D, C, H, K = cfg
    n = 1000
    x = x_d[:1] if one_x else x_d[:n]
    g = torch.Generator().manual_seed(11)
    u = torch.rand(n, generator=g)
    zeta = torch.randn(n, D, generator=g)
    with torch.no_grad():
        cum64 = o64.cumulative_weights(x.double()).expand(n, K)
        comp = torch.searchsorted(cum64.contiguous(), u.double()[:, None], right=True)[:, 0].clamp(max=K - 1)
        keep = ((cum64 - u.double()[:, None]).abs() > 1e-5).all(1)      # rows that sit on a boundary are left out
        ref = o32.sample_given(comp, zeta, x)
        ref64 = o64.sample_given(comp, zeta.double(), x.double())
    left_out = int((~keep).sum())
    assert left_out <= n // 100
    got = mdn_sample_call(est.net, zeta.cuda(), x.cuda(), u=u.cuda())
    e_hip, e_ref = _errs(got[keep.cuda()], ref[keep], ref64[keep])
    record("mdn_sample_u", f"{_id(cfg)} {'one_x' if one_x else 'paired'}", left_out=left_out, hip_vs_f64=e_hip,
           o32_vs_f64=e_ref)
    print(f"left out {left_out}; |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
    assert e_hip <= 2.0 * e_ref + 1e-5


@pytest.mark.parametrize("one_x", [False, True], ids=["paired", "one_x"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_training_pass_matches_fp64_autograd_and_is_deterministic(cfg, n, one_x):
    o32, o64, est, theta_d, x_d = mdn_pair(*cfg)
    D = cfg[0]
    net = est.net
    theta, x = theta_d[:n].contiguous(), (x_d[:1] if one_x else x_d[:n])
    w = torch.linspace(0.5, 1.5, n) / n if n > 1 else torch.ones(1)
    o64.zero_grad()
    th = theta.double().clone().requires_grad_(True)
    loss_ref = o64.loss(th[:, None], x.double())[:, 0] if one_x else o64.loss(th, x.double())
    (loss_ref * w.double()).sum().backward()
    gref, gth_ref = o64.flat_grads(), th.grad.clone()

    def run(theta_c, x_c, w_c):
        grad = torch.full_like(net.flat_params.data, float("nan"))
        ws = torch.full((net.train_workspace_floats(n),), float("nan"), device="cuda")
        losses, gth = mdn_loss_fwd_bwd(net, theta_c, x_c, w_c, 0.0, grad, want_grad_theta=True, workspace=ws)
        torch.cuda.synchronize()
        return losses, grad, gth

    tc, xc, wc = theta.cuda(), x.cuda(), w.cuda()
    losses, grad, gth = run(tc, xc, wc)
    got = grad.cpu().double()
    assert torch.isfinite(got).all() and torch.isfinite(gth).all() and torch.isfinite(losses).all()
    assert (losses.cpu().double() - loss_ref.detach()).abs().max() <= 1e-5 + 1e-5 * loss_ref.abs().max()
    scale = gref.abs().max().item()
    rel = (got - gref).abs().max().item() / scale
    worst = 0.0
    for key, off, cnt, _ in net._slices():
        a, b = got[off : off + cnt], gref[off : off + cnt]
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale)
        worst = max(worst, e)
        assert e <= 3e-4, f"{key}: {e:.3e}"
    e_th = (gth.cpu().double() - gth_ref).abs().max().item() / gth_ref.abs().max().item()
    record("mdn_train_grad", f"{_id(cfg)} n{n} {'one_x' if one_x else 'paired'}", rel_grad_err_vs_f64=rel,
           worst_block_rel_err=worst, rel_grad_theta_err=e_th)
    print(f"grad rel {rel:.3e} worst block {worst:.3e} d/dtheta rel {e_th:.3e}")
    assert rel <= 2e-4 and e_th <= 3e-4
    # deterministic: a second call, and the same rows as the second half of a longer buffer
    l2, g2, t2 = run(tc, xc, wc)
    assert torch.equal(grad, g2) and torch.equal(gth, t2) and torch.equal(losses, l2)
    big_t = torch.cat([torch.randn(n + 3, D, device="cuda"), tc]).contiguous()
    big_w = torch.cat([torch.rand(n + 3, device="cuda"), wc]).contiguous()
    big_x = xc if one_x else torch.cat([torch.randn(n + 3, x.shape[1], device="cuda"), xc]).contiguous()
    l3, g3, t3 = run(big_t[n + 3:], big_x if one_x else big_x[n + 3:], big_w[n + 3:])
    assert torch.equal(grad, g3) and torch.equal(gth, t3) and torch.equal(losses, l3)


@pytest.mark.parametrize("n", ROWS + [1000])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_one_observation_kernels_are_bit_identical_to_the_paired_kernels(cfg, n):
    _, _, est, theta_d, x_d = mdn_pair(*cfg)
    D, K = cfg[0], cfg[3]
    net = est.net
    theta = theta_d[:n].cuda().contiguous()
    x1 = x_d[7:8].cuda().contiguous()
    xr = x1.expand(n, -1).contiguous()
    assert torch.equal(mdn_log_prob_call(net, theta, x1), mdn_log_prob_call(net, theta, xr))
    g = torch.Generator().manual_seed(3)
    u, zeta = torch.rand(n, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()
    comp = torch.randint(0, K, (n,), generator=g).to(torch.int32).cuda()
    assert torch.equal(mdn_sample_call(net, zeta, x1, u=u), mdn_sample_call(net, zeta, xr, u=u))
    assert torch.equal(mdn_sample_call(net, zeta, x1, comp=comp), mdn_sample_call(net, zeta, xr, comp=comp))


def test_autograd_bridge_and_fused_step():
    from sbi_amd.inference.trainers.fused import FusedMDNStep

    o32, _, est, theta_d, x_d = mdn_pair(3, 5, 32, 4)
    est = copy.deepcopy(est)
    theta, x = theta_d[:200], x_d[:200]
    o32.zero_grad()
    o32.loss(theta, x).mean().backward()
    gref = o32.flat_grads()
    est.zero_grad()
    th = theta.cuda().requires_grad_(True)
    est.loss(th, x.cuda()).mean().backward()
    assert (est.net.flat_params.grad.cpu() - gref).abs().max() <= 2e-4 * gref.abs().max()
    assert th.grad is not None and torch.isfinite(th.grad).all()
    stepper = FusedMDNStep(est, lr=5e-4, clip_max_norm=5.0)
    stepper.loss_and_grad(theta.cuda(), x.cuda())
    assert (stepper.grad.cpu() - gref).abs().max() <= 2e-4 * gref.abs().max()
    first = stepper.step(theta.cuda(), x.cuda()).mean().item()
    for _ in range(40):
        last = stepper.step(theta.cuda(), x.cuda()).mean().item()
    print(f"loss {first:.4f} -> {last:.4f}")
    assert last < first - 0.05
    with pytest.raises(NotImplementedError, match="single-round"):
        stepper.atomic_loss_and_grad(theta.cuda(), x.cuda(), None, None, 10)


@functools.lru_cache(maxsize=None)
def trained_npe():
    """One NPE run with MDNConfig() on the dim-3 linear-Gaussian task of the maf_rqs test, shared by the tests below."""
    from sbi_amd.inference import NPE
    from sbi_amd.neural_nets import MDNConfig
    from sbi_amd.simulators.linear_gaussian import linear_gaussian, true_posterior_linear_gaussian_mvn_prior

    dim, n = 3, 3000
    torch.manual_seed(0)
    shift, cov = -1.0 * torch.ones(dim), 0.3 * torch.eye(dim)
    prior = MultivariateNormal(torch.zeros(dim, device="cuda"), torch.eye(dim, device="cuda"))
    theta = prior.sample((n,)).cpu()
    x = linear_gaussian(theta, shift, cov)
    x_o = torch.zeros(1, dim)
    target = true_posterior_linear_gaussian_mvn_prior(x_o, shift, cov, torch.zeros(dim), torch.eye(dim))
    torch.manual_seed(1)
    inf = NPE(prior=prior, density_estimator=MDNConfig(), device="cuda", show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inf.append_simulations(theta, x).train(training_batch_size=100)
    return inf, theta, x, x_o, target


def test_npe_with_mdn_recovers_the_linear_gaussian_posterior():
    from sbi_amd.diagnostics import run_sbc
    from sbi_amd.utils.metrics import c2st

    inf, theta, x, x_o, target = trained_npe()
    dim = 3
    assert inf._stepper is not None          # the fused device-resident step trained it
    post = inf.build_posterior().set_default_x(x_o)
    samples = post.sample((1000,), show_progress_bars=False).cpu()
    score = c2st(samples, target.sample((1000,))).item()
    print(f"mdn NPE c2st={score:.3f} epochs={inf.summary['epochs_trained'][-1]}")
    record("c2st", "mdn dim3 3k sims", c2st=score)
    assert 0.4 <= score <= 0.6
    assert torch.isfinite(post.log_prob(samples[:5].cuda())).all()
    assert torch.isfinite(post.log_prob_batched(samples[:6].reshape(2, 3, dim).cuda(), x[:3].cuda())).all()
    assert post.sample_batched((4,), x[:3].cuda(), show_progress_bars=False).shape == (4, 3, dim)
    ranks, dap = run_sbc(theta[:50], x[:50], post, num_posterior_samples=100, show_progress_bar=False)
    assert ranks.shape == (50, dim) and torch.isfinite(dap).all()


def test_mcmc_and_rejection_posteriors_sample_the_mdn():
    """`sample_with="mcmc" | "rejection"`: the potential is the MDN's log-prob inside the prior support; the chains tick
    on the MDN's own log_prob kernel (never on the NSF's persistent sampler).  The analytic posterior has mean
    (x_o - shift) / 1.3 = 0.769 and variance 0.3 / 1.3 = 0.231 per coordinate; with 400 draws of 20 chains the mean's
    standard error is below 0.05 even at an autocorrelation time of 4, so 0.2 is four standard errors."""
    inf, theta, x, x_o, target = trained_npe()
    dim = 3
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mcmc = inf.build_posterior(sample_with="mcmc", mcmc_parameters=dict(num_chains=20, warmup_steps=20, thin=2))
        draws = mcmc.sample((400,), x=x_o.cuda(), show_progress_bars=False).cpu()
        assert draws.shape == (400, dim) and torch.isfinite(draws).all()
        assert (draws.mean(0) - target.mean.reshape(-1)).abs().max() <= 0.2
        batched = mcmc.sample_batched((60,), x=x[:3].cuda(), show_progress_bars=False).cpu()
        assert batched.shape == (60, 3, dim) and torch.isfinite(batched).all()
        rej = inf.build_posterior(sample_with="rejection")
        draws = rej.sample((400,), x=x_o.cuda(), show_progress_bars=False).cpu()
        assert draws.shape == (400, dim) and torch.isfinite(draws).all()
        assert (draws.mean(0) - target.mean.reshape(-1)).abs().max() <= 0.2
        with pytest.raises(NotImplementedError):          # (no posterior family samples batched by rejection)
            rej.sample_batched((4,), x=x[:3].cuda(), show_progress_bars=False)


def test_map_tarp_and_lc2st_run_on_the_mdn_posterior():
    from sbi_amd.diagnostics import LC2ST, check_tarp, run_tarp

    inf, theta, x, x_o, target = trained_npe()
    dim = 3
    post = inf.build_posterior().set_default_x(x_o)
    m = post.map(num_iter=50, num_to_optimize=20, num_init_samples=200).cpu().reshape(-1)
    assert m.shape == (dim,) and (m - target.mean.reshape(-1)).abs().max() <= 0.3     # a Gaussian's mode is its mean
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ecp, alpha = run_tarp(theta[:100], x[:100], post, num_posterior_samples=100, show_progress_bar=False)
        atc, ks_p = check_tarp(ecp, alpha)
        assert ecp.shape == alpha.shape and abs(atc) < 0.5 and 0.0 <= ks_p <= 1.0
        xs = x[:400]
        post_samples = post.sample_batched((1,), xs.cuda(), show_progress_bars=False)[0].cpu()
        lc = LC2ST(theta[:400], xs, post_samples, seed=1, num_trials_null=4,
                   classifier_kwargs=dict(max_epochs=20, patience=5))
        lc.train_on_observed_data().train_under_null_hypothesis()
        p = lc.p_value(theta_o=post.sample((300,), show_progress_bars=False).cpu(), x_o=x_o)
    assert 0.0 <= p <= 1.0


def test_abi_refuses_unsupported_configurations_and_zero_condition_rows():
    lib = _lib.load()
    _, _, est, theta_d, x_d = mdn_pair(3, 5, 32, 4)
    net = est.net
    packed = mdn_packed_weights(net)
    theta, x = theta_d[:8].cuda().contiguous(), x_d[:8].cuda().contiguous()
    out = torch.zeros(8, device="cuda")
    st = _lib.current_stream(theta.device)
    for bad in (_lib.MDNConfigC(17, 5, 32, 4, 1e-4), _lib.MDNConfigC(3, 5, 32, 17, 1e-4),
                _lib.MDNConfigC(3, 5, 65, 4, 1e-4), _lib.MDNConfigC(3, 65, 32, 4, 1e-4), _lib.MDNConfigC(0, 5, 32, 4, 1e-4),
                _lib.MDNConfigC(3, 5, 32, 0, 1e-4)):
        assert lib.sbi_amd_mdn_param_count(bad) == _lib.E_UNSUPPORTED
        assert lib.sbi_amd_mdn_packed_floats(bad) == _lib.E_UNSUPPORTED
        assert lib.sbi_amd_mdn_train_workspace_floats(bad, 8) == _lib.E_UNSUPPORTED
        rc = lib.sbi_amd_mdn_log_prob(bad, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(theta), _lib.ptr(x), 8, 8,
                                      _lib.ptr(out), st)
        assert rc == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == 0).all()                       # nothing was launched
    cfg = net.hyper.c_config()
    rc = lib.sbi_amd_mdn_log_prob(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(theta), _lib.ptr(x), 8, 0,
                                  _lib.ptr(out), st)
    assert rc == _lib.E_BADARG
    zeta = torch.zeros(8, 3, device="cuda")
    rc = lib.sbi_amd_mdn_sample(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(out), None, _lib.ptr(zeta),
                                _lib.ptr(x), 8, 0, _lib.ptr(theta.clone()), st)
    assert rc == _lib.E_BADARG
    grad = torch.zeros_like(net.flat_params.data)
    ws = torch.zeros(net.train_workspace_floats(8), device="cuda")
    rc = lib.sbi_amd_mdn_loss_fwd_bwd(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(theta), _lib.ptr(x), 8, 0,
                                      None, 1.0, None, _lib.ptr(grad), None, _lib.ptr(ws), st)
    assert rc == _lib.E_BADARG
    torch.cuda.synchronize()
    assert (out == 0).all() and (grad == 0).all()
    # no rows: every entry point is a no-op that returns 0; the training pass leaves the gradient of an empty sum
    grad.fill_(float("nan"))
    rc = lib.sbi_amd_mdn_loss_fwd_bwd(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), None, None, 0, 1, None, 1.0, None,
                                      _lib.ptr(grad), None, None, st)
    assert rc == 0
    assert lib.sbi_amd_mdn_log_prob(cfg, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(theta), _lib.ptr(x), 0, 1,
                                    _lib.ptr(out), st) == 0
    torch.cuda.synchronize()
    assert (grad == 0).all()
    empty = torch.zeros(0, 3, device="cuda", requires_grad=True)
    est.loss(empty, x[:0]).sum().backward()            # the autograd bridge on an empty batch
    assert empty.grad.shape == (0, 3)
