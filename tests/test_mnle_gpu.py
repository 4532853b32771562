"""GPU parity of the MNLE kernels (csrc/mnle_kernel.h) through the C ABI against the eager restatement
(tests/mnle_oracle.py) on identical perturbed weights and inputs: log_prob / loss / per-part log_prob / logits, mask
properties that do not rest on recalled nflows details, sample for given draws, the fused training pass, the iid-trials
entry point, the autograd bridge and the fused step, end-to-end MNLE on a toy simulator with an analytic likelihood,
the ABI's refusals.
Tolerances as for the MDN path (tests/test_mdn_gpu.py): 1e-5 + 1e-5 max|ref| against the fp32 restatement and "no
further from fp64 than the fp32 restatement is (x2) + 1e-5"; gradients 2e-4 of their max norm, 3e-4 per parameter
block and for d loss / d theta."""
import copy
import functools
import itertools
import json
import math
import os
import warnings

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.estimators.mixed_density_estimator import (mnle_log_prob_call, mnle_loss_fwd_bwd,
                                                                    mnle_packed_weights, mnle_sample_call,
                                                                    mnle_trials_call, split_input)
from tests.mnle_envelope import BASE_CONFIGS as CONFIGS
from tests.mnle_envelope import category_values, mnle_pair_cpu, smooth_rows
from tests.mnle_oracle import toy_log_likelihood, toy_sets, toy_simulator

pytestmark = pytest.mark.gpu

ROWS = [1, 17, 333]
E2E = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnle_e2e.json")


@functools.lru_cache(maxsize=None)
def mnle_pair(name, log_x=False, perturb=0.05, seed=1):
    """(fp32 restatement, fp64 restatement, HIP estimator, theta, x): identical perturbed weights and z-scoring."""
    oracle, oracle64, est, theta, x = mnle_pair_cpu(name, log_x, perturb, seed)
    return oracle, oracle64, est.cuda(), theta, x


def _errs(got, ref32, ref64):
    return (got.double().cpu() - ref64).abs().max().item(), (ref32.double() - ref64).abs().max().item()


def _dev_rows(net, x):
    xc, idx, val = split_input(net, x.cuda())
    return xc, idx, val


@pytest.mark.parametrize("log_x", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_log_prob_loss_parts_and_logits_match_the_restatement(name, n, log_x):
    o32, o64, est, theta_d, x_d = mnle_pair(name, log_x)
    net = est.net
    theta = theta_d[:n].contiguous()
    z0, z1 = net.zstats[0].item(), net.zstats[1].item()
    stress = x_d[1000 - n:].clone()
    zt = torch.where(torch.arange(n) % 2 == 0, torch.tensor(12.0), torch.tensor(-12.0))     # beyond +- tail_bound
    stress[:, 0] = torch.exp((zt - z0) / z1) if log_x else (zt - z0) / z1
    for what, x in (("in-distribution", x_d[:n].contiguous()), ("stress", stress)):
        with torch.no_grad():
            d32, c32 = o32.parts(x, theta)
            d64, c64 = o64.parts(x.double(), theta.double())
            lg32, lg64 = o32.logits(x, theta), o64.logits(x.double(), theta.double())
        xc, idx, val = _dev_rows(net, x)
        th = theta.cuda()
        joint, logits = mnle_log_prob_call(net, xc, idx, val, th, 3, want_logits=True)
        disc = mnle_log_prob_call(net, None, idx, None, th, 1)
        cont = mnle_log_prob_call(net, xc, None, val, th, 2)
        for part, got, r32, r64 in (("joint", joint, d32 + c32, d64 + c64), ("discrete", disc, d32, d64),
                                    ("continuous", cont, c32, c64)):
            e_hip, e_ref = _errs(got, r32, r64)
            e32 = (got.cpu() - r32).abs().max().item()
            print(f"{what} {part}: |hip-o32|={e32:.3e} |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e} "
                  f"max|ref|={r32.abs().max():.1f}")
            assert torch.isfinite(got).all()
            if what == "in-distribution":
                assert e32 <= 1e-5 + 1e-5 * r32.abs().max().item(), part
            assert e_hip <= 2.0 * e_ref + 1e-5, part
        fin = torch.isfinite(lg64)
        assert torch.equal(torch.isneginf(logits.cpu()), ~fin)          # -inf exactly beyond num_categories[v]
        e_hip = (logits.cpu().double()[fin] - lg64[fin]).abs().max().item()
        e_ref = (lg32.double()[fin] - lg64[fin]).abs().max().item()
        print(f"{what} logits: |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
        assert e_hip <= 2.0 * e_ref + 1e-5
        if what == "in-distribution":      # the estimator surface: (B,) loss, (S, B) log_prob, the two views
            loss = est.loss(x.cuda(), th).cpu()
            assert loss.shape == (n,) and torch.equal(loss, -joint.cpu())
            assert torch.equal(est.log_prob(x.cuda(), th).cpu(), joint.cpu()[None])
            assert torch.equal(est.discrete_net.log_prob(x[:, 1:].cuda(), th).cpu(), disc.cpu()[None])
            comb = torch.cat([x[:, 1:], theta], 1).cuda()
            assert torch.equal(est.continuous_net.log_prob(x[:, :1].cuda(), comb).cpu(), cont.cpu()[None])


def test_categorical_probabilities_sum_to_one_and_respect_the_autoregressive_order():
    o32, o64, est, theta_d, x_d = mnle_pair("multi")
    net = est.net
    cats = CONFIGS["multi"][0]
    vals = category_values(cats)
    combos = list(itertools.product(*[range(c) for c in cats]))
    m = 7
    idx = torch.tensor(combos, dtype=torch.int32).repeat(m, 1).cuda().contiguous()             # theta-major blocks
    th = theta_d[:m].repeat_interleave(len(combos), 0).cuda().contiguous()
    lp = mnle_log_prob_call(net, None, idx, None, th, 1).reshape(m, len(combos))
    total = lp.double().exp().sum(1).cpu()
    print("sum of probabilities:", total.tolist())
    assert (total - 1.0).abs().max() <= 1e-5
    # logits of variable v do not move when the variables >= v change
    base = torch.zeros(50, len(cats), dtype=torch.int32)
    g = torch.Generator().manual_seed(3)
    other = torch.stack([torch.randint(0, c, (50,), generator=g) for c in cats], 1).to(torch.int32)
    th50 = theta_d[:50].cuda().contiguous()
    _, lg_base = mnle_log_prob_call(net, None, base.cuda(), None, th50, 1, want_logits=True)
    for v in range(len(cats)):
        changed = base.clone()
        changed[:, v:] = other[:, v:]
        _, lg = mnle_log_prob_call(net, None, changed.cuda().contiguous(), None, th50, 1, want_logits=True)
        assert torch.equal(lg[:, : v + 1], lg_base[:, : v + 1]), v
        if v + 1 < len(cats):
            assert not torch.equal(lg[:, v + 1:], lg_base[:, v + 1:])
    del vals


@pytest.mark.parametrize("log_x", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_sample_follows_the_inverse_cdf_and_the_inverse_flow(name, log_x):
    o32, o64, est, theta_d, x_d = mnle_pair(name, log_x)
    n = 1000
    V = len(CONFIGS[name][0])
    g = torch.Generator().manual_seed(11)
    u = torch.rand(n, V, generator=g)
    noise = torch.randn(n, generator=g)
    with torch.no_grad():
        idx64, x64, gap = o64.sample_given(u.double(), noise.double(), theta_d.double())
        idx32, x32, _ = o32.sample_given(u, noise, theta_d)
    keep = gap > 1e-6
    left_out = int((~keep).sum())
    assert left_out <= n // 100
    idx, xc = mnle_sample_call(est.net, u.cuda(), noise.cuda(), theta_d.cuda())
    assert torch.equal(idx.cpu().long()[keep], idx64[keep])
    same = keep & (idx32 == idx64).all(1)
    ref32 = torch.log(x32[:, 0]) if log_x else x32[:, 0]
    ref64 = torch.log(x64[:, 0]) if log_x else x64[:, 0]
    got = torch.log(xc) if log_x else xc
    e_hip, e_ref = _errs(got[same.cuda()], ref32[same], ref64[same])
    print(f"left out {left_out}; |hip-f64|={e_hip:.3e} |o32-f64|={e_ref:.3e}")
    assert torch.isfinite(xc).all() and e_hip <= 2.0 * e_ref + 1e-5
    full = est.sample_given(u.cuda(), noise.cuda(), theta_d.cuda()).cpu()
    assert torch.equal(full[keep][:, 1:].double(), x64[keep][:, 1:])            # raw values, not indices
    assert est.sample(torch.Size([3]), theta_d[:5].cuda()).shape == (3, 5, 1 + V)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_training_pass_matches_fp64_autograd_and_is_deterministic(name, n):
    o32, o64, est, theta_d, x_d = mnle_pair(name, True)
    net = est.net
    C = CONFIGS[name][1]
    rows, left_out = smooth_rows(name)
    print(f"rows left out of the pool for a ReLU branch that differs between fp32 and fp64: {left_out}")
    assert left_out <= 10          # 1 % of the pool
    theta, x = theta_d[rows[:n]].contiguous(), x_d[rows[:n]].contiguous()
    w = torch.linspace(0.5, 1.5, n) / n if n > 1 else torch.ones(1)
    o64.zero_grad()
    th = theta.double().clone().requires_grad_(True)
    loss_ref = o64.loss(x.double(), th)
    (loss_ref * w.double()).sum().backward()
    gref, gth_ref = o64.flat_grads(), th.grad.clone()

    def run(x_c, th_c, w_c):
        xc, idx, val = _dev_rows(net, x_c)
        grad = torch.full_like(net.flat_params.data, float("nan"))
        ws = torch.full((net.train_workspace_floats(n),), float("nan"), device="cuda")
        losses, gth = mnle_loss_fwd_bwd(net, xc, idx, val, th_c, w_c, 0.0, grad, want_grad_cond=True, workspace=ws)
        torch.cuda.synchronize()
        return losses, grad, gth

    xg, tg, wg = x.cuda(), theta.cuda(), w.cuda()
    losses, grad, gth = run(xg, tg, wg)
    got = grad.cpu().double()
    assert torch.isfinite(got).all() and torch.isfinite(gth).all() and torch.isfinite(losses).all()
    e_loss = (losses.cpu().double() - loss_ref.detach()).abs().max().item()
    print(f"loss err {e_loss:.3e} (max |ref| {loss_ref.abs().max():.2f})")
    assert e_loss <= 1e-5 + 1e-5 * loss_ref.abs().max().item()
    scale = gref.abs().max().item()
    rel = (got - gref).abs().max().item() / scale
    worst = 0.0
    for key, off, cnt, _ in net._slices():
        a, b = got[off: off + cnt], gref[off: off + cnt]
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale)
        worst = max(worst, e)
        assert e <= 3e-4, f"{key}: {e:.3e}"
    e_th = (gth.cpu().double() - gth_ref).abs().max().item() / gth_ref.abs().max().item()
    print(f"grad rel {rel:.3e} worst block {worst:.3e} d/dtheta rel {e_th:.3e}")
    assert rel <= 2e-4 and e_th <= 3e-4
    masked = o32.flat_mask() == 0
    assert masked.any() and (grad.cpu()[masked] == 0).all()          # masked weight entries: exactly zero
    # deterministic: a second call, and the same rows as the tail of a longer buffer
    l2, g2, t2 = run(xg, tg, wg)
    assert torch.equal(grad, g2) and torch.equal(gth, t2) and torch.equal(losses, l2)
    big_x = torch.cat([x_d[500: 500 + n + 3].cuda(), xg]).contiguous()
    big_t = torch.cat([torch.randn(n + 3, C, device="cuda"), tg]).contiguous()
    big_w = torch.cat([torch.rand(n + 3, device="cuda"), wg]).contiguous()
    l3, g3, t3 = run(big_x[n + 3:], big_t[n + 3:], big_w[n + 3:])
    assert torch.equal(grad, g3) and torch.equal(gth, t3) and torch.equal(losses, l3)


@pytest.mark.parametrize("N", [1, 17, 333])
@pytest.mark.parametrize("T", [1, 7, 100])
def test_trials_sum_is_bit_identical_to_the_paired_kernel_in_trial_order(T, N):
    from torch.distributions import Independent, Normal

    from sbi_amd.inference.potentials.likelihood_based_potential import likelihood_estimator_based_potential

    _, _, est, theta_d, x_d = mnle_pair("multi", True)
    net = est.net
    x_o = x_d[100: 100 + T].cuda().contiguous()
    theta = theta_d[:N].cuda().contiguous()
    xc, idx, val = _dev_rows(net, x_o)
    got = mnle_trials_call(net, xc, idx, val, theta)
    acc = torch.zeros(N, dtype=torch.float32, device="cuda")
    for t in range(T):      # explicit fp32 loop over the paired kernel's pair outputs, trial order
        acc = acc + mnle_log_prob_call(net, xc[t: t + 1].expand(N).contiguous(), idx[t: t + 1].expand(N, -1).contiguous(),
                                       val[t: t + 1].expand(N, -1).contiguous(), theta)
    assert torch.equal(got, acc)
    assert torch.equal(est.log_prob_iid_trials(x_o, theta), got)
    prior = Independent(Normal(torch.zeros(3, device="cuda"), 3.0 * torch.ones(3, device="cuda")), 1)
    potential, _ = likelihood_estimator_based_potential(est, prior, x_o)
    assert torch.equal(potential(theta, track_gradients=False), got + prior.log_prob(theta))


def test_autograd_bridge_and_fused_step():
    """Three steps of FusedMNLEStep against the autograd bridge + torch.optim.Adam + clip_grad_norm_.  Both take their
    gradient from the same training kernel; what differs is the Adam arithmetic (fused fp32 kernel against torch's),
    so the parameters agree to 2e-4 of the largest parameter movement (the MDN test's number for the same comparison
    of flat gradients)."""
    from sbi_amd.inference.trainers.fused import FusedMNLEStep

    o32, _, est, theta_d, x_d = mnle_pair("multi", True)
    a, b = copy.deepcopy(est), copy.deepcopy(est)
    theta, x = theta_d[:200], x_d[:200]
    o32.zero_grad()
    o32.loss(x, theta).mean().backward()
    gref = o32.flat_grads()
    th = theta.cuda().requires_grad_(True)
    b.zero_grad()
    b.loss(x.cuda(), th).mean().backward()
    assert (b.net.flat_params.grad.cpu() - gref).abs().max() <= 2e-4 * gref.abs().max()
    assert th.grad is not None and torch.isfinite(th.grad).all()
    p0 = est.net.flat_params.detach().clone()
    stepper = FusedMNLEStep(a, lr=5e-4, clip_max_norm=5.0)
    opt = torch.optim.Adam(b.parameters(), lr=5e-4)
    for _ in range(3):
        stepper.step(x.cuda(), theta.cuda())
        opt.zero_grad()
        b.loss(x.cuda(), theta.cuda()).mean().backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), 5.0)
        opt.step()
    pa, pb = a.net.flat_params.detach(), b.net.flat_params.detach()
    moved = (pa - p0).abs().max().item()
    err = (pa - pb).abs().max().item()
    print(f"largest movement {moved:.3e}, fused vs bridge + Adam {err:.3e}")
    assert moved > 1e-4 and err <= 2e-4 * moved
    with pytest.raises(NotImplementedError, match="atomic"):
        stepper.atomic_loss_and_grad()


# ------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def trained_mnle():
    from sbi_amd.inference import MNLE
    from sbi_amd.neural_nets import MixedConfig
    from sbi_amd.utils import BoxUniform

    theta, x, theta_t, x_t = toy_sets()
    prior = BoxUniform(torch.tensor([-2.0, -1.0], device="cuda"), torch.tensor([2.0, 1.0], device="cuda"))
    torch.manual_seed(1)
    inf = MNLE(prior=prior, density_estimator=MixedConfig(log_transform_x=True), device="cuda",
               show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = inf.append_simulations(theta, x).train(max_num_epochs=30)
    return inf, est, prior


def test_mnle_learns_the_toy_likelihood_and_samples_its_posterior():
    """Metric: mean held-out (analytic - learned) log-likelihood.  Bound: 1.5 x the worst gap of the eager restatement
    trained with torch Adam on the same data and budget with three seeds (tests/golden/mnle_e2e.json,
    tools/make_golden_mnle.py); the margin covers the seed-to-seed variance of a different initialisation stream."""
    from sbi_amd.diagnostics import run_sbc

    inf, est, prior = trained_mnle()
    assert inf._stepper is not None and type(inf._stepper).__name__ == "FusedMNLEStep"
    theta, x, theta_t, x_t = toy_sets()
    with torch.no_grad():
        learned = est.log_prob(x_t.cuda(), theta_t.cuda())[0].cpu()
    gap = (toy_log_likelihood(theta_t, x_t) - learned).mean().item()
    print(f"held-out gap {gap:.4f}")
    recorded = json.load(open(E2E))["gaps"]
    print(f"restatement gaps {recorded}")
    assert len(recorded) == 3 and gap <= 1.5 * max(recorded)
    g = torch.Generator().manual_seed(5)
    theta_o = torch.tensor([[0.8, 0.3]])
    x_o = toy_simulator(theta_o.expand(100, 2), g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        post = inf.build_posterior(mcmc_parameters=dict(num_chains=20, warmup_steps=20, thin=2))
        draws = post.sample((200,), x=x_o.cuda(), show_progress_bars=False).cpu()
        assert draws.shape == (200, 2) and torch.isfinite(draws).all()
        assert (draws >= torch.tensor([-2.0, -1.0])).all() and (draws <= torch.tensor([2.0, 1.0])).all()
        with pytest.raises(NotImplementedError, match="mcmc"):
            inf.build_posterior(sample_with="vi")
        ranks, dap = run_sbc(theta_t[:20], x_t[:20], post, num_posterior_samples=50, show_progress_bar=False)
    assert ranks.shape == (20, 2) and torch.isfinite(dap).all()


def test_abi_refuses_configurations_outside_the_envelope_without_a_launch():
    lib = _lib.load()
    _, _, est, theta_d, x_d = mnle_pair("multi")
    net = est.net
    packed = mnle_packed_weights(net)
    xc, idx, val = _dev_rows(net, x_d[:8])
    theta = theta_d[:8].cuda().contiguous()
    out = torch.zeros(8, device="cuda")
    st = _lib.current_stream(theta.device)

    def cfg(V=3, cats=(2, 5, 3, 0), C=3, Hd=32, NB=1, E=32, H=32, K=8, T=2, L=0):
        return _lib.MNLEConfigC(V, cats, C, Hd, NB, E, H, K, T, L, 0, 10.0, 1e-3, 1e-3, 1e-3)

    bad = [cfg(V=5), cfg(V=0), cfg(cats=(2, 17, 3, 0)), cfg(cats=(2, 0, 3, 0)), cfg(C=65), cfg(C=0), cfg(Hd=65),
           cfg(E=65), cfg(H=65), cfg(H=0), cfg(NB=5), cfg(T=17), cfg(T=0), cfg(K=7), cfg(K=32), cfg(L=5), cfg(L=-1)]
    for b in bad:
        assert lib.sbi_amd_mnle_param_count(b) == _lib.E_UNSUPPORTED
        assert lib.sbi_amd_mnle_packed_floats(b) == _lib.E_UNSUPPORTED
        assert lib.sbi_amd_mnle_train_workspace_floats(b, 8) == _lib.E_UNSUPPORTED
        rc = lib.sbi_amd_mnle_log_prob(b, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                       _lib.ptr(val), _lib.ptr(theta), 8, 8, 3, _lib.ptr(out), None, st)
        assert rc == _lib.E_UNSUPPORTED
        rc = lib.sbi_amd_mnle_log_prob_trials(b, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                              _lib.ptr(val), _lib.ptr(theta), 8, 8, _lib.ptr(out), _lib.ptr(out), st)
        assert rc == _lib.E_UNSUPPORTED
    good = net.hyper.c_config()
    assert lib.sbi_amd_mnle_param_count(good) == net.flat_params.numel()
    rc = lib.sbi_amd_mnle_log_prob(good, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                   _lib.ptr(val), _lib.ptr(theta), 8, 0, 3, _lib.ptr(out), None, st)
    assert rc == _lib.E_BADARG
    rc = lib.sbi_amd_mnle_log_prob(good, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                   _lib.ptr(val), _lib.ptr(theta), 8, 8, 0, _lib.ptr(out), None, st)
    assert rc == _lib.E_BADARG
    grad = torch.zeros_like(net.flat_params.data)
    ws = torch.zeros(net.train_workspace_floats(8), device="cuda")
    gc = torch.zeros(8, 3, device="cuda")
    rc = lib.sbi_amd_mnle_loss_fwd_bwd(good, _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(xc), _lib.ptr(idx),
                                       _lib.ptr(val), _lib.ptr(theta), 8, 1, None, 1.0, None, _lib.ptr(grad),
                                       _lib.ptr(gc), _lib.ptr(ws), st)
    assert rc == _lib.E_BADARG                     # grad_cond_out needs one condition row per data row
    torch.cuda.synchronize()
    assert (out == 0).all() and (grad == 0).all()          # nothing was launched
    grad.fill_(float("nan"))
    rc = lib.sbi_amd_mnle_loss_fwd_bwd(good, _lib.ptr(packed), _lib.ptr(net.zstats), None, None, None, None, 0, 1,
                                       None, 1.0, None, _lib.ptr(grad), None, None, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert (grad == 0).all()
