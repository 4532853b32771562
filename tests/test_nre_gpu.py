"""NRE on the HIP kernels: log-ratio parity against the fp64 oracle, the iid-trials kernel, the training gradient of
the four trainers against fp64 autograd through the oracle, determinism, and NRE_B / NRE_C end to end on the linear
Gaussian (the reference's tests/linearGaussian_snre_test.py)."""

import warnings

import pytest
import torch
from torch.distributions import MultivariateNormal

from oracle.nsf_oracle import ResidualNet
from sbi_amd.inference import NRE_B, NRE_C
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential
from sbi_amd.inference.trainers.nre.nre import (MODE_A, MODE_B, MODE_BNRE, MODE_C, FusedNREStep, draw_atoms,
                                                row_losses_torch)
from sbi_amd.neural_nets import classifier_nn
from sbi_amd.simulators.linear_gaussian import linear_gaussian, true_posterior_linear_gaussian_mvn_prior
from sbi_amd.utils.metrics import check_c2st
from sbi_amd.utils.sbiutils import within_support
from sbi_amd.utils.torchutils import BoxUniform

pytestmark = pytest.mark.gpu


def _estimator(D, C, H, NB, seed=0, n=500, std=0.3):
    torch.manual_seed(seed)
    theta = torch.randn(n, D) * 1.5 + 0.3
    x = theta[:, :1].repeat(1, C) * 0.7 + torch.randn(n, C)
    est = classifier_nn("resnet", hidden_features=H, num_blocks=NB)(theta, x)
    with torch.no_grad():      # weights away from nflows' near-zero init of the last block layer
        est.net.flat_params.normal_(0.0, std)
    return est.to("cuda"), theta, x


def _oracle(est, dtype=torch.float64):
    h = est.net.hyper
    net = ResidualNet(h.D + h.C, 1, h.H, None, h.NB).to(dtype)
    sd = {k[len("net."):]: v for k, v in est.state_dict().items() if k.startswith("net.")}
    net.load_state_dict({k: v.to(dtype).cpu() for k, v in sd.items()})
    zs = est.net.zstats.detach().cpu().to(dtype)
    D, C = h.D, h.C

    def logit(theta, x):
        zt = (theta.to(dtype) - zs[:D]) / zs[D : 2 * D]
        zx = (x.to(dtype) - zs[2 * D : 2 * D + C]) / zs[2 * D + C :]
        return net(torch.cat([zt, zx], dim=1)).squeeze(-1)

    return net, logit


# (the 96-input, four-block net takes smaller weights: with N(0, 0.3) its activations reach several hundred)
CONFIGS = [(1, 3, 50, 2, 0.3), (3, 5, 32, 1, 0.3), (10, 10, 50, 2, 0.3), (7, 20, 16, 3, 0.3), (32, 64, 64, 4, 0.1),
           (2, 2, 48, 2, 0.3)]


@pytest.mark.parametrize("D,C,H,NB,std", CONFIGS)
def test_log_ratio_parity_against_fp64_oracle(D, C, H, NB, std):
    est, theta, x = _estimator(D, C, H, NB, std=std)
    _, ref_fn = _oracle(est)
    n = 3000
    th = torch.randn(n, D) * 1.5
    xx = torch.randn(n, C) * 1.2
    for x_rows in (n, 1):
        xr = xx[:x_rows]
        with torch.no_grad():
            got = est(th.cuda(), xr.expand(n, C).contiguous().cuda() if x_rows == 1 else xr.cuda()).cpu().double()
            if x_rows == 1:
                one = est.log_ratio_one_x(th.cuda(), xr.cuda()).cpu().double()
                assert torch.equal(one, got)        # the folded single-x path gives the per-pair path's bits
        ref = ref_fn(th.double(), xr.expand(n, C).double())
        err = ((got - ref).abs() / (1 + ref.abs())).max().item()
        _, ref32 = _oracle(est, torch.float32)
        e32 = ((ref32(th, xr.expand(n, C)).double() - ref).abs() / (1 + ref.abs())).max().item()
        print(f"nre log-ratio D={D} C={C} H={H} NB={NB} x_rows={x_rows}: max err / (1+|ref|) = {err:.2e} "
              f"(torch fp32: {e32:.2e})")
        # 1e-5 (1 + |ref|) of fp64 (measured <= 6e-6)
        assert err < 1e-5, (err, e32)


def test_trials_kernel_sums_the_pairs_and_is_bit_stable():
    est, _, _ = _estimator(4, 6, 50, 2)
    T, N = 37, 1000
    xt = torch.randn(T, 6, device="cuda")
    th = torch.randn(N, 4, device="cuda")
    s = est.log_ratio_iid_trials(xt, th)
    with torch.no_grad():
        pairs = est._log_ratio_rows(th.repeat_interleave(T, dim=0), xt, T).reshape(N, T)
    assert torch.equal(s, pairs.double().sum(1).float())
    assert torch.equal(s, est.log_ratio_iid_trials(xt, th))
    perm = torch.randperm(N, device="cuda")
    assert torch.equal(est.log_ratio_iid_trials(xt, th[perm]), s[perm])
    # one trial: the folded single-x path
    s1 = est.log_ratio_iid_trials(xt[:1], th)
    assert torch.equal(s1, est.log_ratio_one_x(th, xt[:1]))


def _ref_atoms(theta, choices):
    return torch.cat([theta[None], theta[choices].permute(1, 0, 2)], dim=0)       # (A, B, D) atoms-major


@pytest.mark.parametrize("mode,D,C,H,NB,B,std", [(MODE_A, 3, 5, 50, 2, 64, 0.1), (MODE_B, 3, 5, 50, 2, 64, 0.1),
                                                 (MODE_C, 3, 5, 50, 2, 64, 0.1), (MODE_BNRE, 3, 5, 50, 2, 64, 0.1),
                                                 (MODE_B, 1, 3, 16, 1, 67, 0.2), (MODE_B, 32, 64, 64, 4, 67, 0.04),
                                                 (MODE_C, 7, 9, 32, 3, 45, 0.1)])
def test_training_gradient_against_fp64_autograd(mode, D, C, H, NB, B, std):
    # batches that are not a multiple of 16 leave partial row sub-chunks in the weight-gradient reduction; H = 64 with
    # 96 inputs needs more than one 4 x 4 output tile per thread
    # (weights that keep |logit| well below 17: beyond, sigmoid rounds to 1 in fp32 and BCELoss's gradient -- the
    # reference's as well as the kernel's -- vanishes where fp64 still has one)
    est, theta, x = _estimator(D, C, H, NB, seed=mode, std=std, n=max(500, B))
    th, xx = theta[:B].cuda(), x[:B].cuda()
    A = {MODE_A: 2, MODE_BNRE: 2, MODE_B: 10, MODE_C: 6}[mode]
    g = torch.Generator().manual_seed(7)

    def choices(k):
        return torch.stack([torch.randperm(B - 1, generator=g)[: k - 1] for _ in range(B)])

    def fix(c):       # rows != b: shift indices >= b by one (uniform over the other rows)
        b = torch.arange(B)[:, None]
        return c + (c >= b).long()

    if mode == MODE_C:
        ch = (fix(choices(A)), fix(choices(A - 1)) if A - 1 > 1 else None)
    else:
        ch = fix(choices(A))
    step = FusedNREStep(est, mode, A, gamma=1.3, regularization_strength=7.0, lr=1e-3, clip_max_norm=5.0)
    flat0 = est.net.flat_params.detach().clone()
    loss = step.loss_and_grad(th, xx, choices=ch)
    grad = step.grad.clone()
    # fp64 reference: the same atoms through the oracle, the reference's loss restated per row, autograd
    net, _ = _oracle(est)
    zs = est.net.zstats.detach().cpu().double()
    thc = th.cpu().double()
    if mode == MODE_C:
        atoms = torch.cat([_ref_atoms(thc, ch[0]), _ref_atoms(thc, ch[1]) if ch[1] is not None else thc[None]])
    else:
        atoms = _ref_atoms(thc, ch)
    zt = (atoms.reshape(-1, D) - zs[:D]) / zs[D : 2 * D]
    zx = ((xx.cpu().double() - zs[2 * D : 2 * D + C]) / zs[2 * D + C :]).repeat(atoms.shape[0], 1)
    logits = net(torch.cat([zt, zx], 1)).squeeze(-1)
    assert logits.abs().max() < 12
    rows = row_losses_torch(mode, logits, B, A, 1.3, 7.0)
    rows.mean().backward()
    ref_grad = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    # the losses: BCELoss on an fp32 sigmoid carries the cancellation of 1 - sigmoid(l) that the reference's fp32 loss
    # has as well, so they are held against the restatement evaluated in fp32 on the oracle's logits
    rows32 = row_losses_torch(mode, logits.detach().float(), B, A, 1.3, 7.0).double()
    lerr = ((loss.double().cpu() - rows32).abs() / (1 + rows32.abs())).max().item()
    print(f"nre mode {mode}: max |loss err| / (1 + |loss|) = {lerr:.2e}")
    assert lerr < 2e-5
    gerr = ((grad.double().cpu() - ref_grad).abs().max() / ref_grad.abs().max()).item()
    print(f"nre mode {mode}: max |grad err| / max |grad| = {gerr:.2e}")
    assert gerr < 2e-5          # (measured <= 8.3e-6 over the four losses)
    # one fused clip + Adam step equals torch's on the oracle (fp32 noise)
    net32, _ = _oracle(est, torch.float32)
    step.apply()
    est_params = est.net.flat_params.detach().clone()
    assert not torch.equal(est_params, flat0)
    opt = torch.optim.Adam(net32.parameters(), lr=1e-3)
    for p, r in zip(net32.parameters(), torch.split(grad.cpu(), [p.numel() for p in net32.parameters()])):
        p.grad = r.reshape(p.shape).clone()
    torch.nn.utils.clip_grad_norm_(net32.parameters(), 5.0)
    opt.step()
    want = torch.cat([p.detach().reshape(-1) for p in net32.parameters()])
    assert torch.allclose(est_params.cpu(), want, atol=2e-6, rtol=1e-5)


def test_two_seeded_trainings_are_bit_identical():
    torch.manual_seed(3)
    theta = torch.randn(1000, 2)
    x = linear_gaussian(theta, -1.0 * torch.ones(2), 0.8 * torch.eye(2))

    def run():
        torch.manual_seed(5)
        inf = NRE_B(device="cuda", show_progress_bars=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = inf.append_simulations(theta, x).train(max_num_epochs=3, training_batch_size=100)
        assert isinstance(inf._stepper, FusedNREStep)
        return est, inf

    a, ia = run()
    b, ib = run()
    assert torch.equal(a.net.flat_params, b.net.flat_params)
    assert ia.summary["validation_loss"] == ib.summary["validation_loss"]


@pytest.mark.parametrize("trainer,num_dim,prior_str", [(NRE_B, 2, "gaussian"), (NRE_B, 3, "uniform"),
                                                       (NRE_C, 2, "gaussian")])
def test_c2st_nre_on_linear_gaussian(trainer, num_dim, prior_str):
    num_samples, num_simulations = 500, 3000
    shift, cov = -1.0 * torch.ones(num_dim), 0.8 * torch.eye(num_dim)
    torch.manual_seed(0)
    if prior_str == "gaussian":
        prior = MultivariateNormal(torch.zeros(num_dim, device="cuda"), torch.eye(num_dim, device="cuda"))
    else:
        prior = BoxUniform(-2.0 * torch.ones(num_dim), 2.0 * torch.ones(num_dim), device="cuda")
    theta = prior.sample((num_simulations,)).cpu()
    x = linear_gaussian(theta, shift, cov)
    inf = trainer(prior=prior, device="cuda", show_progress_bars=False)
    estimator = inf.append_simulations(theta, x).train()
    x_o = torch.zeros(1, num_dim)
    potential_fn, theta_transform = ratio_estimator_based_potential(estimator, prior, x_o.cuda())
    posterior = MCMCPosterior(potential_fn, prior, theta_transform, num_chains=20, thin=3, warmup_steps=100,
                              init_strategy="resample", device="cuda")
    samples = posterior.sample((num_samples,), x=x_o, show_progress_bars=False)
    assert getattr(posterior.potential_, "fused_spec", None) is not None        # the trials-kernel tick ran
    assert samples.shape == (num_samples, num_dim) and torch.isfinite(samples).all()
    if prior_str == "uniform":
        assert bool(within_support(prior, samples).all())
        g = MultivariateNormal(x_o[0] - shift, cov)
        target = g.sample((8 * num_samples,))
        target = target[within_support(prior.to("cpu"), target)][:num_samples]
        prior = prior.to("cuda")
    else:
        target = true_posterior_linear_gaussian_mvn_prior(x_o, shift, cov, torch.zeros(num_dim),
                                                          torch.eye(num_dim)).sample((num_samples,))
    th = samples[:200].contiguous()
    potential_fn.set_x(x_o.cuda())
    fused = potential_fn(th, track_gradients=False)
    generic = potential_fn(th, track_gradients=True).detach()
    assert torch.allclose(fused, generic, atol=1e-4, rtol=1e-5)
    check_c2st(samples.cpu(), target, alg=f"{trainer.__name__}-{prior_str}-{num_dim}d", tol=0.1)    # (measured 0.52 - 0.55)


def test_map_and_rejection_through_the_ratio_potential():
    torch.manual_seed(2)
    prior = BoxUniform(-2.0 * torch.ones(2), 2.0 * torch.ones(2), device="cuda")
    theta = prior.sample((1500,)).cpu()
    x = linear_gaussian(theta, -1.0 * torch.ones(2), 0.8 * torch.eye(2))
    inf = NRE_B(prior=prior, device="cuda", show_progress_bars=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inf.append_simulations(theta, x).train(max_num_epochs=30)
    x_o = torch.zeros(1, 2)
    rej = inf.build_posterior(sample_with="rejection").set_default_x(x_o)
    r = rej.sample((50,), show_progress_bars=False)
    assert r.shape == (50, 2) and bool(within_support(prior, r).all())
    # gradients of the potential w.r.t. theta come through the kernels' backward
    pot, _ = ratio_estimator_based_potential(inf._neural_net, prior, x_o.cuda())
    th = (torch.rand(16, 2, device="cuda") * 2 - 1).requires_grad_(True)
    pot(th, track_gradients=True).sum().backward()
    eps = 1e-2
    with torch.no_grad():
        e0 = torch.tensor([eps, 0.0], device="cuda")
        fd = (pot(th + e0, track_gradients=False) - pot(th - e0, track_gradients=False)) / (2 * eps)
    assert torch.allclose(th.grad[:, 0], fd, atol=5e-2, rtol=5e-2)
    with pytest.raises(NotImplementedError, match="mcmc"):
        inf.build_posterior(sample_with="vi")
    # draws reach the atoms kernel on the device
    a = draw_atoms(theta[:10].cuda().contiguous(), 3, 11)
    assert a.shape == (3, 10, 2) and torch.equal(a[0], theta[:10].cuda())
