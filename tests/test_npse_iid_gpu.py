"""GPU parity of NPSE with iid observations (csrc/npse_iid_kernel.h through the C ABI of include/sbi_amd_npse_iid.h):
 * against outputs of the real sbi classes (tests/golden/npse_iid_reference.pt) and
 * against the per-call CPU restatement tests/npse_iid_oracle.py (pinned to those outputs in fp64) on more shapes.

The tolerance is the rule of tests/test_npse_gpu.py (`held_to_fp64`): the distance to the fp64 reference is at most
2 x the fp32 reference's own distance plus 2e-5 * max|ref|; every figure is recorded with tests.parity_log.record."""

import pytest
import torch

from tests.npse_iid_oracle import (IID_CASES, METHODS, iid_score, load_iid_case, make_prior, random_prior_spec,
                                   sample_iid)
from tests.test_npse_gpu import dist, held_to_fp64, make_pair
from tests.test_npse_host_cpu import estimator_of, oracle_of

pytestmark = pytest.mark.gpu


def score_fn(est, method, kind, spec, prec=None, **kw):
    from sbi_amd.inference.potentials.vector_field_adaptor import get_iid_method

    fn = get_iid_method(method)(est, make_prior(kind, spec), device="cuda", **kw)
    if method == "auto_gauss":
        fn.posterior_precision_est_fn = lambda conditions: prec
    return fn


def random_precisions(N, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = torch.randn(N, D, D, generator=g, dtype=torch.float64) * 0.5
    return B @ B.transpose(1, 2) + 0.1 * torch.eye(D, dtype=torch.float64)


def fused_score(fn, est, th, xs, t):
    """The composed score through `sbi_amd_npse_score_iid`, whichever leg `fn(...)` takes by default."""
    from sbi_amd.neural_nets.estimators.score_estimator import score_iid_fused

    lam, mats, vecs, _ = device_tables(fn, t, xs)
    return score_iid_fused(est, th.cuda().contiguous(), xs.cuda().contiguous(), t.float().cuda(), lam,
                           mats[0].contiguous(), vecs[0].contiguous())


def device_tables(fn, times, xs):
    tb = fn.tables(times, xs)
    return (*tb.on("cuda"), tb.base_scale)


# ------------------------------------------------------------------------------------------------ one-step score
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", IID_CASES)
def test_score_against_real_sbi_outputs(name, method):
    from sbi_amd.neural_nets.estimators.score_estimator import score_iid_loop

    g = load_iid_case(name)
    rec = g["methods"][method]
    est = estimator_of(g).cuda()
    fn = score_fn(est, method, g["prior_kind"], g["prior"], g["prec"])
    thq, xs = g["theta_q"].cuda(), g["xs"].cuda()
    for k in range(4):
        t = g["tq"][k : k + 1]
        got = fn(thq.unsqueeze(1), xs, t)
        assert got.shape == (7, 1, 3)
        held_to_fp64("test_score_against_real_sbi_outputs", f"{name}:{method}:t{float(t):.3g}", "default_leg", got[:, 0],
                     rec["score"][k], rec["score64"][k])
        held_to_fp64("test_score_against_real_sbi_outputs", f"{name}:{method}:t{float(t):.3g}", "fused",
                     fused_score(fn, est, g["theta_q"], g["xs"], t), rec["score"][k], rec["score64"][k])
        lam, mats, vecs, _ = device_tables(fn, t, g["xs"])
        loop = score_iid_loop(est, thq, xs, t.cuda(), lam, mats[0].contiguous(), vecs[0].contiguous())
        held_to_fp64("test_score_against_real_sbi_outputs", f"{name}:{method}:t{float(t):.3g}", "host_loop", loop,
                     rec["score"][k], rec["score64"][k])


NETS = [dict(H=48, L=2), dict(H=100, L=5), dict(H=128, L=2)]


@pytest.mark.parametrize("net", NETS, ids=lambda c: f"H{c['H']}L{c['L']}")
@pytest.mark.parametrize("D", [1, 3, 5, 16])
def test_score_matches_oracle_on_shapes(D, net):
    """D in {1, 3, 5, 16} x N in {2, 3, 17} x n in {1, 150} x three trunk widths; methods, priors, SDE families and
    times rotate over the combinations."""
    sdes = ["ve", "vp", "subvp"]
    sde = sdes[(D + net["L"]) % 3]
    o32, o64, est, theta, x, times, _ = make_pair(sde, D=D, C=4, n=256, seed=D, **net)
    combo = 0
    for N in (2, 3, 17):
        for n in (1, 150):
            method = METHODS[combo % 3]
            kind = ("mvn", "indep")[(combo // 3 + D) % 2]
            t = [est.t_min, 0.3, est.t_max, 0.05, 0.7, 0.5][combo]
            combo += 1
            spec = random_prior_spec(D, seed=combo)
            prec = random_precisions(N, D, seed=combo) * (0.05 if combo % 2 else 1.0)
            th, xs = theta[:n] * 1.3, x[10 : 10 + N]
            kw = dict(prec=prec)
            with torch.no_grad():
                r64 = iid_score(o64, method, kind, spec, th.double(), xs.double(), float(torch.tensor(t).float()), **kw)
                r32 = iid_score(o32, method, kind, spec, th, xs, float(torch.tensor(t).float()), **kw)
            fn = score_fn(est, method, kind, spec, prec)
            got = fused_score(fn, est, th, xs, torch.tensor([t]))
            assert got.shape == (n, D) and torch.isfinite(got).all()
            held_to_fp64("test_score_matches_oracle_on_shapes", f"{sde}-D{D}-H{net['H']}L{net['L']}-N{N}-n{n}",
                         f"{method}:{kind}", got, r32, r64)


# ------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", IID_CASES)
def test_sampler_with_given_noise_against_the_real_diffuser(name, method):
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_iid_fused, sample_sde_iid_loop

    g = load_iid_case(name)
    s = g["methods"][method]["em"]
    est = estimator_of(g).cuda()
    fn = score_fn(est, method, g["prior_kind"], g["prior"], g["prec"])
    lam, mats, vecs, scale = device_tables(fn, s["ts"][:-1], g["xs"])
    assert scale == pytest.approx(5**-0.5 if method == "fnpe" else 1.0)
    xs, ts, noise = g["xs"].cuda(), s["ts"].cuda(), s["noise"].cuda().contiguous()
    fused = sample_sde_iid_fused(est, 32, xs, ts, lam, mats, vecs, 1.0, noise, base_scale=scale)
    loop = sample_sde_iid_loop(est, 32, xs, ts, lam, mats, vecs, 1.0, noise, base_scale=scale)
    t = "test_sampler_with_given_noise_against_the_real_diffuser[iid]"
    held_to_fp64(t, f"{name}:{method}", "fused", fused, s["out"], s["out64"])
    held_to_fp64(t, f"{name}:{method}", "host_loop", loop, s["out"], s["out64"])
    own, floor = dist(s["out"], s["out64"]), 2e-5 * float(s["out64"].abs().max())
    assert dist(fused, loop.cpu()) <= 2 * own + floor


@pytest.mark.parametrize("method,sde,kind", [("fnpe", "ve", "mvn"), ("gauss", "vp", "indep"), ("auto_gauss", "vp", "mvn")])
def test_sampler_20_steps_two_tiles_against_the_oracle_replay(method, sde, kind):
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_iid_fused, sample_sde_iid_loop

    D, N, n = 5, 3, 150       # two workgroup tiles, the second partly filled; the default net: several staging groups
    o32, o64, est, theta, x, _, _ = make_pair(sde, D=D, C=3)
    # + 2 I: with weaker precisions the 20-step trajectories of this random net diverge (max|theta| ~ 5e5 in fp64) and the
    # max-norm rule would be set by a few rows; with these every row stays below ~35
    spec, prec = random_prior_spec(D, 3), random_precisions(N, D, 3) + 2.0 * torch.eye(D, dtype=torch.float64)
    torch.manual_seed(9)
    ts = est.solve_schedule(21).cpu()
    noise = torch.randn(21, n, D)
    xs = x[:N]
    r32 = sample_iid(o32, method, kind, spec, xs, ts, noise, prec=prec)
    r64 = sample_iid(o64, method, kind, spec, xs.double(), ts.double(), noise.double(), prec=prec)
    fn = score_fn(est, method, kind, spec, prec)
    lam, mats, vecs, scale = device_tables(fn, ts[:-1], xs)
    fused = sample_sde_iid_fused(est, n, xs.cuda(), ts.cuda(), lam, mats, vecs, 1.0, noise.cuda(), base_scale=scale)
    loop = sample_sde_iid_loop(est, n, xs.cuda(), ts.cuda(), lam, mats, vecs, 1.0, noise.cuda(), base_scale=scale)
    t = "test_sampler_20_steps_two_tiles_against_the_oracle_replay"
    held_to_fp64(t, f"{method}:{sde}:{kind}", "fused", fused, r32, r64)
    held_to_fp64(t, f"{method}:{sde}:{kind}", "host_loop", loop, r32, r64)
    assert dist(fused, loop.cpu()) <= 2 * dist(r32, r64) + 2e-5 * float(r64.abs().max())
    assert float(r64.abs().max()) < 300, "the replay must stay bounded for the max-norm rule to pin every row"
    # zero steps: the initial draw, mean_base + scaled std_base * z_0
    z0 = noise[:1].cuda().contiguous()
    start = sample_sde_iid_fused(est, n, xs.cuda(), ts[:1].cuda(), lam, mats[:0], vecs[:0], 1.0, z0, base_scale=scale)
    want = (est.mean_base.double() + est.std_base.double() * scale * z0[0].double()).cpu()
    assert dist(start, want) <= 1e-6 * float(want.abs().max())


def test_one_observation_composes_to_the_plain_sampler():
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_fused, sample_sde_iid_fused

    o32, o64, est, theta, x, _, _ = make_pair("vp", D=5, C=3, H=64, L=2)
    spec = random_prior_spec(5, 1)
    torch.manual_seed(4)
    ts = est.solve_schedule(21)
    noise = torch.randn(21, 150, 5).cuda()
    eye = torch.eye(5).cuda()
    for method in METHODS:
        fn = score_fn(est, method, "mvn", spec, random_precisions(1, 5))
        lam, mats, vecs, scale = device_tables(fn, ts[:-1].cpu(), x[:1])
        assert lam is None and scale == 1.0
        assert torch.equal(mats[:, 0], eye.expand(20, 5, 5)) and torch.equal(mats[:, 1], eye.expand(20, 5, 5))
        assert float(mats[:, 2].abs().max()) == 0 and float(vecs.abs().max()) == 0
    plain = sample_sde_fused(est, 150, x[:1].cuda(), ts, 1.0, noise)
    iid = sample_sde_iid_fused(est, 150, x[:1].cuda(), ts, lam, mats, vecs, 1.0, noise)
    r64 = o64.sample_sde(x[:1].double(), ts.cpu().double(), noise.cpu().double(), 1.0)
    floor = 2e-5 * float(r64.abs().max())
    print(f"N=1: |iid - plain| {dist(iid, plain.cpu()):.3e}  floor {floor:.3e}")
    assert dist(iid, plain.cpu()) <= floor          # the summation order differs: no bit-equality


def test_batch_independence_and_rng_contract():
    from sbi_amd.inference.posteriors.vector_field_posterior import VectorFieldPosterior
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_iid_fused

    _, _, est, theta, x, _, _ = make_pair("vp", D=5, C=3, H=64, L=2)
    spec, N = random_prior_spec(5, 2), 4
    xs = x[:N].cuda()
    ts = est.solve_schedule(21)
    fn = score_fn(est, "auto_gauss", "mvn", spec, random_precisions(N, 5, 2))
    lam, mats, vecs, scale = device_tables(fn, ts[:-1].cpu(), x[:N])
    run = lambda n, **kw: sample_sde_iid_fused(est, n, xs, ts, lam, mats, vecs, 1.0, None, base_scale=scale, **kw)
    a, b, c = run(150, seed=123), run(150, seed=123), run(150, seed=124)
    assert torch.equal(a, b) and torch.isfinite(a).all() and (a != c).float().mean() > 0.99
    assert torch.equal(run(1, seed=123), a[:1])                                # row 0 does not depend on n or its tile
    assert torch.equal(run(50, seed=123, row_offset=100), a[100:])             # split calls reproduce the whole call
    noise = torch.randn(21, 150, 5).cuda()
    whole = sample_sde_iid_fused(est, 150, xs, ts, lam, mats, vecs, 1.0, noise, base_scale=scale)
    one = sample_sde_iid_fused(est, 1, xs, ts, lam, mats, vecs, 1.0, noise[:, :1].contiguous(), base_scale=scale)
    assert torch.equal(one, whole[:1])
    # the host loop follows the same Philox draws (sbi_amd_npse_sde_normals) and composes row by row
    # (sbi_amd_npse_compose_iid), so it shares both properties bit for bit
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_iid_loop

    lp = lambda n, **kw: sample_sde_iid_loop(est, n, xs, ts, lam, mats, vecs, 1.0, None, scale, **kw)
    la = lp(150, seed=123)
    assert torch.equal(lp(50, seed=123, row_offset=100), la[100:]) and torch.equal(lp(1, seed=123), la[:1])
    assert torch.equal(lp(150, seed=123), la)
    replay = torch.stack([__import__("sbi_amd.neural_nets.estimators.score_estimator", fromlist=["x"])
                          .sde_normals(150, 5, k, 123, 0, "cuda") for k in range(21)])
    assert torch.equal(sample_sde_iid_fused(est, 150, xs, ts, lam, mats, vecs, 1.0, replay, base_scale=scale), a)
    # ... so posterior.sample does not depend on max_sampling_batch_size
    prior = make_prior("mvn", spec, device="cuda")
    post = VectorFieldPosterior(est, prior, sample_with="sde")
    kw = dict(x=xs, steps=21, iid_method="gauss")
    torch.manual_seed(5)
    whole = post.sample((1000,), max_sampling_batch_size=1000, **kw)
    torch.manual_seed(5)
    split = post.sample((1000,), max_sampling_batch_size=128, **kw)
    torch.manual_seed(6)
    other = post.sample((1000,), **kw)
    assert whole.shape == (1000, 5) and torch.equal(whole, split) and not torch.equal(whole, other)
    # ... also where the prior's support rejects draws (fnpe under BoxUniform): a rounding difference would flip a
    # rejection and shift every later row
    from sbi_amd.utils.torchutils import BoxUniform

    bkw = dict(x=xs, steps=21, iid_method="fnpe")
    wide = BoxUniform(-1e9 * torch.ones(5, device="cuda"), 1e9 * torch.ones(5, device="cuda"))
    torch.manual_seed(5)       # the prior's bounds do not enter fnpe's tables: choose them so that about half is rejected
    free = VectorFieldPosterior(est, wide, sample_with="sde").sample((600,), **bkw)
    bound = float(free.abs().max(-1).values.median())
    box = BoxUniform(-bound * torch.ones(5, device="cuda"), bound * torch.ones(5, device="cuda"))
    bpost = VectorFieldPosterior(est, box, sample_with="sde")
    torch.manual_seed(5)
    bw = bpost.sample((600,), max_sampling_batch_size=1000, **bkw)
    torch.manual_seed(5)
    bs = bpost.sample((600,), max_sampling_batch_size=128, **bkw)
    torch.manual_seed(5)
    unrejected = bpost.sample((600,), max_sampling_batch_size=1000, reject_outside_prior=False, **bkw)
    from sbi_amd.utils.sbiutils import within_support

    inside = within_support(box, unrejected).float().mean()
    print(f"fnpe under BoxUniform: {float(inside):.3f} of the draws inside the support")
    assert bw.shape == (600, 5) and torch.equal(bw, bs) and 0.3 < float(inside) < 0.7
    import sbi_amd.neural_nets.estimators.score_estimator as se

    default_leg = se.IID_DEFAULT_FUSED
    try:                      # the same through the fused sampler
        se.IID_DEFAULT_FUSED = True
        torch.manual_seed(5)
        w2 = post.sample((1000,), max_sampling_batch_size=1000, **kw)
        torch.manual_seed(5)
        s2 = post.sample((1000,), max_sampling_batch_size=128, **kw)
    finally:
        se.IID_DEFAULT_FUSED = default_leg
    assert w2.shape == (1000, 5) and torch.equal(w2, s2)
    # one observation: iid_method is accepted and ignored
    torch.manual_seed(5)
    single = post.sample((64,), x=xs[:1], steps=21, iid_method="gauss")
    torch.manual_seed(5)
    assert torch.equal(single, post.sample((64,), x=xs[:1], steps=21))
    # the potential's gradient is the same composed score
    from sbi_amd.inference.potentials.vector_field_potential import vector_field_estimator_based_potential

    pot, _ = vector_field_estimator_based_potential(est, make_prior("mvn", spec), None)
    pot.set_x(xs, x_is_iid=True, iid_method="gauss")
    t = torch.tensor([0.4])
    want = score_fn(est, "gauss", "mvn", spec)(a[:9].unsqueeze(1), xs, t)[:, 0]
    assert torch.equal(pot.gradient(a[:9], t), want)


@pytest.mark.parametrize("D,N,n", [(17, 3, 40), (3, 1025, 4)], ids=["D17", "N1025"])
def test_outside_the_envelope_the_loop_leg_matches_the_oracle(D, N, n):
    from sbi_amd.neural_nets.estimators.score_estimator import iid_fused_supported, sample_sde_iid

    o32, o64, est, theta, x, _, _ = make_pair("vp", D=D, C=3, H=48, L=2, n=1100)
    assert not iid_fused_supported(est, N)
    spec = random_prior_spec(D, 5)
    torch.manual_seed(2)
    ts = est.solve_schedule(6).cpu()
    noise = torch.randn(6, n, D)
    xs = x[:N]
    r32 = sample_iid(o32, "gauss", "mvn", spec, xs, ts, noise)
    r64 = sample_iid(o64, "gauss", "mvn", spec, xs.double(), ts.double(), noise.double())
    fn = score_fn(est, "gauss", "mvn", spec)
    lam, mats, vecs, scale = device_tables(fn, ts[:-1], xs)
    got = sample_sde_iid(est, n, xs.cuda(), ts.cuda(), lam, mats, vecs, 1.0, base_scale=scale, noise=noise.cuda())
    held_to_fp64("test_outside_the_envelope_the_loop_leg_matches_the_oracle", f"D{D}-N{N}", "dispatch", got, r32, r64)
    th = theta[:n] * 1.2
    with torch.no_grad():
        s64 = iid_score(o64, "gauss", "mvn", spec, th.double(), xs.double(), 0.5)
        s32 = iid_score(o32, "gauss", "mvn", spec, th, xs, 0.5)
    sc = fn(th.cuda().unsqueeze(1), xs.cuda(), torch.tensor([0.5]))[:, 0]
    held_to_fp64("test_outside_the_envelope_the_loop_leg_matches_the_oracle", f"D{D}-N{N}", "score", sc, s32, s64)


def test_auto_gauss_estimates_and_caches_its_precisions():
    """The estimate path itself: sample_batched on the single-observation sampler, second moment, inverse, cache."""
    from sbi_amd.inference.potentials.vector_field_adaptor import AutoGaussCorrectedScoreFn

    _, _, est, theta, x, _, _ = make_pair("vp", D=5, C=3, H=64, L=2)
    xs = x[:3].cuda()
    kw = dict(precision_est_budget=400, precision_initial_sampler_steps=10)
    fn = AutoGaussCorrectedScoreFn(est, make_prior("mvn", random_prior_spec(5, 2)), device="cuda", **kw)
    torch.manual_seed(1)
    prec = fn.posterior_precision_est_fn(xs)
    assert prec.shape == (3, 5, 5) and prec.dtype == torch.float64 and torch.isfinite(prec).all()
    assert float((prec - prec.transpose(1, 2)).abs().max()) <= 1e-9 * float(prec.abs().max())
    assert float(torch.linalg.eigvalsh(0.5 * (prec + prec.transpose(1, 2))).min()) > 0
    torch.manual_seed(2)       # a second call is served from the estimator's cache: no new draws
    assert fn.posterior_precision_est_fn(xs) is prec
    assert fn.posterior_precision_est_fn(xs.clone() + 1.0) is not prec
    diag = AutoGaussCorrectedScoreFn(est, fn.prior, device="cuda", precision_est_only_diag=True, **kw)
    assert diag.posterior_precision_est_fn(xs).shape == (3, 5) and diag.tables(torch.tensor([0.5]), xs).lam.shape == (3, 5, 5)
    with torch.no_grad():      # new parameters invalidate the cache
        est.net.flat_params.add_(0.01)
    assert fn.posterior_precision_est_fn(xs) is not prec
