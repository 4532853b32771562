"""sbi_amd_nre_mcmc_slice_run (csrc/nre_mcmc.hip) across its five instantiations (HP 16 / 32 / 48 / 56 / 64), the edges of
its envelope (D <= 64, C <= 128, H <= 64, NB <= 4) and chain layouts that leave ragged waves: the value it ticks on
against the fp64 oracle, the persistent route against the two-launch loop bit for bit, and launches after the end."""

import functools

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential
from sbi_amd.neural_nets import classifier_nn
from sbi_amd.samplers.mcmc import SliceSamplerVectorized
from sbi_amd.utils.torchutils import BoxUniform
from tests.parity_log import record
from tests.test_nre_gpu import _oracle

pytestmark = pytest.mark.gpu

# (D, C, H, NB): HP, weight scale.  The scale keeps the fp64 oracle's |logit| below 50 on the points of this file
# (asserted below); wider and deeper nets take smaller weights.
NETWORKS = {
    (1, 1, 16, 1): (16, 0.5),
    (2, 5, 7, 2): (16, 0.5),            # H not a multiple of 16
    (5, 3, 32, 4): (32, 0.2),
    (17, 9, 20, 1): (32, 0.3),
    (3, 128, 48, 2): (48, 0.2),
    (3, 3, 50, 2): (56, 0.3),
    (64, 128, 64, 4): (64, 0.13),       # the envelope
    (4, 6, 53, 3): (56, 0.2),           # H = 49 .. 56 is rounded to 56, not to 64: see test_h53_...
}
LAYOUTS = [(1, 1), (3, 23), (69, 1), (2, 200)]        # num_x x chains_per_x
WG_SIZES = {(2, 5, 7, 2): (0, 128, 256), (3, 3, 50, 2): (0, 128, 256)}      # every other network: 0 (the default, 64)


def _packed_floats(D, C, NB, hp):
    """The packed image of csrc/nre.hip for a hidden width padded to `hp`."""
    return hp * (1 + C + D) + 2 * NB * (hp * hp + hp) + hp + 4


@functools.lru_cache(maxsize=None)
def _setup(D, C, H, NB):
    """(estimator on the GPU, fp64 oracle logit, box prior, posterior) of one network, built once."""
    torch.manual_seed(0)
    theta = torch.randn(500, D) * 1.5 + 0.3
    x = theta[:, :1].repeat(1, C) * 0.7 + torch.randn(500, C)
    est = classifier_nn("resnet", hidden_features=H, num_blocks=NB)(theta, x)
    with torch.no_grad():      # weights away from nflows' near-zero init of the last block layer
        est.net.flat_params.normal_(0.0, NETWORKS[(D, C, H, NB)][1])
    est = est.to("cuda")
    _, logit = _oracle(est)
    d = torch.arange(D)
    prior = BoxUniform(-2.0 - 0.25 * (d % 3), 2.0 + 0.5 * (d % 2), device="cuda")      # unequal bounds
    pot, tf = ratio_estimator_based_potential(est, prior, x_o=None)
    return est, logit, prior, MCMCPosterior(pot, prior, tf, device="cuda")


def _spec(post, xs, K):
    post.potential_fn.set_x(xs.repeat_interleave(K, dim=0), x_is_iid=False)
    fused = post._fused_potential_batched(xs, K)
    assert fused is not None and fused.nre_persistent is not None and fused.fused_spec[0] == 2
    return fused


def test_h53_is_padded_to_56_by_both_roundings():
    """csrc/nre.hip (`check_cfg`, which sizes and packs the weight image) and the entry point of csrc/nre_mcmc.hip (which
    picks the kernel instantiation) each round H on their own.  The image size shows the first: 56 for H = 49 .. 56, the
    next multiple of 16 elsewhere.  The second is held by test_one_tick_and_full_runs at H = 53 and 50: a kernel of
    another HP would read that image with the wrong strides and miss the oracle."""
    lib = _lib.load()
    for H, hp in [(7, 16), (16, 16), (17, 32), (20, 32), (48, 48), (49, 56), (50, 56), (53, 56), (56, 56), (57, 64), (64, 64)]:
        cfg = _lib.NREConfigC(4, 6, H, 3)
        assert lib.sbi_amd_nre_packed_floats(cfg) == _packed_floats(4, 6, 3, hp), H
    for net, (hp, _) in NETWORKS.items():
        D, C, H, NB = net
        assert lib.sbi_amd_nre_packed_floats(_lib.NREConfigC(D, C, H, NB)) == _packed_floats(D, C, NB, hp), net


def _launch(lib, nre, bufs, NS, TUNE, seed, tick0, nticks, spec, wg=0):
    kind, p0, p1 = spec
    pk, zs = nre["net"].packed(torch.device("cuda"))
    return lib.sbi_amd_nre_mcmc_slice_run(
        nre["net"].hyper.c_config(), _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(nre["x"]), nre["num_x"], nre["chains_per_x"],
        NS, TUNE, 3.0e38, *[_lib.ptr(bufs[k]) for k in ("x", "nxt", "width", "order", "istate", "fstate", "samples", "done")],
        seed, tick0, nticks, kind, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(nre["low"]), _lib.ptr(nre["high"]),
        nre["prior_log_prob"], _lib.ptr(bufs["theta"]), _lib.ptr(bufs["lad"]), _lib.ptr(bufs["scratch"]), wg,
        _lib.current_stream(torch.device("cuda")))


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l[0]}x{l[1]}")
@pytest.mark.parametrize("net", list(NETWORKS), ids=lambda n: "D{}-C{}-H{}-NB{}".format(*n))
def test_one_tick_and_full_runs(net, layout):
    D, C, H, NB = net
    B, K = layout
    n = B * K
    est, logit, prior, post = _setup(*net)
    g = torch.Generator().manual_seed(B + K)
    xs = torch.randn(B, C, generator=g).cuda()
    fused = _spec(post, xs, K)
    kind, p0, p1 = fused.fused_spec[:3]
    nre = fused.nre_persistent
    lib = _lib.load()
    stream = _lib.current_stream(torch.device("cuda"))
    NS, TUNE, POLL = (2, 1, 5) if D > 8 else (4, 2, 5)

    # 1. one launch of one tick from prepared states: the value the tick reads is log r(theta_c, x_{c // K}) + log p(theta_c)
    u0 = (torch.randn(n, D, generator=g) * 0.8).cuda()
    bufs = dict(x=u0.clone(), nxt=u0.clone(), width=torch.full((n, D), 0.5, device="cuda"),
                order=torch.rand(n, D, generator=g).argsort(1).to(torch.int32).cuda().contiguous(),
                istate=torch.zeros(n, 4, dtype=torch.int32, device="cuda"), fstate=torch.zeros(n, 8, device="cuda"),
                samples=torch.zeros(n, NS, D, device="cuda"), done=torch.zeros(1, dtype=torch.int32, device="cuda"),
                theta=torch.empty(n, D, device="cuda"), lad=torch.empty(n, device="cuda"),
                scratch=torch.full((n,), float("nan"), device="cuda"))
    assert lib.sbi_amd_mcmc_to_constrained(kind, n, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u0), _lib.ptr(bufs["theta"]),
                                           _lib.ptr(bufs["lad"]), stream) == 0
    theta0 = bufs["theta"].clone()
    assert bool(prior.support.check(theta0).all())
    seed = 0x5EED0000 + n
    assert _launch(lib, nre, bufs, NS, TUNE, seed, 0, 1, (kind, p0, p1)) == 0
    with torch.no_grad():
        ref_logit = logit(theta0.cpu().double(), xs.cpu().double().repeat_interleave(K, dim=0))
    assert ref_logit.abs().max() < 50, ref_logit.abs().max()
    ref = ref_logit + prior.log_prob(theta0).cpu().double()
    err = ((bufs["scratch"].cpu().double() - ref).abs() / (1 + ref.abs())).max().item()
    print(f"nre persistent tick D={D} C={C} H={H} NB={NB} {B}x{K}: max err / (1+|ref|) = {err:.2e}, "
          f"max |logit| {ref_logit.abs().max().item():.1f}")
    record("test_one_tick_and_full_runs", f"D{D}-C{C}-H{H}-NB{NB}:{B}x{K}", err_over_1_plus_ref=err,
           max_abs_logit=ref_logit.abs().max().item())
    assert err < 1e-5, err                 # the bar of tests/test_nre_gpu.py
    assert bool((bufs["istate"][:, 0] == 1).all())

    # 3. + 4. on to the end, five ticks per launch (chains finish in the middle of a launch), then once more
    tick = 1
    for _ in range(4000):
        if int(bufs["done"].item()) == n:
            break
        assert _launch(lib, nre, bufs, NS, TUNE, seed, tick, POLL, (kind, p0, p1)) == 0
        tick += POLL
    assert int(bufs["done"].item()) == n and bool((bufs["istate"][:, 0] == 4).all())
    assert torch.isfinite(bufs["samples"]).all()
    before = {k: v.clone() for k, v in bufs.items()}
    assert _launch(lib, nre, bufs, NS, TUNE, seed, tick, POLL, (kind, p0, p1)) == 0
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), k

    # 2. the sampler: persistent against two launches per tick, bit for bit
    init = (torch.randn(n, D, generator=g) * 0.5).cuda()
    runs = []
    for persistent, wg in [(False, 0)] + [(True, w) for w in WG_SIZES.get(net, (0,))]:
        torch.manual_seed(11)
        s = SliceSamplerVectorized(fused, init.clone(), num_chains=n, thin=1, tuning=TUNE, poll_every=POLL,
                                   init_width=0.5, persistent=persistent, nre_wg_size=wg)
        runs.append((s.run(NS).clone(), s))
    (want, two), rest = runs[0], runs[1:]
    assert two.route == "two_launch"
    assert torch.isfinite(want).all() and (n * NS * D < 8 or want.std() > 0.05)
    for got, s in rest:
        assert s.route == "nre_persistent"
        assert s.num_ticks >= two.num_ticks and s.num_ticks - two.num_ticks < POLL
        assert torch.equal(got, want) and torch.equal(s.width, two.width) and torch.equal(s.x, two.x)
