"""sbi_amd_mcmc_slice_run (csrc/nsf_coop_kernel.h, MC = true) across its ten instantiations (num_bins 4 / 5 / 8 / 10 / 16
x hidden K-steps 13 / 16), both priors the fused tick knows, chain counts around the 16-chain workgroup, and more than
4096 chains: the persistent route against the two-launch loop bit for bit, and its log-density against the fp64
oracle."""

import pytest
import torch
from torch.distributions import MultivariateNormal

from sbi_amd import _lib
from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior
from sbi_amd.inference.potentials.posterior_based_potential import posterior_estimator_based_potential
from sbi_amd.neural_nets.estimators.nsf_flow import packed_weights
from sbi_amd.samplers.mcmc import SliceSamplerVectorized
from sbi_amd.utils.sbiutils import mcmc_transform
from sbi_amd.utils.torchutils import BoxUniform
from tests.helpers import matched_pair
from tests.parity_log import record
from tests.test_nsf_parity_gpu import ATOL, RTOL, _assert_as_accurate_as_fp32_reference

pytestmark = pytest.mark.gpu

# hidden_features 50 -> 13 hidden K-steps, 32 -> 16 (csrc/nsf_plan_layout.h: KSH)
TEN = [dict(D=4, C=3, num_bins=K, hidden_features=H) for K in (4, 5, 8, 10, 16) for H in (50, 32)]
NETS = TEN + [
    dict(D=2, C=32, num_bins=10, hidden_features=50),          # the widest context the cooperative kernels take
    dict(D=10, C=3, num_bins=16, hidden_features=50),          # d_tr * PT = 5 * 3 = 15: the edge of d_tr * PT <= 16
    dict(D=4, C=3, num_bins=10, hidden_features=50, num_blocks=1),
]
# what the entry point refuses (E_UNSUPPORTED; the sampler then takes two launches per tick), with the refusing line
REFUSED = [
    (dict(D=12, C=3, num_bins=16, hidden_features=50),
     "nsf_coop_plan.cpp, coop_build_plan: `!wide && pl.shape[0].d_tr * pl.PT > 16` (6 * 3 final-layer tiles)"),
    (dict(D=4, C=33, num_bins=10, hidden_features=50),
     "nsf_coop_plan.cpp, coop_build_plan: `pl.C > (wide ? 64 : 32)` (the context K-steps live in registers)"),
]
CHAINS = (1, 16, 17, 100)
NS, TUNE, POLL = 4, 2, 16


def _ids(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def _prior(kind, D):
    if kind == "gaussian":
        return MultivariateNormal(torch.zeros(D, device="cuda"), torch.eye(D, device="cuda"))
    d = torch.arange(D)
    return BoxUniform(-2.0 - 0.25 * (d % 3), 2.0 + 0.5 * (d % 2), device="cuda")


def _fused(cfg, prior_kind):
    oracle, est, _, x = matched_pair(**cfg)
    prior = _prior(prior_kind, cfg["D"])
    potential_fn, _ = posterior_estimator_based_potential(est, prior, x_o=None)
    post = MCMCPosterior(potential_fn, prior, mcmc_transform(prior, device="cuda"), device="cuda")
    x_o = x[:1].cuda()
    post.set_default_x(x_o)
    post.potential_fn.set_x(x_o, x_is_iid=True)
    fused = post._fused_potential()
    assert fused is not None and len(fused.fused_spec) == 6
    assert fused.fused_spec[0] == (1 if prior_kind == "gaussian" else 2)
    return fused, oracle, x[:1]


def _both_routes(fused, D, chains):
    g = torch.Generator().manual_seed(chains)
    init = (torch.randn(chains, D, generator=g) * 0.3).cuda()
    out = []
    for persistent in (True, False):
        torch.manual_seed(11)
        s = SliceSamplerVectorized(fused, init.clone(), num_chains=chains, thin=1, tuning=TUNE, poll_every=POLL,
                                   init_width=0.3, persistent=persistent)
        out.append((s.run(NS).clone(), s))
    return out


def test_none_of_the_ten_instantiations_is_in_the_refusal_table():
    assert len(TEN) == 10 and not any(cfg in TEN for cfg, _ in REFUSED)


@pytest.mark.parametrize("prior_kind", ["gaussian", "box"])
@pytest.mark.parametrize("cfg", NETS, ids=_ids)
def test_persistent_route_equals_the_two_launch_loop(cfg, prior_kind):
    """Same Philox counters, same log-density kernel (<= 4096 rows: the one-tile cooperative forward on both routes) ->
    the same chains, bit for bit, at every chain count: one chain, a full 16-chain workgroup, one chain more, and
    seven workgroups with a partial last one."""
    fused, _, _ = _fused(cfg, prior_kind)
    for chains in CHAINS:
        (a, sa), (b, sb) = _both_routes(fused, cfg["D"], chains)
        assert sa.route == "persistent" and sb.route == "two_launch", (chains, sa.route, sb.route)
        assert sa.num_ticks >= sb.num_ticks and sa.num_ticks - sb.num_ticks < POLL
        assert torch.equal(a, b), chains
        assert torch.equal(sa.width, sb.width) and torch.equal(sa.x, sb.x), chains
        assert torch.isfinite(a).all() and a.std() > 0.02


@pytest.mark.parametrize("cfg,reason", REFUSED, ids=lambda v: _ids(v) if isinstance(v, dict) else "")
def test_refused_configurations_take_the_two_launch_route(cfg, reason):
    fused, _, _ = _fused(cfg, "gaussian")
    (a, sa), (b, sb) = _both_routes(fused, cfg["D"], 17)
    assert sa.route == "two_launch" == sb.route, reason
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_more_than_4096_chains_one_tick_against_the_oracle():
    """4100 chains = 257 workgroups, the last one with 4 chains: one launch of one tick.  The log-density the tick read
    (logp_scratch) is held to the oracle at the gate of tests/test_nsf_parity_gpu.py, and every chain has left ST_BEGIN."""
    cfg = dict(D=4, C=3)
    fused, oracle, x_o = _fused(cfg, "gaussian")
    kind, p0, p1, _, net, x_row = fused.fused_spec
    n, D = 4100, cfg["D"]
    lib = _lib.load()
    stream = _lib.current_stream(torch.device("cuda"))
    g = torch.Generator().manual_seed(5)
    u0 = (torch.randn(n, D, generator=g) * 0.3).cuda()
    f = lambda *shape: torch.zeros(*shape, device="cuda")                      # noqa: E731
    i = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda")   # noqa: E731
    x, nxt, width = u0.clone(), u0.clone(), torch.full((n, D), 0.3, device="cuda")
    order = torch.rand(n, D, generator=g).argsort(1).to(torch.int32).cuda().contiguous()
    istate, fstate, samples, done = i(n, 4), f(n, 8), f(n, 1, D), i(1)
    theta, lad, scratch = f(n, D), f(n), torch.full((n,), float("nan"), device="cuda")
    assert lib.sbi_amd_mcmc_to_constrained(kind, n, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u0), _lib.ptr(theta),
                                           _lib.ptr(lad), stream) == 0
    theta0 = theta.clone().cpu()
    packed = packed_weights(net, rows=None)
    rc = lib.sbi_amd_mcmc_slice_run(net.hyper.c_config(), _lib.ptr(packed), _lib.ptr(net.zstats), _lib.ptr(x_row), n, 1, 0,
                                    3.0e38, _lib.ptr(x), _lib.ptr(nxt), _lib.ptr(width), _lib.ptr(order), _lib.ptr(istate),
                                    _lib.ptr(fstate), _lib.ptr(samples), _lib.ptr(done), 7, 0, 1, kind, _lib.ptr(p0),
                                    _lib.ptr(p1), _lib.ptr(theta), _lib.ptr(lad), _lib.ptr(scratch), stream)
    assert rc == 0
    got = scratch.cpu()
    xx = x_o.expand(n, -1)
    with torch.no_grad():
        ref = oracle.log_prob(theta0, xx)[0]
        ref64 = oracle.double().log_prob(theta0.double(), xx.double())[0]
        oracle.float()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print(f"4100 chains: max|persistent - oracle32| = {err:.3e}, max|ref| = {ref.abs().max().item():.1f}")
    record("test_more_than_4096_chains_one_tick_against_the_oracle", "D4-C3", max_abs_vs_oracle32=err,
           max_abs_ref=ref.abs().max().item())
    assert err <= ATOL + RTOL * ref.abs().max().item()
    _assert_as_accurate_as_fp32_reference(got, ref, ref64, "persistent tick log_prob, 4100 chains")
    assert bool((istate[:, 0] == 1).all()) and int(done.item()) == 0
    assert not torch.equal(nxt, u0) and bool((nxt != u0).any(dim=1).all())
