"""Configurations, row lists and helpers of the mixture-density-network parity tests (tests/test_mdn_gpu.py,
test_mdn_envelope_gpu.py, test_mdn_envelope_cpu.py): the shapes and row counts at which csrc/mdn_kernel.h and the host
side in csrc/mdn.hip take another path, a restatement of that host side's plan in Python, the matched (restatement,
estimator) pairs, and the chunked fp32 / fp64 references.  Importable without a GPU; no test functions here.

Bounds are the project's (docstring of tests/test_mdn_gpu.py): forward quantities finite and "no further from fp64 than
the fp32 restatement is (x2) + 1e-5", in-distribution log_prob additionally within 1e-5 + 1e-5 max|ref| of the fp32
restatement; for the training pass 1e-5 + 1e-5 max|ref| on the losses, 2e-4 of the gradient's max norm, 3e-4 per
parameter block (relative to max(|block|, 1e-3 max|gradient|)) and 3e-4 for d loss / d theta.
"""
import copy
import functools

import torch

from tests.helpers import linear_gaussian_data
from tests.mdn_oracle import MDNOracle

# name: (D, C, H, K)
CONFIGS = {
    "corner": (16, 64, 64, 16),     # every maximum: KS1 = 16, ld1 = 66, R = 153, ~150 KiB of LDS at 4 waves
    "floor": (1, 1, 1, 1),          # every minimum; no upper head; 10 parameters
    "ksh13": (4, 4, 52, 4),         # last H on 13 K-steps; D = 4 with R = 15; K*D = 16 exactly one gradient plane
    "ksh16": (5, 5, 53, 3),         # first H on 16 K-steps; D = 5 with R = 21; C = 5 one past a K-step
    "wideC": (11, 63, 17, 3),       # C = 63; K*D = 33 (one past two planes); K*U = 165
    "oneK": (16, 3, 33, 1),         # K = 1; K*D = 16; K*U = 120
    "thinH": (2, 17, 1, 16),        # H = 1 with K = 16
    "defaults": (10, 10, 50, 10),   # already in tests/test_mdn_gpu.py; used for the large-row cases
}
NEW_CONFIGS = [name for name in CONFIGS if name != "defaults"]
SOFTPLUS_CONFIGS = {"mid": (3, 5, 32, 4), "defaults": CONFIGS["defaults"], "corner": CONFIGS["corner"]}
SOFTPLUS_SHIFT = 19.4               # added to the raw-diagonal bias of the odd components: raw entries straddle 20
POOL_ROWS = 1000
LARGE_SEED = 2                      # the large-row pools: another seed than the 1000-row pool's (0)

ROWS = [1, 17, 333]
# last row count on 1 wave per workgroup, first on 2, last on 2, first on 4 (8161 and 16321 leave a last workgroup
# with one valid row and whole invalid waves)
WAVE_ROWS = [8160, 8161, 16320, 16321]
WAVE_CONFIGS = ["defaults", "ksh16"]
# weight-gradient chunks of 512 rows in sub-chunks of 128: 1, 1, 1, 2, 3 partial slabs
CHUNK_ROWS = [128, 129, 512, 513, 1025]
CHUNK_CONFIGS = ["defaults", "wideC", "floor"]
# (n, condition rows): x[i % x_rows] with 1 < x_rows < n and x_rows > n
XROWS_CASES = [(17, 2), (17, 7), (17, 40), (513, 3), (513, 500)]
# one-observation kernels: 512 workgroups of 4 waves, 16 rows (log_prob) / 64 rows (sample) per wave and trip
BCAST_LOG_PROB_ROWS = 32768 + 17
BCAST_SAMPLE_ROWS = 131072 + 65
BCAST_CONFIGS = ["defaults", "floor"]
SELECT_CONFIGS = ["defaults", "floor", "oneK"]
REF_CHUNK = 2048                    # rows per evaluation of a restatement

MAF_DW_CHUNK = 512
LDS_LIMIT_BYTES = 160 * 1024
MDN_LDH, MDN_ZW = 66, 17


# ---------------------------------------------------------------------- the plan of csrc/mdn.hip, restated
def _round_up(v, m):
    return (v + m - 1) // m * m


def _two_odd(v):
    x = (v + 1) // 2
    if x % 2 == 0:
        x += 1
    return 2 * x


def plan(D, C, H, K):
    """mdn_build_plan(): the sizes (floats) the launches and the workspace are computed from."""
    U = D * (D - 1) // 2
    R = 1 + 2 * D + U
    MT = (R + 15) // 16
    RP = 16 * MT
    KS1 = (C + 3) // 4
    ld1 = _two_odd(4 * KS1)
    hid = _round_up(64 * ld1 + 64 + 64 * MDN_LDH + 64 + 16 * MDN_LDH + 16, 4)
    slice_floats = RP * MDN_LDH + RP
    SW = RP + 4
    sc = _round_up(3 * 16 * MDN_ZW, 4)
    sc = _round_up(sc + 16 * ld1, 4)
    sc_total = _round_up(sc + 16 * SW, 4)
    bc_total = _round_up(16 * MDN_ZW + 16 * ld1 + 64 * MDN_ZW, 4)
    outs, ins = (H, H, K, K * D, K * D, K * U), (C, H, H, H, H, H)
    return dict(D=D, C=C, H=H, K=K, U=U, R=R, MT=MT, RP=RP, KS1=KS1, ld1=ld1, hid_floats=hid, slice_floats=slice_floats,
                img_floats=hid + K * slice_floats, n_params=sum(o * i + o for o, i in zip(outs, ins)), SW=SW,
                sc_total=sc_total, bc_total=bc_total)


def ksh(cfg):
    """mdn_ksh(): K-steps of the register-chained hidden GEMMs."""
    return 13 if (cfg[2] + 3) // 4 <= 13 else 16


def paired_lds_bytes(cfg, nw):
    P = plan(*cfg)
    return 4 * (P["hid_floats"] + P["slice_floats"] + nw * P["sc_total"])


def bcast_lds_bytes(cfg, nw=4):
    P = plan(*cfg)
    return 4 * (P["hid_floats"] + P["K"] * P["RP"] + P["slice_floats"] + nw * P["bc_total"])


def waves(cfg, n):
    """mdn_waves(): the largest workgroup (4, 2, 1 waves of 16 rows) that fits LDS and still yields 256 of them."""
    nw = 4
    while nw > 1 and ((n + 16 * nw - 1) // (16 * nw) < 256 or paired_lds_bytes(cfg, nw) > LDS_LIMIT_BYTES):
        nw >>= 1
    return nw


def nchunks(n):
    return (max(n, 1) + MAF_DW_CHUNK - 1) // MAF_DW_CHUNK


def workspace_floats(cfg, n):
    """The formula in include/sbi_amd_mdn.h, each term rounded up to a multiple of 4."""
    D, C, H, K = cfg
    U = D * (D - 1) // 2
    npad = nchunks(n) * MAF_DW_CHUNK

    def planes(o):
        return (o + 15) // 16

    terms = [npad * 3 * 64, npad * 16 * (8 + 1 + 2 * planes(K * D) + planes(K * U)),
             (npad // MAF_DW_CHUNK) * plan(*cfg)["n_params"]]
    return sum(_round_up(t, 4) for t in terms)


def bcast_grid_and_trips(n, sample):
    """mdn_launch_bcast(): (workgroups, trips of the busiest wave) over 16-row tiles (log_prob) / 64-row groups."""
    per = 64 if sample else 16
    units = (n + per - 1) // per
    grid = min(max((units + 3) // 4, 1), 512)
    return grid, (units + 4 * grid - 1) // (4 * grid)


# ---------------------------------------------------------------------- matched pairs
@functools.lru_cache(maxsize=None)
def mdn_pair_cpu(D, C, H, K, perturb=0.05, seed=1, diag_shift=0.0):
    """(fp32 restatement, fp64 restatement, HIP estimator on the CPU, theta, x): identical perturbed weights and
    z-scoring; theta and x are the 1000-row pool the estimator was built from.  `diag_shift` is added to
    `_unconstrained_diagonal_layer.bias` of the odd components before the weights are copied."""
    from sbi_amd.neural_nets.net_builders.mdn import build_mdn

    theta, x = linear_gaussian_data(POOL_ROWS, D, C)
    torch.manual_seed(seed)
    est = build_mdn(theta, x, hidden_features=H, num_components=K)
    oracle = MDNOracle(D, C, H, K)
    oracle.set_zstats(est.net.zstats)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in oracle.parameters():
            p.add_(perturb * torch.randn(p.shape, generator=g))
        if diag_shift:
            oracle.net._unconstrained_diagonal_layer.bias.reshape(K, D)[1::2] += diag_shift
    est.load_state_dict(oracle.state_dict())
    assert torch.equal(est.net.flat_params.detach(), oracle.flat_params())
    return oracle, copy.deepcopy(oracle).double(), est, theta, x


@functools.lru_cache(maxsize=None)
def mdn_pair_gpu(D, C, H, K, perturb=0.05, seed=1, diag_shift=0.0):
    """The same with a copy of the estimator on the device (the CPU one stays where it is)."""
    o32, o64, est, theta, x = mdn_pair_cpu(D, C, H, K, perturb, seed, diag_shift)
    return o32, o64, copy.deepcopy(est).cuda(), theta, x


@functools.lru_cache(maxsize=None)
def large_pool(name, n):
    """(theta, x) rows for the wave-count and broadcast cases: `linear_gaussian_data` with another seed than the
    estimator's pool."""
    D, C = CONFIGS[name][:2]
    return linear_gaussian_data(n, D, C, seed=LARGE_SEED)


def sample_draws(n, D, K, seed=5):
    """The sampling tests' draws: components (n,) int64, normal draws (n, D), uniforms (n,)."""
    g = torch.Generator().manual_seed(seed + n)
    return torch.randint(0, K, (n,), generator=g), torch.randn(n, D, generator=g), torch.rand(n, generator=g)


def bcast_subset(n, sample):
    """Rows of a looping one-observation launch that are held to fp64: the first tile (16 rows; 64 for the sampler),
    the tiles on both sides of the wrap to the workgroups' second trip, and everything up to the last partial tile."""
    per = 64 if sample else 16
    wrap = 512 * 4 * per
    return torch.cat([torch.arange(0, per), torch.arange(wrap - per, n)])


def training_weights(n, seed=7):
    """Non-uniform row weights of the order 1 / n with exact zeros (every 5th row, and the last one when n > 1)."""
    g = torch.Generator().manual_seed(seed + n)
    w = (0.5 + torch.rand(n, generator=g)) / n
    if n > 1:
        w[3::5] = 0.0
        w[-1] = 0.0
    return w


# ---------------------------------------------------------------------- references (chunked, restatement's precision)
def _dtype(o):
    return next(o.parameters()).dtype


def row_chunks(n):
    return [(s, min(s + REF_CHUNK, n)) for s in range(0, n, REF_CHUNK)]


def _x_rows(x, s, e):
    return x if x.shape[0] == 1 else x[s:e]


def packed_factors(A, D):
    """(n, K, D, D) upper-triangular factors -> the kernels' (n, K, D + U): diagonal, then np.triu_indices(D, 1)."""
    idx = torch.arange(D)
    r, c = torch.triu_indices(D, D, 1)
    return torch.cat([A[..., idx, idx], A[..., r, c]], -1)


def errs(got, ref32, ref64):
    """(max |got - fp64|, max |fp32 restatement - fp64|)."""
    return (got.double().cpu() - ref64).abs().max().item(), (ref32.double() - ref64).abs().max().item()


def ref_components(o, x):
    """(logits (n, K), means (n, K, D), packed factors (n, K, D + U)) of the condition rows."""
    dt, out = _dtype(o), []
    with torch.no_grad():
        for s, e in row_chunks(x.shape[0]):
            lg, mu, A = o.components(x[s:e].to(dt))
            out.append((lg, mu, packed_factors(A, o.D)))
    return tuple(torch.cat(p) for p in zip(*out))


def ref_log_prob(o, theta, x):
    """log p(theta_i | x_i), or log p(theta_i | x_0) for a single condition row; (n,)."""
    dt, out = _dtype(o), []
    with torch.no_grad():
        for s, e in row_chunks(theta.shape[0]):
            th, xx = theta[s:e].to(dt), _x_rows(x, s, e).to(dt)
            out.append(o.log_prob(th[:, None], xx)[:, 0] if x.shape[0] == 1 else o.log_prob(th, xx))
    return torch.cat(out)


def ref_sample(o, comp, zeta, x):
    dt, out = _dtype(o), []
    with torch.no_grad():
        for s, e in row_chunks(zeta.shape[0]):
            out.append(o.sample_given(comp[s:e], zeta[s:e].to(dt), _x_rows(x, s, e).to(dt)))
    return torch.cat(out)


def ref_pick(o64, u, x):
    """Components the fp64 restatement selects for the uniforms `u` (the number of cumulative weights <= u, clamped),
    and the rows further than 1e-5 from every cumulative boundary: (comp (n,), keep (n,))."""
    n, K = u.shape[0], o64.K
    comp, keep = [], []
    with torch.no_grad():
        for s, e in row_chunks(n):
            cum = o64.cumulative_weights(_x_rows(x, s, e).double()).expand(e - s, K).contiguous()
            ud = u[s:e].double()[:, None]
            comp.append(torch.searchsorted(cum, ud, right=True)[:, 0].clamp(max=K - 1))
            keep.append(((cum - ud).abs() > 1e-5).all(1))
    return torch.cat(comp), torch.cat(keep)


def training_reference(o, theta, x, w):
    """(per-row losses, flat parameter gradient, d / d theta) of sum_i w_i loss_i by autograd in the restatement's own
    precision, the gradients accumulated over row chunks; returned as fp64.  x: (n, C) or (1, C)."""
    dt = _dtype(o)
    o.zero_grad()
    losses, gth = [], []
    for s, e in row_chunks(theta.shape[0]):
        th = theta[s:e].to(dt).clone().requires_grad_(True)
        xx = _x_rows(x, s, e).to(dt)
        loss = o.loss(th[:, None], xx)[:, 0] if x.shape[0] == 1 else o.loss(th, xx)
        (loss * w[s:e].to(dt)).sum().backward()
        losses.append(loss.detach().double())
        gth.append(th.grad.double())
    out = torch.cat(losses), o.flat_grads().double().clone(), torch.cat(gth)
    o.zero_grad()
    return out


def training_distances(net, got, gth, gref, gth_ref):
    """(whole-gradient distance / max norm, worst block distance / max(|block|, 1e-3 scale) with its key, d / d theta
    distance / max norm) of a flat gradient and a theta gradient against fp64 references."""
    got, gth = got.double().cpu(), gth.double().cpu()
    scale = gref.abs().max().item()
    rel = (got - gref).abs().max().item() / scale
    worst, worst_key = 0.0, None
    for key, off, cnt, _ in net._slices():
        a, b = got[off: off + cnt], gref[off: off + cnt]
        e = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale)
        if worst_key is None or e > worst:
            worst, worst_key = e, key
    e_th = (gth - gth_ref).abs().max().item() / gth_ref.abs().max().item()
    return rel, worst, worst_key, e_th


def raw_diagonal(o, x):
    """The pre-softplus diagonal entries (n, K, D) of the condition rows."""
    with torch.no_grad():
        h = o.net._hidden_net(o._embedding_net(x.to(_dtype(o))))
        return o.net._unconstrained_diagonal_layer(h).reshape(x.shape[0], o.K, o.D)


def softplus_fraction(name):
    """Share of the shifted (odd) components' raw diagonal entries above softplus's threshold of 20 over the 1000-row
    pool, in the fp64 restatement."""
    o64, x = softplus_pair_cpu(name)[1], softplus_pair_cpu(name)[4]
    return (raw_diagonal(o64, x)[:, 1::2] > 20.0).double().mean().item()


def softplus_pair_cpu(name):
    return mdn_pair_cpu(*SOFTPLUS_CONFIGS[name], diag_shift=SOFTPLUS_SHIFT)


@functools.lru_cache(maxsize=None)
def softplus_theta(name, n, one_x):
    """theta rows drawn from the fp64 mixture itself for the first n condition rows (or the first alone), component
    i % K: the shifted components have a precision factor of ~20 on their diagonal and take no responsibility for the
    pool's own theta rows, so those rows alone would leave their gradients at zero in the kernel and in the reference
    alike."""
    _, o64, _, _, x = softplus_pair_cpu(name)
    D, K = SOFTPLUS_CONFIGS[name][0], SOFTPLUS_CONFIGS[name][3]
    g = torch.Generator().manual_seed(23)
    zeta = torch.randn(n, D, generator=g)
    return ref_sample(o64, torch.arange(n) % K, zeta, x[:1] if one_x else x[:n]).float().contiguous()
