"""Case table and helpers of the vector-field envelope tests (tests/test_vf_envelope_gpu.py, test_npse_envelope_gpu.py,
test_vf_envelope_cpu.py): the shapes at which csrc/fmpe_kernel.h switches paths, and the batch sizes at which its
reductions and its persistent tile loop do.  No test functions here.

Gate for losses and gradients: the project's rule (docstring of tests/test_npse_gpu.py), with the fp64 oracle as the
reference and the fp32 oracle supplying its own distance from it; for gradients it is applied to every parameter block
of `est.net.slices()` on its own, so a block is judged against its own scale."""

import functools
import math

import torch

from oracle.fmpe_oracle import FMPEOracle, sinusoidal_frequencies
from tests.npse_oracle import NPSEOracle
from tests.parity_log import record

# (D, C, H, L, E[, max_freq, noise_scale]): what each case reaches in csrc/fmpe_kernel.h
NET_CASES = [
    dict(D=5, C=3, H=16, L=1, E=2),            # smallest H and E, one frequency
    dict(D=5, C=3, H=17, L=2, E=6),            # odd H, 47 of 64 lanes padding
    dict(D=9, C=4, H=53, L=2, E=34),           # odd H, EB = 3 with a 2-wide last block
    dict(D=3, C=7, H=65, L=1, E=64),           # first H of HB 7, widest E
    dict(D=6, C=5, H=112, L=2, E=16),          # last H of HB 7, E exactly one block
    dict(D=6, C=5, H=113, L=1, E=32),          # first H of HB 8
    dict(D=120, C=5, H=100, L=1, E=32),        # input linear <7,8>, output linear <8,7>
    dict(D=70, C=6, H=128, L=1, E=32),         # <8,7> and <7,8> from the HB 8 side
    dict(D=5, C=120, H=100, L=1, E=32),        # condition linear <7,8>
    dict(D=4, C=3, H=127, L=8, E=32),          # deepest net, odd H
    dict(D=5, C=3, H=100, L=7, E=30, max_freq=10.0, noise_scale=1e-2),   # other frequency base / sigma_min, E % 4 != 0
]

# Batch sizes.  An int is a row count; a tuple (m, a, r) stands for  rows_per_tile * (m * cus + a) + r  rows, with
# cus = multi_processor_count of device 0 (the value fm_grid uses) and rows_per_tile = 128 (64 for NPSE training with
# the control variate, where a wave holds 8 rows twice).  Figures in the comments are for cus = 256.
CUS_PLUS_ONE_RAGGED = (1, 0, 77)               # 128 * cus + 77: cus + 1 tiles, the last with 77 rows
TWO_OR_THREE_TILES = (2, 2, 5)                 # 128 * (2 * cus + 2) + 5: workgroups take two or three tiles
SIZE_NET = dict(D=5, C=3, H=48, L=2, E=32)
SIZE_CASES = [(SIZE_NET, n) for n in (
    1, 127, 128, 129,
    1025,      # 9 tiles, 2 weight-gradient chunks, the second with 8 wave-tiles and one valid row; nln = 72
    2944,      # nchunk 3
    4200,      # nchunk 5
)] + [
    # Staging groups of these two nets, by fm_build_plan's grouping rule (restated as `staging_groups` below and held
    # to 6 / 7 by tests/test_vf_envelope_cpu.py): a hidden image is 112 * 116 + 3 * 112 = 13 328 floats of the 17 920 a
    # group holds, so forward {IN, MA} {CT, MB} {TM, L0} {L1} .. {L(L-1), OUT} = L + 2 groups and backward
    # {OUT, L(L-1)} {L(L-2)} .. {L0} {MA} {MB} = L + 2 groups: an even and an odd count, so the pipe wraps from one tile
    # into the next at both buffer parities.
    (dict(D=5, C=3, H=100, L=4, E=32), CUS_PLUS_ONE_RAGGED),
    (dict(D=5, C=3, H=100, L=5, E=32), CUS_PLUS_ONE_RAGGED),
    (dict(D=5, C=3, H=48, L=1, E=32), TWO_OR_THREE_TILES),
]


def case_id(cfg):
    return "-".join(f"{k}{v}" for k, v in cfg.items())


def size_id(n):
    return str(n) if isinstance(n, int) else f"{n[0]}cus{n[1]:+d}tiles{n[2]:+d}"


def rows_of(n, rows_per_tile=128):
    if isinstance(n, int):
        return n
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return rows_per_tile * (n[0] * cus + n[1]) + n[2]


def hyper_of(cfg):
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import FMPEHyper

    return FMPEHyper(D=cfg["D"], C=cfg["C"], hidden_features=cfg["H"], num_layers=cfg["L"],
                     time_embedding_dim=cfg["E"], sinusoidal_max_freq=cfg.get("max_freq", 1000.0),
                     noise_scale=cfg.get("noise_scale", 1e-3))


# ------------------------------------------------------------------------------------------------ dispatch rules
def _round_up(a, m):
    return (a + m - 1) // m * m


def linears_of(cfg):
    """[(name, OB, KB)] in plan order (IN CT TM MA MB L0.. OUT), as fm_build_plan sets them."""
    D, C, H, L, E = cfg["D"], cfg["C"], cfg["H"], cfg["L"], cfg["E"]
    HB = hb_of(cfg)
    DB, CB, EB = (D + 15) // 16, (C + 15) // 16, (E + 15) // 16
    return ([("IN", HB, DB), ("CT", HB, CB), ("TM", HB, EB), ("MA", HB, HB), ("MB", HB, HB)]
            + [(f"L{l}", HB, HB) for l in range(L)] + [("OUT", DB, HB)])


def hb_of(cfg):
    return 4 if cfg["H"] <= 64 else (7 if cfg["H"] <= 112 else 8)


def dw_pairs_of(cfg):
    """(ot, kt) of every linear's weight-gradient instantiation: the block counts rounded up to 4, 7 or 8."""
    t = lambda b: 4 if b <= 4 else (7 if b <= 7 else 8)
    return [(t(ob), t(kb)) for _, ob, kb in linears_of(cfg)]


def staging_groups(cfg, group_floats=17920):
    """(forward groups, backward groups, packed floats) of the weight staging: fm_build_plan's rule -- images are laid
    out in execution order, a linear opens a new group when its image no longer fits into the current one, and a
    group is padded to 256 floats.  The packed total is what the C ABI shows of it (sbi_amd_fmpe_packed_floats)."""
    lin = {name: (ob, kb) for name, ob, kb in linears_of(cfg)}
    L = cfg["L"]

    def count(order, size):
        groups, used, total = 0, 0, 0
        for k, name in enumerate(order):
            sz = size(*lin[name])
            assert sz <= group_floats
            if k == 0 or used + sz > group_floats:
                groups, used, total = groups + 1, 0, total + _round_up(used, 256)
            used += sz
        return groups, total + _round_up(used, 256)

    fwd, nf = count(["IN", "MA", "CT", "MB", "TM"] + [f"L{l}" for l in range(L)] + ["OUT"],
                    lambda ob, kb: _round_up(16 * ob * (16 * kb + 4) + 3 * 16 * ob, 4))
    bwd, nb = count(["OUT"] + [f"L{l}" for l in reversed(range(L))] + ["MA", "MB"],
                    lambda ob, kb: _round_up(16 * kb * (16 * ob + 4) + 16 * ob, 4))
    return fwd, bwd, nf + nb


# ------------------------------------------------------------------------------------------------ pairs and inputs
def _draw(D, C, n):
    theta = torch.randn(n, D) * torch.linspace(0.5, 2.5, D) + torch.linspace(-1.0, 1.0, D)
    x = torch.randn(n, C) * 0.7 + theta[:, :1] * 0.5 + 0.3
    return theta, x


def _in_fp64(o, E, max_freq):
    """The oracle in fp64, its frequencies included (`.double()` alone keeps the fp32 roundings of div_term)."""
    o = o.double()
    o.div_term.copy_(torch.exp(torch.arange(0, E, 2, dtype=torch.float64) * (-math.log(max_freq) / E)))
    return o


@functools.lru_cache(maxsize=4)
def _fmpe_pair(key, seed):
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import build_flow_matching_estimator

    cfg = dict(key)
    D, C, H, L, E = cfg["D"], cfg["C"], cfg["H"], cfg["L"], cfg["E"]
    mf, ns = cfg.get("max_freq", 1000.0), cfg.get("noise_scale", 1e-3)
    torch.manual_seed(seed)
    theta, x = _draw(D, C, 512)       # always 512 rows: the builder's z-scoring needs more than one
    est = build_flow_matching_estimator(theta, x, hidden_features=H, num_layers=L, time_embedding_dim=E,
                                        sinusoidal_max_freq=mf, noise_scale=ns)
    with torch.no_grad():
        est.net.flat_params.add_(0.05 * torch.randn_like(est.net.flat_params))
    sd = est.net.reference_state_dict()
    o32 = FMPEOracle(D, C, H=H, L=L, E=E, max_freq=mf, noise_scale=ns)
    o64 = _in_fp64(FMPEOracle(D, C, H=H, L=L, E=E, max_freq=mf, noise_scale=ns), E, mf)
    o32.load_reference_state_dict(sd)
    o64.load_reference_state_dict(sd)
    assert torch.equal(o32.div_term, sinusoidal_frequencies(E, mf))
    return o32, o64, est, theta, x, torch.rand(512), torch.randn(512, D)


def make_pair(cfg, n=512, seed=0, device="cuda"):
    """tests/test_fmpe_gpu.py::make_pair with the fp32 and the fp64 oracle and every hyper-parameter of the builder:
    (fp32 oracle, fp64 oracle, estimator on `device`, theta, x, times, noise), the inputs with n rows.  Up to 512 rows
    they are the leading rows of the draw the estimator was built from; larger batches are drawn afresh."""
    o32, o64, est, theta, x, times, noise = _fmpe_pair(tuple(sorted(cfg.items())), seed)
    if n > 512:
        torch.manual_seed(seed + 1)
        theta, x = _draw(cfg["D"], cfg["C"], n)
        times, noise = torch.rand(n), torch.randn(n, cfg["D"])
    return o32, o64, est.to(device), theta[:n], x[:n], times[:n], noise[:n]


def flat_grad_of(oracle, est):
    """tests/test_fmpe_gpu.py::flat_grad_of in the oracle's dtype."""
    return torch.cat([oracle.p[("net." + key).replace(".", "/")].grad.reshape(-1) for key, _, _, _ in est.net.slices()])


def fmpe_loss_and_grad(o, est, th, x, t, nz, w):
    dt = o.mean_0.dtype
    o.zero_grad()
    losses = o.loss(th.to(dt), x.to(dt), t.to(dt), nz.to(dt))
    (losses * w.to(dt)).sum().backward()
    return losses.detach(), flat_grad_of(o, est).clone()


def make_npse_pair(sde, D, C, H, L, E=32, n=512, seed=0, weight="max_likelihood", device="cuda"):
    """tests/test_npse_gpu.py::make_pair with the time-embedding width and batches beyond 512 rows."""
    from sbi_amd.neural_nets import build_score_matching_estimator

    torch.manual_seed(seed)
    theta, x = _draw(D, C, 512)
    est = build_score_matching_estimator(theta, x, sde_type=sde, hidden_features=H, num_layers=L, weight_fn=weight,
                                         time_embedding_dim=E)
    with torch.no_grad():
        est.net.flat_params.add_(0.05 * torch.randn_like(est.net.flat_params))
    sd = est.reference_state_dict()
    o32 = NPSEOracle(D, C, sde=sde, H=H, L=L, E=E, weight=weight)
    o64 = NPSEOracle(D, C, sde=sde, H=H, L=L, E=E, weight=weight).double()
    o32.load_reference_state_dict(sd)
    o64.load_reference_state_dict(sd)
    if n > 512:
        torch.manual_seed(seed + 1)
        theta, x = _draw(D, C, n)
    times = torch.rand(n) * (est.t_max - est.t_min) + est.t_min
    times[0] = est.t_min
    if n > 1:
        times[1] = est.t_max
    return o32, o64, est.to(device), theta[:n], x[:n], times, torch.randn(n, D)


# ------------------------------------------------------------------------------------------------ gates
def dist(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


def held_to_fp64(test, config, what, got, ref32, ref64):
    """tests/test_npse_gpu.py::held_to_fp64: |got - fp64| <= 2 |fp32 reference - fp64| + 2e-5 max|fp64|."""
    err, own, floor = dist(got, ref64), dist(ref32, ref64), 2e-5 * float(ref64.abs().max())
    print(f"{test}[{config}] {what}: |got - fp64| {err:.3e}  |fp32 ref - fp64| {own:.3e}  floor {floor:.3e}")
    record(test, f"{config}:{what}", err_vs_fp64=err, fp32_reference_err_vs_fp64=own, floor=floor)
    assert err <= 2 * own + floor, f"{what}: {err:.3e} > 2 * {own:.3e} + {floor:.3e}"


def blocks_held_to_fp64(test, config, est, got, ref32, ref64):
    """`held_to_fp64` on every parameter block of est.net.slices() separately.  Holds first that no block is small
    against the whole gradient (largest entry >= 1e-3 of the global largest), so that every block is judged on its own
    scale and none against another's; records the block that comes closest to its bound."""
    got, scale = got.double().cpu(), float(ref64.abs().max())
    worst, failures = None, []
    for key, off, cnt, _ in est.net.slices():
        g, r32, r64 = got[off : off + cnt], ref32[off : off + cnt], ref64[off : off + cnt]
        bmax = float(r64.abs().max())
        assert bmax >= 1e-3 * scale, (f"{key}: block maximum {bmax:.3e} below 1e-3 of the gradient's {scale:.3e}: "
                                      "change the seed")
        err, own, floor = dist(g, r64), dist(r32, r64), 2e-5 * bmax
        ratio = err / (2 * own + floor)
        if worst is None or ratio > worst[0]:
            worst = (ratio, key, err, own, floor)
        if not err <= 2 * own + floor:
            failures.append(f"{key}: {err:.3e} > 2 * {own:.3e} + {floor:.3e}")
    _, key, err, own, floor = worst
    print(f"{test}[{config}] gradient, block nearest its bound {key}: |got - fp64| {err:.3e}  |fp32 ref - fp64| "
          f"{own:.3e}  floor {floor:.3e}")
    record(test, f"{config}:gradient", block=key, err_vs_fp64=err, fp32_reference_err_vs_fp64=own, floor=floor)
    assert not failures, "; ".join(failures)
