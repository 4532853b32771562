"""NPSE (csrc/npse.hip, modes 3-6 of fm_fwd_kernel) on the batch sizes of tests/vf_envelope.py: the trunk is the one
tests/test_vf_envelope_gpu.py covers, the row-to-tile mapping and the score prologue / epilogue are NPSE's own.  Beyond
one tile per workgroup the existing suite only holds these kernels to "deterministic and finite".

Gates: the project's rule (tests/vf_envelope.py::held_to_fp64), for gradients on every parameter block separately;
score / ode_fn 2e-5 * max|fp64|, the number of tests/test_npse_gpu.py."""

import pytest
import torch

from tests.test_npse_gpu import oracle_loss_and_grad
from tests.vf_envelope import (CUS_PLUS_ONE_RAGGED, blocks_held_to_fp64, dist, held_to_fp64, make_npse_pair, rows_of,
                               size_id)

pytestmark = pytest.mark.gpu

# with the control variate a wave holds 8 rows twice, a tile 64 rows: 64 * cus + 37 rows are cus + 1 tiles
CV_CUS_PLUS_ONE_RAGGED = (1, 0, 37)
LOSS_CASES = [
    (dict(sde="vp", D=5, C=3, H=100, L=4), CV_CUS_PLUS_ONE_RAGGED, True),      # 6 staging groups
    (dict(sde="ve", D=5, C=3, H=100, L=5), CV_CUS_PLUS_ONE_RAGGED, True),      # 7 staging groups
    (dict(sde="subvp", D=5, C=3, H=48, L=2), CUS_PLUS_ONE_RAGGED, False),
    (dict(sde="subvp", D=5, C=3, H=48, L=2), 1025, False),                     # 2 weight-gradient chunks, nln = 72
    (dict(sde="vp", D=9, C=4, H=53, L=2, E=34), 333, True),                    # EB = 3 with a 2-wide last block
    (dict(sde="vp", D=9, C=4, H=53, L=2, E=34), 333, False),
]


def _id(cfg, size, cv):
    return "-".join(f"{k}{v}" for k, v in cfg.items()) + f"-n{size_id(size)}" + ("" if cv else "_nocv")


@pytest.mark.parametrize("cfg,size,cv", LOSS_CASES, ids=[_id(*c) for c in LOSS_CASES])
def test_loss_and_gradients_match_oracle(cfg, size, cv):
    from sbi_amd.neural_nets.estimators.score_estimator import loss_fwd_bwd, train_workspace

    n = rows_of(size, 64 if cv else 128)
    o32, o64, est, th, xx, tt, ee = make_npse_pair(**cfg, n=n)
    w = torch.linspace(0.5, 1.5, n) / n
    l64, g64 = oracle_loss_and_grad(o64, est, th, xx, tt, ee, w, cv)
    l32, g32 = oracle_loss_and_grad(o32, est, th, xx, tt, ee, w, cv)
    thr = 0.3 if cv else 0.0
    grad = torch.empty_like(est.net.flat_params.data)
    ws = train_workspace(est, n, "cuda", thr)
    ws.fill_(float("nan"))     # nothing the kernels do not write themselves may reach the result
    losses = loss_fwd_bwd(est, th.cuda(), xx.cuda(), tt.cuda(), ee.cuda(), w.cuda(), 0.0, grad, thr, workspace=ws)
    torch.cuda.synchronize()
    assert losses.shape == (n,) and torch.isfinite(losses).all() and torch.isfinite(grad).all()
    held_to_fp64("npse_envelope_loss_and_gradients", _id(cfg, size, cv), "loss", losses, l32, l64)
    blocks_held_to_fp64("npse_envelope_loss_and_gradients", _id(cfg, size, cv), est, grad, g32, g64)


def test_score_and_ode_fn_beyond_one_tile_per_workgroup():
    n = rows_of(CUS_PLUS_ONE_RAGGED)
    _, o64, est, theta, x, times, _ = make_npse_pair("ve", 5, 3, 100, 4, n=n)
    th = theta * 1.3
    with torch.no_grad():
        for what, xr, tr, xg, tg in (("rows", x, times, x.cuda(), times.cuda()),
                                     ("broadcast", x[:1], times[:1].expand(n), x[:1].cuda(), times[:1].cuda())):
            for fn, ofn in (("score", o64.score), ("ode_fn", o64.ode_fn)):
                ref = ofn(th.double(), xr.double(), tr.double())
                got = (est if fn == "score" else est.ode_fn)(th.cuda(), xg, tg)
                assert got.shape == (n, 5)
                assert dist(got, ref) <= 2e-5 * float(ref.abs().max()), (what, fn)


def test_sampler_with_given_noise_beyond_one_tile_per_workgroup():
    from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_fused, sample_sde_loop

    n = rows_of(CUS_PLUS_ONE_RAGGED)
    o32, o64, est, _, x, _, _ = make_npse_pair("ve", 3, 4, 48, 1)
    torch.manual_seed(9)
    ts = est.solve_schedule(4).cpu()       # 3 steps
    noise = torch.randn(4, n, 3)
    r32 = o32.sample_sde(x[:1], ts, noise, 1.0)
    r64 = o64.sample_sde(x[:1].double(), ts.double(), noise.double(), 1.0)
    fused = sample_sde_fused(est, n, x[:1].cuda(), ts.cuda(), 1.0, noise.cuda())
    loop = sample_sde_loop(est, n, x[:1].cuda(), ts.cuda(), 1.0, noise.cuda())
    assert fused.shape == (n, 3)
    cid = f"ve-D3-C4-H48-L1-n{size_id(CUS_PLUS_ONE_RAGGED)}"
    held_to_fp64("npse_envelope_sampler", cid, "fused", fused, r32, r64)
    held_to_fp64("npse_envelope_sampler", cid, "host_loop", loop, r32, r64)
