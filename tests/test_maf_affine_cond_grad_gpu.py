"""d loss / d condition of the affine MAF's training pass (NLE ascends on it: theta is the condition there, and
rejection sampling and MAP run gradient ascent on the potential).  Compared with fp64 autograd of the oracle to the
relative bound tests/test_maf_affine_gpu.py holds d loss / d theta to (3e-4 of the largest entry)."""
import pytest
import torch

from sbi_amd.neural_nets.estimators.maf_affine_flow import maf_affine_loss_fwd_bwd
from tests.parity_log import record
from tests.test_maf_affine_gpu import CONFIGS, _ids, maf_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_training_pass_returns_the_condition_gradient(cfg):
    oracle, est, theta_d, x_d = maf_pair(**cfg)
    n = 333      # ragged: not a multiple of the 16-row wave tile
    theta, x = theta_d[:n], x_d[:n]
    w = torch.linspace(0.5, 1.5, n) / n
    oracle.double().zero_grad()
    xr = x.double().clone().requires_grad_(True)
    (oracle.loss(theta.double(), xr) * w.double()).sum().backward()
    gx_ref = xr.grad.clone()
    oracle.float()
    grad = torch.empty_like(est.net.flat_params.data)
    gx = torch.full((n, cfg["C"]), float("nan"), device="cuda")
    maf_affine_loss_fwd_bwd(est.net, theta.cuda(), x.cuda(), w.cuda(), 0.0, grad, grad_x_out=gx)
    assert torch.isfinite(gx).all()
    e = (gx.cpu().double() - gx_ref).abs().max().item() / gx_ref.abs().max().item()
    print(f"d/dx rel {e:.3e}")
    record("maf_affine_train_grad_condition", _ids(cfg), rel_grad_x_err=e)
    assert e <= 3e-4
    # the other outputs do not depend on whether it is asked for, and a second call gives the same bits
    grad0, gx2 = torch.empty_like(grad), torch.full_like(gx, float("nan"))
    maf_affine_loss_fwd_bwd(est.net, theta.cuda(), x.cuda(), w.cuda(), 0.0, grad0)
    maf_affine_loss_fwd_bwd(est.net, theta.cuda(), x.cuda(), w.cuda(), 0.0, grad, grad_x_out=gx2)
    assert torch.equal(grad, grad0) and torch.equal(gx, gx2)


def test_autograd_reaches_the_condition_and_broadcast_conditions_are_summed():
    oracle, est, theta_d, x_d = maf_pair(D=3, C=4, num_transforms=2)
    theta = theta_d[:50].cuda()
    x = x_d[:50].cuda().requires_grad_(True)
    est.log_prob(theta, condition=x).sum().backward()
    xr = x_d[:50].double().requires_grad_(True)
    oracle.double().log_prob(theta_d[:50].double(), xr)[0].sum().backward()
    oracle.float()
    assert (x.grad.cpu().double() - xr.grad).abs().max() <= 3e-4 * xr.grad.abs().max()
    # NLE's potential: several inputs (trials) against every condition row
    trials = theta_d[100:103].cuda()
    c = x_d[:7].cuda().requires_grad_(True)
    est.log_prob(trials.unsqueeze(1).expand(-1, 7, -1), condition=c).sum().backward()
    cr = x_d[:7].double().requires_grad_(True)
    tr = theta_d[100:103].double()
    oracle.double()
    sum(oracle.log_prob(tr[i : i + 1].expand(7, -1), cr)[0].sum() for i in range(3)).backward()
    oracle.float()
    assert (c.grad.cpu().double() - cr.grad).abs().max() <= 3e-4 * cr.grad.abs().max()
    # the kernel refuses a broadcast condition for this output
    with pytest.raises(ValueError):
        maf_affine_loss_fwd_bwd(est.net, theta, x_d[:1].cuda(), None, 1.0, torch.empty_like(est.net.flat_params.data),
                                grad_x_out=torch.empty(1, 4, device="cuda"))
