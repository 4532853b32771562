"""The ABC distances through `Distance` on device tensors against fp64: l1 / mse / l2 against the written formulas,
`mmd_distance` (one launch of the split kernel for all simulated sets) against tests/mmd_oracle.py within the 2e-6
absolute the README states for the MMD kernel, `wasserstein_distance` (the persistent Sinkhorn kernel, x_o never
repeated) against tests/abc_oracle.py within the project bound."""

import pytest
import torch

from sbi_amd.utils.metrics import Distance, mmd_distance, wasserstein_distance
from tests import abc_oracle, mmd_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    return dict(x_o=torch.randn(1, 3, generator=g), x=torch.randn(50, 3, generator=g),
                xs_o=torch.randn(6, 2, generator=g), xs=torch.randn(50, 5, 2, generator=g) + 0.3)


@pytest.mark.parametrize("batch_size", [-1, 7])
def test_pairwise_distances(data, batch_size):
    x_o, x = data["x_o"], data["x"]
    d64 = (x.double() - x_o.double())
    want = {"l1": d64.abs().mean(-1), "mse": (d64**2).mean(-1), "l2": (d64**2).sum(-1).sqrt()}
    for name, ref in want.items():
        got = Distance(name, batch_size=batch_size)(x_o.cuda(), x.cuda())
        assert got.is_cuda and got.shape == (50,)
        assert ((got.cpu().double() - ref).abs() <= 1e-5 * (1 + ref.abs())).all()
        assert torch.equal(got, Distance(name)(x_o.cuda(), x.cuda()))


@pytest.mark.parametrize("scale", [None, 0.7])
def test_mmd_distance(data, scale):
    xs_o, xs = data["xs_o"], data["xs"]
    kw = {} if scale is None else dict(scale=scale)
    got = Distance("mmd", distance_kwargs=kw)(xs_o.cuda(), xs.cuda())
    want = torch.tensor([mmd_oracle.unbiased_mmd_squared(xs_o, xs[b], scale) for b in range(50)], dtype=torch.float64)
    err = (got.cpu().double() - want).abs().max().item()
    print(f"mmd_distance scale={scale}: max abs err {err:.3e}")
    assert got.is_cuda and got.shape == (50,) and err <= 2e-6
    assert torch.equal(Distance("mmd", distance_kwargs=kw, batch_size=7)(xs_o.cuda(), xs.cuda()), got)
    assert torch.allclose(mmd_distance(xs_o, xs, **kw), got.cpu(), atol=2e-6, rtol=0)          # the host composition


def test_wasserstein_distance(data):
    xs_o, xs = data["xs_o"], data["xs"]
    kw = dict(epsilon=0.5, max_iter=1000, tol=1e-5)
    got = Distance("wasserstein", distance_kwargs=kw)(xs_o.cuda(), xs.cuda())
    a, b = torch.full((50, 6), 1 / 6), torch.full((50, 5), 1 / 5)
    cost = abc_oracle.squared_distances(xs_o.unsqueeze(0).expand(50, 6, 2), xs)
    _, _, w64, _ = abc_oracle.sinkhorn(cost, a, b, 0.5, 1000, 1e-5)
    assert got.is_cuda and ((got.cpu().double() - w64).abs() <= 1e-5 * (1 + w64.abs())).all()
    assert torch.equal(Distance("wasserstein", distance_kwargs=kw, batch_size=7)(xs_o.cuda(), xs.cuda()), got)
    host = wasserstein_distance(xs_o, xs, **kw)
    assert ((host.double() - w64).abs() <= 1e-5 * (1 + w64.abs())).all()


def test_shape_assertions_fire_with_the_reference_messages(data):
    with pytest.raises(AssertionError, match="simulated data needs batch dimension"):
        Distance("l2")(data["x_o"][0].cuda(), data["x"][0].cuda())
    with pytest.raises(AssertionError, match="simulated data needs batch dimension"):
        Distance("mmd")(data["xs_o"].cuda(), data["xs"][0].cuda())
    with pytest.raises(AssertionError):
        Distance("wasserstein")(data["xs_o"][0].cuda(), data["xs"].cuda())
    with pytest.warns(UserWarning, match="By default, we assume that `requires_iid_data=False`"):
        Distance(lambda a, b: (a - b).abs().sum(-1))
