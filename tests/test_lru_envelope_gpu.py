"""The lru_embed kernels over the edges of their envelope (include/sbi_amd_lru.h), one factor at a time around
(T, B, I, H, S, bidirectional, blocks, aggregation) = (17, 3, 3, 20, 5, yes, 2, mean); the table and the reason of every
case are in tests/lru_envelope.py.  Each case is one forward and backward of the module on the kernel route and on the
eager route (`kernel_route(x)[0]` asserted on both), against the fp64 oracle one sequence at a time:

* features: the whole-quantity bound of tests/test_lru_embedding_gpu.py (`check`);
* gradient: the per-slot bound of tests/lru_envelope.py (`slot_check`): in every slot of the flat gradient the kernel's
  worst error is at most max(4 x the eager route's, 16 x 2^-24 x max over the slot of sum_b |g_b|).

Besides the sizes: both conditioning extremes (|lambda| = 1 - 1e-3, phases within 1e-3 of pi) over nine tiles, the C ABI
on a workspace of exactly the stated size pre-filled with NaN and with zeros, and the dynamic-LDS attribute raised by
the largest image between two launches of a small one.  Measured figures per slot go to the parity artifact
(tests/parity_log.py; profiles/parity_lru_envelope.json).

Measured on the MI355X: every slot of every case passes.  At B <= 17 the kernel / eager ratio stays below 4 wherever the
eager error is above 1e-8 (worst: input.W 3.9, log_gamma.rev 3.9, Wg 3.8; log_theta.rev 7.6 at I = 4 under the floor).
At B >= 511 the floor decides: the kernel adds the workgroups' partials in one fp32 chain of up to 512 terms where torch
reduces pairwise, ratios 15.7 (D), 17.7 (bg), 24 (log_nu.fwd); the nearest any slot comes to its bound is D at B = 512
with 0.94 of the 16-ulp floor, then log_theta.rev 0.80 (I = 4) and log_theta 0.76 (T = 32, unidirectional)."""
import copy
import ctypes

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets import lru as L
from tests import lru_envelope as env
from tests.test_lru_embedding_gpu import both_routes, check, kernel_grad, run_both

pytestmark = pytest.mark.gpu


def parity(test, case, conditioned=None, tag=""):
    """one case on both routes against the oracle; returns (kernel-route module, x, wts, distinct, results)"""
    net, x, wts, n = env.inputs(case, conditioned=conditioned)
    features, grad, mag = env.per_sequence(net, x, wts, n)
    net, twin = both_routes(net)
    got = run_both(net, twin, x, wts)
    config = env.case_id(case) + (":" + tag if tag else "")
    check(test, config, "forward", got["kernel"][0], got["eager"][0], features)
    env.slot_check(test, case, got["kernel"][1], got["eager"][1], grad, mag, tag=tag)
    return net, x, wts, n, got


# ---- the dynamic-LDS attribute ---------------------------------------------------------------------------------------
# first in the module: the corner's image is the largest any launch has asked for so far, so this is the launch that
# raises the attribute
def test_a_small_image_before_and_after_the_largest_gives_the_same_bits():
    small, x, wts, _ = env.inputs(env.SMALL_NET)
    small = small.cuda()
    corner = env.LDS_CORNERS[0][0]
    assert (corner[3], corner[4], corner[5]) == (128, 17, False)

    def run_small():
        m = copy.deepcopy(small)
        assert m.kernel_route(x.cuda())[0]
        out = m.features(x.cuda())
        (out * wts.cuda()).sum().backward()
        return out.detach(), kernel_grad(m)

    before = run_small()
    parity("lru_envelope_lds_order", corner, tag="between_two_small_images")
    after = run_small()
    assert torch.isfinite(before[1]).all() and before[1].abs().max() > 0
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


@pytest.mark.parametrize("case", [c for c, _ in env.GPU_CASES if c[1] <= env.DISTINCT],
                         ids=[env.case_id(c) for c, _ in env.GPU_CASES if c[1] <= env.DISTINCT])
def test_parity_per_slot(case):
    parity("lru_envelope", case)


@pytest.mark.parametrize("case", [c for c, _ in env.BATCHES], ids=[env.case_id(c) for c, _ in env.BATCHES])
def test_parity_per_slot_around_the_grid_wrap(case):
    """repeated batches: besides the bounds, every row carries the bits of the same sequence run alone"""
    net, x, wts, n, got = parity("lru_envelope", case)
    with torch.no_grad():
        alone = net.features(x[:n].cuda())
    assert n == env.DISTINCT and torch.equal(got["kernel"][0].detach(), alone[torch.arange(case[1]) % n])


@pytest.mark.parametrize("case,what", env.CONDITIONING, ids=[w for _, w in env.CONDITIONING])
def test_parity_per_slot_at_the_conditioning_extremes(case, what):
    parity("lru_envelope_conditioning", case, conditioned=what, tag=what)


# ---- the C ABI on a pre-filled workspace -----------------------------------------------------------------------------
def abi_run(net, x, wts, fill):
    """sbi_amd_lru_forward and _backward on live tensors of exactly the stated sizes plus one sentinel float each,
    everything the calls write pre-filled with `fill`; (features, grad_params), sentinels asserted"""
    lib = _lib.load()
    cfg = L.lru_config(net.dims)
    flat = L.flat_image(net.kernel_parameters()).contiguous()
    B, T = x.shape[0], x.shape[1]
    stream = _lib.current_stream(x.device)

    def buffer(n):
        t = torch.full((n + 1,), fill, dtype=torch.float32, device=x.device)
        t[n] = float("nan")
        return t

    sizes = [int(lib.sbi_amd_lru_workspace_bytes(ctypes.byref(cfg), B, T, backward)) for backward in (0, 1)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes[0] < sizes[1]
    ws_f, ws_b = buffer(sizes[0] // 4), buffer(sizes[1] // 4)
    features, grad = buffer(B * net.dims[1]), buffer(flat.numel())
    _lib.check(lib.sbi_amd_lru_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), B, T, features.data_ptr(),
                                       ws_f.data_ptr(), stream), "lru_forward")
    _lib.check(lib.sbi_amd_lru_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), B, T, wts.data_ptr(),
                                        grad.data_ptr(), ws_b.data_ptr(), stream), "lru_backward")
    torch.cuda.synchronize()
    for name, t in (("forward workspace", ws_f), ("backward workspace", ws_b), ("features", features), ("grad", grad)):
        assert torch.isnan(t[-1]), name + ": the float behind the stated size was written"
    return features[:-1].view(B, net.dims[1]), grad[:-1]


@pytest.mark.parametrize("case", env.ABI_CASES, ids=[env.case_id(c) for c in env.ABI_CASES])
def test_the_c_abi_reads_only_what_it_wrote(case):
    net, x, wts, n = env.inputs(case)
    ref_features, ref_grad, mag = env.per_sequence(net, x, wts, n)
    net, twin = both_routes(net)
    xd, wd = x.cuda(), wts.cuda()
    assert net.kernel_route(xd)[0]
    from_nan = abi_run(net, xd, wd, float("nan"))
    from_zero = abi_run(net, xd, wd, 0.0)
    for a, b in zip(from_nan, from_zero):
        assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b)
    # the module (a workspace from the caching allocator) gives the same bits
    eager = run_both(net, twin, x, wts)
    assert torch.equal(eager["kernel"][0].detach(), from_nan[0]) and torch.equal(eager["kernel"][1], from_nan[1])
    check("lru_envelope_abi", env.case_id(case), "forward", from_nan[0], eager["eager"][0], ref_features)
    env.slot_check("lru_envelope_abi", case, from_nan[1], eager["eager"][1], ref_grad, mag, tag="nan_workspace")
