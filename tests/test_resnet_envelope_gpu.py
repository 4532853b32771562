"""The resnet_embed kernels over the edges of their plan (include/sbi_amd_resnet.h): the row counts either side of every
change of row tile and of split count, widths that need more than one weight panel with a short last one at every tile
size, both corners of the envelope at 64 blocks; the table and the reason of every case are in
tests/resnet_envelope.py.  Each case is one forward and backward of the module on the kernel route and on the eager
route (`kernel_route(x)[0]` asserted on both), against the fp64 oracle:

* trunk and module output: the whole-quantity bound of tests/test_resnet_embedding_gpu.py (`check`);
* gradient: the per-slot bound of tests/resnet_envelope.py (`slot_check`): in every one of the 6 n_blocks (+ 2) + 6
  tensors of the flat gradient the kernel's worst error is at most max(4 x the eager route's, 16 x 2^-24 x the slot's
  largest sum_r |g_r|);
* the trunk under `torch.no_grad()` (inference: the tiles cover `rows`, no stash) has the bits of the trunk of the
  training forward (the tiles cover Rp, the stash is written).

Besides the table: a net with a dead hidden unit and one with a dead residual stream, whose gradients are exactly zero
where the oracle's are; the bitwise conditions of tests/test_resnet_embedding_gpu.py at widths 65 / 113 / 97 and at the
first calls of the 32-row and 64-row tiles; the calling conventions the module hides (strided x, a stride-0 grad_out,
frozen parameters); and the C ABI called directly on buffers of exactly the stated sizes pre-filled with NaN and with
zeros, up to 131 072 rows, which only the ABI reaches.  Measured figures per slot go to the parity artifact
(tests/parity_log.py; profiles/parity_resnet_envelope.json).

Measured on the MI355X: every slot of every case passes (1226 slot figures), without a change to the kernels.  Nearest
their bounds, all at (1, 128, 128, 64, 128): final.2.weight 0.54 of the 16-ulp floor, blocks.63.f.4.weight 0.43 and
final.4.weight 0.42 of 4 x eager (ratios 1.73, 1.66).  From 4097 rows on no slot passes 0.045 of its bound; the
kernels' weight gradients are 3 to 8 times nearer the oracle than eager's there (ratios 0.12 .. 0.35).  Ratios above 4
only far under the floor: blocks.1.f.2.bias 5.35 at 131 072 rows (0.001 of its bound), 5.18 at 4096 rows.  Outputs: at
most 0.52 of their bound (the one-row case).
"""
import copy
import ctypes
import functools

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets import resnet as RN
from tests import resnet_embedding_oracle as O
from tests import resnet_envelope as env
from tests.test_resnet_embedding_gpu import both_routes, check, make, spread

pytestmark = pytest.mark.gpu

CASES = [c for c, _ in env.GPU_CASES]


def ids(cases):
    return [env.case_id(c) for c in cases]


def run(m, x, wts, kernel):
    """(trunk under no_grad, trunk of the training forward, out, flat gradient) of one route"""
    xd = x.cuda()
    assert m.kernel_route(xd)[0] == kernel, m.kernel_route(xd)
    m.zero_grad()
    with torch.no_grad():
        inference = m.trunk(xd)
    trunk = m.trunk(xd)
    out = m.final(trunk)
    (out * wts.cuda()).sum().backward()
    return inference, trunk.detach(), out.detach(), O.flat_grad(m).clone()


def parity(test, case, drawn, tag="", exact_zero=()):
    """one net on both routes against the oracle, and the inference trunk against the training one; returns the
    kernel-route module and what it gave"""
    net, x, wts, near, ref, scale = drawn[:6]
    print(f"{test}[{env.case_id(case)}] rows within the margin of a kink: {len(near)} of {x.shape[0]}")
    assert 3 * len(near) <= x.shape[0], (len(near), x.shape[0])
    net, twin = both_routes(net)
    kernel, eager = run(net, x, wts, True), run(twin, x, wts, False)
    config = env.case_id(case) + (":" + tag if tag else "")
    check(test, config, "trunk", kernel[1], eager[1], ref[0])
    check(test, config, "forward", kernel[2], eager[2], ref[1])
    env.slot_check(test, case, kernel[3], eager[3], ref[2], scale, tag=tag, exact_zero=exact_zero)
    assert torch.isfinite(kernel[0]).all() and torch.equal(kernel[0], kernel[1])
    return net, kernel


# ---- parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_parity_per_slot(case):
    parity("resnet_envelope", case, env.draw(case))


@pytest.mark.parametrize("variant", ["unit", "stream"])
def test_a_dead_unit_and_a_dead_stream_give_exact_zeros(variant):
    """blocks.0.f.0.bias[j] = -1e3: row j of that weight, entry j of the bias and column j of blocks.0.f.2.weight are
    exactly zero; all of blocks.1.f.4.bias = -1e3: every trunk tensor of blocks 0, 1 and the initial Linear is"""
    drawn = env.dead_unit_net(variant)
    parity("resnet_envelope_dead", env.DEAD_UNIT, drawn, tag=variant, exact_zero=drawn[6])


# ---- bitwise conditions, at widths with short last panels ------------------------------------------------------------
BITWISE = dict(c_in=65, c_out=6, n_blocks=2, c_internal=113, c_hidden_final=24,
               construct_mapping_kwargs={"c_hidden": 97})
TILE_EDGES = ((4097, 32), (16385, 64))          # the first calls of the 32-row and of the 64-row tile


@functools.lru_cache(maxsize=None)
def bitwise_net():
    torch.manual_seed(9)
    return spread(make(BITWISE), 9).cuda()


@functools.lru_cache(maxsize=None)
def bitwise_rows(rows):
    g = torch.Generator().manual_seed(31)
    x = torch.randn(16385, 65, generator=g) * 1.3
    wts = torch.randn(16385, 6, generator=g)
    return x[:rows].cuda(), wts[:rows].cuda()


def gradient_of(net, loss, **kw):
    net.zero_grad()
    loss.backward(**kw)
    g = O.flat_grad(net).clone()
    assert torch.isfinite(g).all() and g.abs().max() > 0
    return g


def test_the_first_rows_of_a_large_call_carry_the_bits_of_the_same_rows_alone():
    net = bitwise_net()
    with torch.no_grad():
        x = bitwise_rows(200)[0]
        assert net.kernel_route(x)[0] and RN.plan(net.kernel_config(), 200)[1] == 16
        alone = net.trunk(x)
        assert torch.isfinite(alone).all() and alone.abs().max() > 0
        for rows, tile in TILE_EDGES:
            big = bitwise_rows(rows)[0]
            assert net.kernel_route(big)[0] and RN.plan(net.kernel_config(), rows)[1] == tile
            assert torch.equal(big[:200], x) and torch.equal(net.trunk(big)[:200], alone), rows
    # ... and so do those of the training forward, whose tiles cover Rp
    big = bitwise_rows(4097)[0]
    assert torch.equal(net.trunk(big)[:200].detach(), alone)


def test_two_backward_calls_at_the_first_64_row_tile_give_identical_gradients():
    net = bitwise_net()
    x, wts = bitwise_rows(16385)
    assert net.kernel_route(x)[0] and RN.plan(net.kernel_config(), 16385)[1:] == (64, [138240, 138240], 17)
    grads = [gradient_of(net, (net(x) * wts).sum()) for _ in range(2)]
    assert torch.equal(grads[0], grads[1])


def test_a_second_backward_on_one_graph_gives_the_same_bits():
    """`backward(retain_graph=True)` twice: the stash is read, not consumed"""
    net = bitwise_net()
    x, wts = bitwise_rows(1025)
    assert net.kernel_route(x)[0]
    loss = (net(x) * wts).sum()
    first = gradient_of(net, loss, retain_graph=True)
    second = gradient_of(net, loss)
    assert torch.equal(first, second)
    assert torch.equal(first, gradient_of(net, (net(x) * wts).sum()))


def test_two_graphs_alive_at_once_give_the_bits_of_each_alone():
    net = bitwise_net()
    (xa, wa), (xb, wb) = bitwise_rows(1025), bitwise_rows(200)
    xb, wb = xb.flip(0).contiguous(), wb.flip(0).contiguous()
    alone = [gradient_of(net, (net(x) * w).sum()) for x, w in ((xa, wa), (xb, wb))]
    loss_a = (net(xa) * wa).sum()
    loss_b = (net(xb) * wb).sum()
    together = [gradient_of(net, loss_a), gradient_of(net, loss_b)]
    assert not torch.equal(alone[0], alone[1])
    assert torch.equal(together[0], alone[0]) and torch.equal(together[1], alone[1])


# ---- calling conventions through the module --------------------------------------------------------------------------
def test_a_strided_input_gives_the_bits_of_its_contiguous_copy():
    net = bitwise_net()
    x, wts = bitwise_rows(400)
    transposed = x.t().contiguous().t()
    views = {"transposed": (transposed, wts), "every second row": (x[::2], wts[::2].contiguous())}
    assert not transposed.is_contiguous() and torch.equal(transposed, x) and not x[::2].is_contiguous()
    for name, (view, w) in views.items():
        got = []
        for v in (view, view.contiguous()):
            assert net.kernel_route(v)[0]
            with torch.no_grad():
                trunk = net.trunk(v)
            got.append((trunk, gradient_of(net, (net(v) * w).sum())))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), name


def test_a_stride_0_grad_out_gives_the_bits_of_a_dense_one():
    net = bitwise_net()
    x = bitwise_rows(200)[0]
    assert net.kernel_route(x)[0]
    expanded = gradient_of(net, net.trunk(x).sum())
    dense = gradient_of(net, (net.trunk(x) * torch.ones(200, 113, device="cuda")).sum())
    assert torch.equal(expanded, dense)
    assert all(p.grad is None for p in net.final.parameters())


def test_frozen_parameters_get_no_gradient_and_the_others_the_same_bits():
    net = copy.deepcopy(bitwise_net())
    x, wts = bitwise_rows(200)
    free = gradient_of(net, (net(x) * wts).sum())
    frozen = list(net.initial.parameters()) + list(net.blocks[0].parameters())
    assert len(frozen) == 8
    for p in frozen:
        p.requires_grad_(False)
    assert net.kernel_route(x)[0]
    net.zero_grad()
    for p in net.parameters():
        p.grad = None
    (net(x) * wts).sum().backward()
    assert all(p.grad is None for p in frozen)
    sizes = env.sizes_of_kwargs(BITWISE)
    named = dict(net.named_parameters())
    seen = 0
    for name, lo, hi in env.slot_table(sizes):
        if name.startswith(("initial.", "blocks.0.")):
            continue
        assert torch.equal(named[name].grad.reshape(-1), free[lo:hi]), name
        seen += 1
    assert seen == 6 + 6


# ---- the C ABI on pre-filled buffers ---------------------------------------------------------------------------------
SENTINEL = -12345.0


def abi_run(net, x, wts, fill):
    """sbi_amd_resnet_forward with training = 0 and = 1 and sbi_amd_resnet_backward on tensors of exactly the stated
    sizes plus one sentinel float each, everything the calls write pre-filled with `fill`.  grad_out is torch's, from
    the head on the training call's trunk.  (trunk of the inference call, trunk of the training call, module output,
    flat gradient in state_dict order), sentinels asserted."""
    lib = _lib.load()
    cfg = net.kernel_config()
    rows, ci = x.shape[0], int(cfg.c_internal)
    params = net.kernel_parameters()
    flat = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
    stream = _lib.current_stream(x.device)
    assert x.is_contiguous() and flat.numel() == RN.param_count(cfg)[0]

    def buffer(n):
        t = torch.full((n + 1,), fill, dtype=torch.float32, device=x.device)
        t[n] = SENTINEL
        return t

    sizes = [RN.workspace_bytes(cfg, rows, training) for training in (False, True)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes[0] < sizes[1]
    ws = [buffer(s // 4) for s in sizes]
    outs = [buffer(rows * ci), buffer(rows * ci)]
    grad = buffer(flat.numel())
    for training in (0, 1):
        _lib.check(lib.sbi_amd_resnet_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), rows,
                                              outs[training].data_ptr(), ws[training].data_ptr(), training, stream),
                   "resnet_forward")
    trunk = outs[1][:-1].view(rows, ci).clone().requires_grad_(True)
    net.zero_grad()
    out = net.final(trunk)
    (out * wts).sum().backward()
    grad_out = trunk.grad.contiguous()
    _lib.check(lib.sbi_amd_resnet_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), rows, grad_out.data_ptr(),
                                           grad.data_ptr(), ws[1].data_ptr(), stream), "resnet_backward")
    torch.cuda.synchronize()
    for name, t in (("inference workspace", ws[0]), ("training workspace", ws[1]), ("inference out", outs[0]),
                    ("training out", outs[1]), ("grad_params", grad)):
        assert t[-1].item() == SENTINEL, name + ": the float behind the stated size was written"
    # the flat gradient in state_dict order: initial.*, the head (torch's), the blocks
    n_init = sum(p.numel() for p in net.initial.parameters())
    head = torch.cat([p.grad.reshape(-1) for p in net.final.parameters()])
    whole = torch.cat([grad[:n_init], head, grad[n_init:-1]])
    return outs[0][:-1].view(rows, ci), outs[1][:-1].view(rows, ci), out.detach(), whole, grad[:-1].clone()


@pytest.mark.parametrize("case", env.ABI_CASES, ids=ids(env.ABI_CASES))
def test_the_c_abi_stays_inside_its_buffers_and_reads_only_what_it_wrote(case):
    net, x, wts, near, ref, scale = env.draw(case)
    assert 3 * len(near) <= case[0]
    net, twin = both_routes(net)
    xd, wd = x.cuda(), wts.cuda()
    from_nan = abi_run(net, xd, wd, float("nan"))
    from_zero = abi_run(net, xd, wd, 0.0)
    for a, b in zip(from_nan, from_zero):
        assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b)
    assert torch.equal(from_nan[0], from_nan[1])                   # inference and training forward
    routed = net.kernel_route(xd)[0]
    assert routed == (case[0] < RN.MAX_ROWS_TRAINING)
    if routed:    # the module (a workspace from the caching allocator) gives the same bits
        module = run(net, x, wts, True)
        trunk_grad = torch.cat([p.grad.reshape(-1) for p in net.kernel_parameters()])
        assert torch.equal(module[1], from_nan[1]) and torch.equal(trunk_grad, from_nan[4])
    eager = run(twin, x, wts, False)                               # the forced route runs at any row count
    config = env.case_id(case)
    check("resnet_envelope_abi", config, "trunk", from_nan[1], eager[1], ref[0])
    check("resnet_envelope_abi", config, "forward", from_nan[2], eager[2], ref[1])
    env.slot_check("resnet_envelope_abi", case, from_nan[3], eager[3], ref[2], scale, tag="nan_workspace")
