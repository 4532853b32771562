"""The tr_embed kernels over the edges of their envelope (include/sbi_amd_tr.h), one factor at a time around
(B, T, (F, H, KV), I, L) = (3, 17, (36, 6, 3), 17, 2), rotary, causal, gelu, scalar input; the table and the reason of
every case are in tests/transformer_envelope.py.  Each case is one forward and backward of the module on the kernel
route and on the eager route (`kernel_route(x)[0]` asserted on both), against the fp64 oracle one sequence at a time:

* output: the whole-quantity bound of tests/test_transformer_embedding_gpu.py (`check`);
* gradient: the per-slot bound of tests/transformer_envelope.py (`slot_check`): in every one of the 9 L + 5 slots of
  the flat gradient the kernel's worst error is at most max(4 x the eager route's, 16 x 2^-24 x max over the slot of
  sum_b |g_b|);
* the kernel-route forward under `torch.no_grad()` (h in place, one block's buffers) gives the bits of the training
  forward (the stash layout).

Besides the sizes: dropout with the exported masks in two more configurations (every key with grouped heads past one
64-key step; p = 0.9 over three key steps), the dynamic-LDS limits raised by the largest images between two launches
of a small net, and the C ABI on buffers of exactly the stated sizes pre-filled with NaN and with zeros, with packed
and with strided inputs.  Measured figures per slot go to the parity artifact (tests/parity_log.py;
profiles/parity_transformer_envelope.json).

Measured on the MI355X: every slot of every case passes (1356 slot figures).  Kernel / eager ratios where the eager
error is above 1e-8 stay below 4 except under the floor: aggregator.bias 15.0 and norm.weight / layernorm weights up to
7.9 at T = 4096 (eager errors of 1e-7 against scales near 1), v rows 6.3.  Nearest their bound: layers.1
input_layernorm.weight at T = 4096, every key, hd = 4 with 0.98 of the 16-ulp floor; the k rows of layer 0 at 64 query
heads on one key / value head with 0.87 of 4 x eager (ratio 3.47); the v rows of layer 1 at T = 2046, every key, 0.90
of the floor; the k rows of layer 0 at I = 512, 0.75.  Outputs: at most 0.41 of their bound (T = 4096, every key).

What the first run of this table found, and what was changed in the kernels for it (csrc/tr_embed_kernel.h):
* B = 1365, 1366 and the 257-tile features case: aggregator.weight at 1.08 - 1.33 x its bound.  `tr_final_wgrad_kernel`
  added the B terms in one fp32 chain; it and `tr_reduce_kernel` (T = 2047: down_proj 1.19 x, k rows 1.06 x) now use the
  file's four chains.
* 64 query heads on one key / value head: k rows of layer 0 at 1.13 x.  `tr_attn_bwd_dkv_kernel` added the group's heads
  in one chain; four chains now.
* Rows with one key (T = 1; query 0 of every causal row): the q and k rows of qkv_proj have gradient exactly 0, and the
  eager route gives 0, but `dq` carried dP - D = rounding of two differently ordered sums (up to 1.7e-5 at B = 40,
  F = 128).  D = rowsum(dO o O) also put the rounding of the stored O, relative to |dO| |O|, into every dS of a row.  D
  is now sum_k P dP as the P-weighted mean of dP around key 0's: exactly dP for a one-key row, and relative to the
  spread of dP otherwise.  (sum_k P dP without the division by sum_k P failed the peaked case and L = 8: the common
  factor of the rebuilt P, from the rounding of lse, then multiplies D.)
* test_parity's (1, 2, (16, 1, 1), 17, 3, positional, every key, relu, features) under the per-slot bound: two tokens with
  nearly uniform attention, dS = P (dP - D) a tenth of dP and dP = dO . v sixteen products that cancel; with the new D
  the k rows of layer 0 still stood at 1.30 x their floor from the fp32 rounding of dP alone.  Both attention-backward
  kernels now sum dP in fp64 and round once (`tr_dot_wide`): 0.96 of the floor.
"""
import copy
import ctypes

import pytest
import torch

from sbi_amd import _lib
from sbi_amd.neural_nets import TransformerEmbedding
from sbi_amd.neural_nets.embedding_nets import transformer as TR
from tests import transformer_embedding_oracle as O
from tests import transformer_envelope as env
from tests.test_transformer_embedding_gpu import both_routes, check, masks_of, run_both, spread

pytestmark = pytest.mark.gpu


def ids(cases):
    return [env.case_id(c) for c in cases]


def parity(test, case, tag=""):
    """one case on both routes against the oracle, and the inference forward against the training forward; returns
    (kernel-route module, x, wts, distinct, results)"""
    net, x, wts, n = env.inputs(case)
    out, grad, mag = env.per_sequence(net, x, wts, case, n)
    others = []
    if case[7] == "relu":
        near, others = env.kink_references(net, x, wts, case, n)
        print(f"{test}[{env.case_id(case)}] pre-activations within the margin of a kink: {near}")
    net, twin = both_routes(net)
    got = run_both(net, twin, x, wts)
    config = env.case_id(case) + (":" + tag if tag else "")
    check(test, config, "forward", got["kernel"][0], got["eager"][0], out, [o[0] for o in others])
    env.slot_check(test, case, got["kernel"][1], got["eager"][1], grad, mag, tag=tag, others=[o[1] for o in others])
    with torch.no_grad():
        assert net.kernel_route(x.cuda())[0]
        inference = net(x.cuda())
    assert torch.isfinite(inference).all() and torch.equal(inference, got["kernel"][0].detach())
    return net, x, wts, n, got


# ---- the dynamic-LDS attributes --------------------------------------------------------------------------------------
# First in the module: no other test of the suite asks for more than 48 KiB in tr_tail_bwd_kernel (the largest elsewhere
# is F = 96, I = 256, 39.9 KB), so the F = 128, I = 512 case below is the first launch that raises that kernel's limit.
def test_a_small_net_before_and_after_the_largest_images_gives_the_same_bits():
    small, x, wts, _ = env.inputs(env.SMALL_NET)
    small = small.cuda()
    wide, long = env.INTER_LDS[4][0], env.LONG_ROWS[4][0]
    assert env.lds_bytes(wide)[3] > 64 * env.KIB and env.lds_bytes(long)[4] > 64 * env.KIB
    assert max(env.lds_bytes(env.SMALL_NET)) < 48 * env.KIB

    def run_small():
        m = copy.deepcopy(small)
        assert m.kernel_route(x.cuda())[0]
        out = m(x.cuda())
        (out * wts.cuda()).sum().backward()
        return out.detach(), O.flat_grad(m).clone()

    before = run_small()
    parity("tr_envelope_lds_order", wide, tag="between_two_small_nets")
    parity("tr_envelope_lds_order", long, tag="between_two_small_nets")
    after = run_small()
    assert torch.isfinite(before[1]).all() and before[1].abs().max() > 0
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


CASES = [c for c, _ in env.GPU_CASES if c != env.PEAKED]


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_parity_per_slot(case):
    parity("tr_envelope", case)


def test_parity_per_slot_with_peaked_attention():
    """q and k rows times 3: the probabilities rebuilt as exp(S - lse) are limited by the rounding of lse"""
    net, x, _, _ = env.inputs(env.PEAKED)
    peaks = env.max_score(net, x, env.PEAKED)
    print(f"tr_envelope_peaked: fp64 max|S| per layer {peaks}")
    assert all(env.PEAKED_SCORES[0] <= s <= env.PEAKED_SCORES[1] for s in peaks)
    parity("tr_envelope_peaked", env.PEAKED)


@pytest.mark.parametrize("case", [c for c, _ in env.PARTITION], ids=ids([c for c, _ in env.PARTITION]))
def test_parity_per_slot_around_the_weight_gradient_partition(case):
    """repeated batches: besides the bounds, every row carries the bits of the same sequence run alone"""
    net, x, wts, n, got = parity("tr_envelope", case)
    with torch.no_grad():
        alone = torch.cat([net(x[b:b + 1].cuda()) for b in range(n)])
    assert n == env.DISTINCT and torch.equal(got["kernel"][0].detach(), alone[torch.arange(case[0]) % n])


# ---- dropout with the exported masks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,p", env.DROPOUT, ids=[f"{env.case_id(c)}-p{p}" for c, p in env.DROPOUT])
def test_dropout_parity_with_the_exported_masks(case, p):
    """forward and backward use the masks the mask kernel exports: the eager formula and the oracle are fed them"""
    B, T = case[0], case[1]
    F, H, KV, hd, I, L, E = env.sizes_of(case)
    torch.manual_seed(5)
    net = spread(TransformerEmbedding(**dict(env.kwargs_of(case), attention_dropout=p)), 5).cuda().train()
    net.dropout_seed = 1234567890123
    g = torch.Generator().manual_seed(7)
    x, wts = (torch.randn(B, T, generator=g) * 1.3 + 0.2).cuda(), torch.randn(B, E, generator=g).cuda()
    assert net.kernel_route(x) == (True, "kernel")
    out = net(x)
    (out * wts).sum().backward()
    grad = O.flat_grad(net).clone()
    keep = masks_of(net, B, T)
    if p == 0.9:
        for mask in keep:
            n = mask.numel()
            assert mask.shape == (B, H, T, T)
            rate, sd = mask.float().mean().item(), (p * (1 - p) / n) ** 0.5
            print(f"keep rate at p={p}: {rate:.5f} (1 - p = {1 - p:.1f}, 5 sd = {5 * sd:.5f})")
            assert abs(rate - (1 - p)) <= 5 * sd
    params = [q.detach().clone().requires_grad_(True) for q in net.parameters()]
    eager = TR.tr_functional(x, params, dict(net.config, head_dim=hd), keep)
    eager_grad = torch.cat([t.reshape(-1) for t in torch.autograd.grad((eager * wts).sum(), params)])
    ref_out, ref_grad, mag = env.per_sequence(net, x, wts, case, keep_masks=keep)
    config = f"{env.case_id(case)}:p{p}"
    check("tr_envelope_dropout", config, "forward", out, eager, ref_out)
    env.slot_check("tr_envelope_dropout", case, grad, eager_grad, ref_grad, mag, tag=f"p{p}")
    net.eval()
    with torch.no_grad():
        assert (net(x) - out).abs().max() > 1e-3          # the masks did something


# ---- the C ABI on pre-filled buffers, packed and strided -------------------------------------------------------------
SENTINEL = -12345.0


def abi_run(net, x, wts, fill):
    """sbi_amd_tr_forward with training = 0 and = 1 and sbi_amd_tr_backward on live tensors of exactly the stated sizes
    plus one sentinel float each, everything the calls write pre-filled with `fill`; x (B, T) or (B, T, F), any batch
    and time strides.  (out of the inference call, out of the training call, grad_params), sentinels asserted."""
    lib = _lib.load()
    cfg = net.kernel_config(x.ndim == 2)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).contiguous()
    B, T, E = x.shape[0], x.shape[1], int(cfg.final_emb_dimension)
    stream = _lib.current_stream(x.device)
    assert x.ndim == 2 or x.stride(2) == 1

    def buffer(n):
        t = torch.full((n + 1,), fill, dtype=torch.float32, device=x.device)
        t[n] = SENTINEL
        return t

    sizes = [TR.workspace_bytes(cfg, B, T, training) for training in (False, True)]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes[0] < sizes[1]
    assert flat.numel() == TR.param_count(cfg)[0]
    ws = [buffer(s // 4) for s in sizes]
    outs = [buffer(B * E), buffer(B * E)]
    grad = buffer(flat.numel())
    for training in (0, 1):
        _lib.check(lib.sbi_amd_tr_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                          B, T, 0.0, 0, outs[training].data_ptr(), ws[training].data_ptr(), training,
                                          stream), "tr_forward")
    _lib.check(lib.sbi_amd_tr_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                       B, T, 0.0, 0, wts.data_ptr(), grad.data_ptr(), ws[1].data_ptr(), stream),
               "tr_backward")
    torch.cuda.synchronize()
    for name, t in (("inference workspace", ws[0]), ("training workspace", ws[1]), ("inference out", outs[0]),
                    ("training out", outs[1]), ("grad_params", grad)):
        assert t[-1].item() == SENTINEL, name + ": the float behind the stated size was written"
    return outs[0][:-1].view(B, E), outs[1][:-1].view(B, E), grad[:-1]


def strided(x):
    """x as a view of a larger NaN-filled tensor: non-trivial batch and time strides, NaN in every gap"""
    if x.ndim == 2:
        B, T = x.shape
        big = torch.full((B, T + 3, 2), float("nan"), device=x.device)
        view = big[:, 1:T + 1, 0]
    else:
        B, T, F = x.shape
        big = torch.full((B, T + 2, F + 5), float("nan"), device=x.device)
        view = big[:, 1:T + 1, :F]
    view.copy_(x)
    assert not view.is_contiguous() and view.stride(0) != x.stride(0) and view.stride(1) != x.stride(1)
    assert torch.equal(view, x) and torch.isnan(big).sum() == big.numel() - x.numel()
    return view


@pytest.mark.parametrize("case", env.ABI_CASES, ids=ids(env.ABI_CASES))
def test_the_c_abi_reads_only_what_it_wrote_and_follows_the_strides(case):
    net, x, wts, n = env.inputs(case)
    ref_out, ref_grad, mag = env.per_sequence(net, x, wts, case, n)
    net, twin = both_routes(net)
    xd, wd = x.cuda(), wts.cuda()
    assert net.kernel_route(xd)[0]
    from_nan = abi_run(net, xd, wd, float("nan"))
    from_zero = abi_run(net, xd, wd, 0.0)
    for a, b in zip(from_nan, from_zero):
        assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b)
    assert torch.equal(from_nan[0], from_nan[1])                   # inference and training forward
    # the module (a workspace from the caching allocator) gives the same bits
    module = run_both(net, twin, x, wts)
    assert torch.equal(module["kernel"][0].detach(), from_nan[1]) and torch.equal(module["kernel"][1], from_nan[2])
    check("tr_envelope_abi", env.case_id(case), "forward", from_nan[1], module["eager"][0], ref_out)
    env.slot_check("tr_envelope_abi", case, from_nan[2], module["eager"][1], ref_grad, mag, tag="nan_workspace")
    # x through non-trivial strides: tr_input_kernel and the scalar-projection gradient of tr_qkv_bwd_kernel read it
    view = strided(xd)
    from_view = abi_run(net, view, wd, float("nan"))
    for a, b in zip(from_view, from_nan):
        assert torch.equal(a, b)
