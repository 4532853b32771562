"""Cases, slot table, LDS image and the per-slot bound of the LRU envelope tests (tests/test_lru_envelope_cpu.py,
test_lru_envelope_gpu.py; also the gradient of tests/test_lru_embedding_gpu.py's test_parity).  Importable without a
GPU; no test functions here.

A case is the tuple of tests/test_lru_embedding_gpu.py: (T, B, input_dim, hidden_dim, state_dim, bidirectional,
num_blocks, aggregation).

The per-slot bound.  The flat gradient is cut into the slots different code writes: the input layer's weight and bias,
and per block log_nu, log_theta, B, C, D, log_gamma, gate weight, gate bias; the state-indexed ones (log_nu, log_theta,
log_gamma, B by row, C by column) once more into the forward (s < S) and the reversed (s >= S) half of a bidirectional
unit, whose adjoints are different sweeps of the kernel.  In every slot
    kernel error <= max(4 x eager error, 16 x 2^-24 x scale),
errors against the fp64 oracle, worst entry of the slot; factor and floor are those of tests/test_embedding_nets_gpu.py.
`scale` is the slot's largest entry of sum_b |g_b|, g_b the fp64 gradient of sequence b alone: an fp32 sum over the
batch is accurate relative to the sum of the magnitudes of its terms, not to a total they may cancel in.  It is max|ref|
at B = 1.  Batches above 17 repeat 17 distinct sequences and weight rows (x[b] = x17[b % 17]), so their oracle is 17
calls and a weighted sum."""
import math

import torch

from tests import lru_embedding_oracle as O
from tests import parity_log

ULP = 2.0**-24
LDS_LIMIT_BYTES = 160 * 1024
AGGREGATIONS = ("mean", "last_step")
DISTINCT = 17                                  # distinct sequences of a repeated batch
TILE = 16                                      # time steps of a tile, rows and columns of an MFMA tile
BLOCK_TENSORS = ("log_nu", "log_theta", "B", "C", "D", "log_gamma", "Wg", "bg")


def case_id(c):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def dims_of(case):
    """(input_dim, hidden_dim, state_dim, num_blocks, bidirectional, aggregation code): the module's `dims`"""
    _, _, I, H, S, bidir, blocks, agg = case
    return (I, H, S, blocks, int(bool(bidir)), AGGREGATIONS.index(agg))


# ---------------------------------------------------------------------------- the flat image, restated from the header
def tensor_table(dims):
    """[(name, offset, length)] of the flat fp32 image: input.W (H, I), input.b (H), then per block log_nu (S2),
    log_theta (S2), B (S2, H, 2), C (H, S2, 2), D (H), log_gamma (S2), Wg (H, H), bg (H)."""
    I, H, S, blocks, bidir, _ = dims
    S2 = S * (2 if bidir else 1)
    sizes = [("input.W", H * I), ("input.b", H)]
    for i in range(blocks):
        for name, n in zip(BLOCK_TENSORS, (S2, S2, S2 * H * 2, H * S2 * 2, H, S2, H * H, H)):
            sizes.append((f"b{i}.{name}", n))
    table, o = [], 0
    for name, n in sizes:
        table.append((name, o, n))
        o += n
    return table


def slot_table(dims):
    """[(name, index)]: the slots of the module docstring, `index` the slot's flat positions (int64).  log_nu,
    log_theta, log_gamma and B split into contiguous halves; C (H, S2, 2) splits by column, an index set."""
    I, H, S, blocks, bidir, _ = dims
    slots = []
    for name, o, n in tensor_table(dims):
        idx = torch.arange(o, o + n)
        kind = name.split(".")[-1]
        if not bidir or kind not in ("log_nu", "log_theta", "log_gamma", "B", "C"):
            slots.append((name, idx))
            continue
        if kind == "C":
            fwd = (torch.arange(n) // 2) % (2 * S) < S         # (h, s, c): s = (e // 2) % S2
        else:
            fwd = torch.arange(n) < n // 2                     # rows s < S of (S2, ...) come first
        slots.append((name + ".fwd", idx[fwd]))
        slots.append((name + ".rev", idx[~fwd]))
    return slots


def lds_floats(I, H, S2):
    """(backward, forward) LDS image in floats, from the formula of include/sbi_amd_lru.h"""
    weights = 2 * S2 + 4 * S2 * H + H * H + 2 * H
    forward_tiles = (TILE + 2) * 2 * S2 + 4 * TILE * H
    backward_tiles = TILE * 2 * S2 + 3 * TILE * H + TILE * I
    return weights + forward_tiles + backward_tiles, weights + forward_tiles


def fits(I, H, S2):
    return 4 * lds_floats(I, H, S2)[0] <= LDS_LIMIT_BYTES


def largest_hidden(I, S2):
    """the widest block of the envelope (H <= 128) whose backward image fits the LDS"""
    return max(H for H in range(1, 129) if fits(I, H, S2))


# ---------------------------------------------------------------------------------------------------------- the cases
BASE = (17, 3, 3, 20, 5, True, 2, "mean")


def vary(**kw):
    names = ("T", "B", "I", "H", "S", "bidir", "blocks", "agg")
    assert set(kw) <= set(names)
    return tuple(kw.get(n, v) for n, v in zip(names, BASE))


HIDDEN = [(vary(H=1), "one row / column / K step everywhere H is a GEMM dimension"),
          (vary(H=2), "K % 4 = 2, M and N below a tile"),
          (vary(H=3), "K % 4 = 3"),
          (vary(H=5), "K % 4 = 1, two K steps"),
          (vary(H=15), "one short of a tile, K % 4 = 3"),
          (vary(H=17), "one tile + 1: a second tile with one live row / column, K % 4 = 1"),
          (vary(H=18), "K % 4 = 2 past a tile"),
          (vary(H=19), "K % 4 = 3 past a tile"),
          (vary(H=50), "K % 4 = 2, four tiles the last with 2 live"),
          (vary(H=127, S=4), "eight tiles, the last one short, K % 4 = 3"),
          (vary(H=128, S=4), "the envelope's widest block: eight full tiles")]
STATES = [(vary(S=1), "one state lane; the reversed half starts at column 2"),
          (vary(S=2), "W2 = 8: two K steps over the states"),
          (vary(S=15), "W2 = 60: the state columns one pair short of four tiles"),
          (vary(S=16), "each half exactly two tiles of columns"),
          (vary(S=17), "each half two tiles + one state"),
          (vary(S=64), "S2 = 128 bidirectional: the envelope's most states, a full wave of state lanes"),
          (vary(S=65, bidir=False), "state lanes span two waves, the second holds one lane"),
          (vary(S=128, bidir=False), "S2 = 128 unidirectional: two full waves of state lanes")]
INPUTS = [(vary(I=i), why) for i, why in (
    (2, "N = 2 of dW_in"), (4, "one full K step of the input layer"), (5, "I % 4 = 1"),
    (16, "the XI tile and dW_in exactly one tile wide"), (17, "a second tile of dW_in with one live column"),
    (63, "one short of the envelope"), (64, "the envelope's widest input"))]
BLOCKS = [(vary(blocks=8), "the envelope's deepest stack, bidirectional"),
          (vary(blocks=8, bidir=False), "the envelope's deepest stack, unidirectional")]
# every T with both directions and both aggregations: (T, bidirectional), (T, aggregation) and (bidirectional,
# aggregation) are pairwise covered; last_step meets a full last tile (16, 32, 48) and a one-row last tile (17, 33, 49)
STEP_VALUES = (1, 2, 16, 17, 31, 32, 33, 48, 49)
STEPS = []
for _i, _T in enumerate(STEP_VALUES):
    STEPS.append((vary(T=_T, bidir=_i % 2 == 0, agg="mean"),
                  f"T = {_T}: {-(-_T // TILE)} tiles, {(_T - 1) % TILE + 1} rows in the last"))
    STEPS.append((vary(T=_T, bidir=_i % 2 == 1, agg="last_step"),
                  f"T = {_T}: the last step is row {(_T - 1) % TILE} of its tile"))
# repeated batches (x[b] = x17[b % 17]) around the 512-workgroup grid
BATCHES = [(vary(B=511, I=1, H=8, S=3), "one workgroup short of the grid"),
           (vary(B=512, I=1, H=8, S=3), "exactly the grid: every workgroup one sequence"),
           (vary(B=513, I=1, H=8, S=3), "the grid wraps: workgroup 0 adds a second sequence onto its partial"),
           (vary(B=1025, I=1, H=8, S=3), "workgroup 0 adds three sequences, the others two")]
CORNER_I64_S2 = 16
LDS_CORNERS = [(vary(T=33, B=2, H=128, S=17, bidir=False), "H = 128 at its last S2 = 17"),
               (vary(T=33, B=2, H=72, S=76, bidir=False), "H = 72 at its last S2 = 76, unidirectional"),
               (vary(T=33, B=2, H=72, S=38), "H = 72 at S2 = 76, bidirectional"),
               (vary(T=33, B=2, H=47, S=128, bidir=False), "S = 128 at its last H = 47"),
               (vary(T=33, B=2, I=64, H=largest_hidden(64, CORNER_I64_S2), S=CORNER_I64_S2 // 2),
                "I = 64 at the widest block that fits with S2 = 16")]
# (case, what is conditioned): T = 130 is 9 tiles, the last with 2 rows
CONDITIONING = [(vary(T=130, B=2), "radius"), (vary(T=130, B=2), "phase")]

GPU_CASES = HIDDEN + STATES + INPUTS + BLOCKS + STEPS + BATCHES + LDS_CORNERS + [(BASE, "the base case")]
# the C ABI with a pre-filled workspace: a partial last tile, then the grid wrap
ABI_CASES = [vary(T=37, B=5), vary(T=17, B=600)]
SMALL_NET = vary(T=37, B=5, H=8, S=3)          # the attribute-order test: this, the first LDS corner, this again
ALL_CASES = [c for c, _ in GPU_CASES] + [c for c, _ in CONDITIONING] + ABI_CASES + [SMALL_NET]


def condition(net, what):
    """|lambda| = 1 - 1e-3 in every state ("radius"), or every phase within 1e-3 of pi ("phase"), in every block"""
    with torch.no_grad():
        for blk in net.lru_blocks:
            u = blk.lru
            if what == "radius":
                u.log_nu.fill_(math.log(-math.log(1.0 - 1e-3)))
            else:
                n = u.log_theta.numel()
                u.log_theta.copy_(torch.log(math.pi + 1e-3 * torch.linspace(-1.0, 1.0, n + 2)[1:-1]))
    return net


def inputs(case, seed=0, conditioned=None):
    """(net on the host, x (B, T, I), wts (B, H), distinct): the recipe of tests/test_lru_embedding_gpu.py
    (`parity_inputs`) for min(B, 17) sequences, repeated to B"""
    from tests.test_lru_embedding_gpu import make_net, spread

    T, B, I, H = case[:4]
    n = min(B, DISTINCT)
    torch.manual_seed(seed)
    net = spread(make_net(case), seed)
    if conditioned:
        condition(net, conditioned)
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(n, T, I, generator=g) * 1.3 + 0.2
    wts = torch.randn(n, H, generator=g)
    rows = torch.arange(B) % n
    return net, x[rows].contiguous(), wts[rows].contiguous(), n


# ------------------------------------------------------------------------------------------------------- the oracle
def per_sequence(net, x, wts, distinct=None):
    """fp64 (features (B, H), flat gradient (P), sum_b |g_b| (P)) of loss = sum(wts * features), one oracle call per
    distinct sequence; rows b >= distinct repeat row b % distinct"""
    d = net.dims
    B = x.shape[0]
    n = B if distinct is None else distinct
    state = net.state_dict()
    features, grad, mag = [], 0.0, 0.0
    for b in range(n):
        count = len(range(b, B, n))
        _, f, g = O.reference(state, x[b:b + 1], wts[b:b + 1], d[2], bool(d[4]), AGGREGATIONS[d[5]], through="features")
        features.append(f)
        grad = grad + count * g
        mag = mag + count * g.abs()
    return torch.cat(features)[torch.arange(B) % n], grad, mag


# ---------------------------------------------------------------------------------------------------- the slot check
def slot_figures(dims, kernel, eager, ref, per_seq_abs):
    """{slot: dict(kernel_err, eager_err, scale, ratio, bound)}"""
    e_k = (kernel.detach().double().cpu() - ref).abs()
    e_e = (eager.detach().double().cpu() - ref).abs()
    out = {}
    for name, idx in slot_table(dims):
        k, e, scale = e_k[idx].max().item(), e_e[idx].max().item(), per_seq_abs[idx].max().item()
        ratio = k / e if e > 0 else float("inf") if k > 0 else 0.0
        out[name] = dict(kernel_err=k, eager_err=e, scale=scale, ratio=ratio, bound=max(4 * e, 16 * ULP * scale))
    return out


def slot_check(test, config, kernel, eager, ref, per_seq_abs, tag=""):
    """The bound of the module docstring in every slot of the flat gradient of case `config`.  Prints and records every
    slot before it asserts, and names every failing slot at once."""
    label = case_id(config) + (":" + tag if tag else "")
    P = sum(n for _, _, n in tensor_table(dims_of(config)))
    assert kernel.numel() == eager.numel() == ref.numel() == per_seq_abs.numel() == P
    figures = slot_figures(dims_of(config), kernel, eager, ref, per_seq_abs)
    for name, f in figures.items():
        print(f"{test}[{label}] {name}: kernel {f['kernel_err']:.3e} eager {f['eager_err']:.3e} "
              f"scale {f['scale']:.3e} bound {f['bound']:.3e} ratio {f['ratio']:.2f}")
    parity_log.record(test, label, **{name: {k: f[k] for k in ("kernel_err", "eager_err", "scale", "ratio")}
                                      for name, f in figures.items()})
    failing = {name: (f["kernel_err"], f["bound"]) for name, f in figures.items()
               if not f["kernel_err"] <= f["bound"]}
    if failing:
        raise AssertionError((label, failing))
    return figures
