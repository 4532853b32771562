"""Cases, slot table, plan restatement and the per-slot bound of the ResNetEmbedding1D envelope tests
(tests/test_resnet_envelope_cpu.py, test_resnet_envelope_gpu.py; also the gradient of
tests/test_resnet_embedding_gpu.py's test_parity and recorded 1D cases).  Importable without a GPU; no test functions
here.

A case is the tuple of tests/test_resnet_embedding_gpu.py: (rows, c_internal, c_hidden, n_blocks, c_in or "id"), with
that module's head (c_hidden_final 16, c_out 5) and its recipe (`spread`, seed 0, x = 1.3 randn + 0.2).

The per-slot bound.  The flat gradient (state_dict order) is cut into the tensors different launches write:
initial.weight and .bias when c_in != c_internal, per block f.0.weight, f.0.bias, f.2.weight, f.2.bias, f.4.weight,
f.4.bias (include/sbi_amd_resnet.h), and the six head tensors final.{0,2,4}.{weight,bias}, which torch computes on
both routes from the kernels' trunk bits: 6 n_blocks (+ 2) + 6 slots.  In every slot
    kernel error <= max(4 x eager error, 16 x 2^-24 x scale),
errors against the fp64 oracle, worst entry of the slot; factor and floor are those of tests/test_embedding_nets_gpu.py.
`scale` is the slot's largest entry of sum_r |g_r|, g_r the fp64 gradient of row r alone: an fp32 sum over the rows is
accurate relative to the sum of the magnitudes of its terms, not to a total they may cancel in.  For a Linear with
input A (rows, K) and output-side delta D (rows, N) the gradient of row r alone is the outer product D[r]^T A[r], so
sum_r |g_r| = |D|^T |A| for the weight and the column sums of |D| for the bias: no per-row oracle calls.

Kinks: the rule of tests/test_resnet_embedding_gpu.py.  The rows `near_kink_rows` returns, decided by the oracle alone,
get grad_out = 0; no case may zero more than one third of its rows.

The plan is restated from the header's text and `rn_plan_shape` (sbi_amd/csrc/resnet_embed_kernel.h): P(v) pads to 16,
Rp to 64; the row tile is 16 up to 16 x 256 rows, 32 up to 64 x 256, then 64; weight panels have 64 rows, 32 at tile
64; S0 = min(ceil(Rp / 1024), 64), chunk = 64 ceil(Rp / 64 / S0), S = ceil(Rp / chunk)."""
import functools

import torch

from tests import parity_log
from tests import resnet_embedding_oracle as O

ULP = 2.0**-24
GRID = 256                                     # workgroups of the row-tile kernels (RN_GRID)
MAX_SPLITS = 64                                # SBI_AMD_RESNET_MAX_SPLITS
SPLIT_ROWS = 1024                              # splits = ceil(Rp / 1024) before the cap
HEAD = (16, 5)                                 # (c_hidden_final, c_out) of every case of the table


def case_id(c):
    return "-".join(str(v) for v in c)


def sizes_of(case, head=HEAD):
    """(c_in, c_internal, c_hidden, n_blocks, c_hidden_final, c_out)"""
    _, ci, ch, nb, cin = case
    return (ci if cin == "id" else cin, ci, ch, nb) + tuple(head)


def sizes_of_kwargs(kwargs):
    """the same of the constructor's keywords (defaults of ResNetEmbedding1D)"""
    ci = kwargs.get("c_internal", 128)
    mapping = kwargs.get("construct_mapping_kwargs") or {"c_hidden": 128}
    return (kwargs["c_in"], ci, mapping["c_hidden"], kwargs.get("n_blocks", 20), kwargs.get("c_hidden_final", 1000),
            kwargs["c_out"])


def kwargs_of(case):
    cin, ci, ch, nb, hf, cout = sizes_of(case)
    return dict(c_in=cin, c_out=cout, n_blocks=nb, c_internal=ci, c_hidden_final=hf,
                construct_mapping_kwargs={"c_hidden": ch})


def pad16(v):
    return -(-v // 16) * 16


# ---------------------------------------------------------------------------- the flat image, restated from the header
def trunk_table(sizes):
    """[(name, rows, columns)] of the kernels' flat image in its own order: initial.* when c_in != c_internal, then per
    block f.0.weight (c_hidden, c_internal), f.0.bias, f.2.weight (c_hidden, c_hidden), f.2.bias, f.4.weight
    (c_internal, c_hidden), f.4.bias.  A vector has columns 0."""
    cin, ci, ch, nb, _, _ = sizes
    shapes = [("initial.weight", ci, cin), ("initial.bias", ci, 0)] if cin != ci else []
    for b in range(nb):
        pre = f"blocks.{b}.f."
        shapes += [(pre + "0.weight", ch, ci), (pre + "0.bias", ch, 0), (pre + "2.weight", ch, ch),
                   (pre + "2.bias", ch, 0), (pre + "4.weight", ci, ch), (pre + "4.bias", ci, 0)]
    return shapes


def head_table(sizes):
    _, ci, _, _, hf, cout = sizes
    return [("final.0.weight", hf, ci), ("final.0.bias", hf, 0), ("final.2.weight", hf, hf), ("final.2.bias", hf, 0),
            ("final.4.weight", cout, hf), ("final.4.bias", cout, 0)]


def tensor_table(sizes):
    """[(name, offset, rows, columns)] in the order of `O.flat_grad` and of the module's state_dict: the module
    registers `initial`, `final`, then `blocks`, so the head lies between the initial Linear and block 0 there (the
    kernels' own image has no head: `trunk_table`)."""
    trunk = trunk_table(sizes)
    n_init = 2 if sizes[0] != sizes[1] else 0
    table, o = [], 0
    for name, rows, cols in trunk[:n_init] + head_table(sizes) + trunk[n_init:]:
        table.append((name, o, rows, cols))
        o += rows * max(cols, 1)
    return table


def param_count(sizes):
    name, o, rows, cols = tensor_table(sizes)[-1]
    return o + rows * max(cols, 1)


def slot_table(sizes):
    """[(name, start, stop)]: one slot per tensor, contiguous ranges of the flat gradient"""
    return [(name, o, o + rows * max(cols, 1)) for name, o, rows, cols in tensor_table(sizes)]


def slot_of(sizes, name):
    """(offset, rows, columns) of one tensor"""
    return {n: (o, r, c) for n, o, r, c in tensor_table(sizes)}[name]


# --------------------------------------------------------------------------------------- the plan, from the header
def plan_of(case):
    """the plan of a training call of `case`, restated: Rp, tile, panel_rows, panels {K: (count, rows of the last)} for
    the padded K of every streamed matrix (CN, CI, CH), tiles (of the training forward and the delta pass: they cover
    Rp), tiles_per_workgroup, real_rows_last_tile (of the inference forward: its tiles cover rows), S, chunk,
    last_split, lds_bytes, workspace_floats (inference, training)"""
    rows = case[0]
    cin, ci, ch, nb, _, _ = sizes_of(case)
    CN, CI, CH = pad16(cin), pad16(ci), pad16(ch)
    Rp = -(-rows // 64) * 64
    tile = 16 if rows <= 16 * GRID else 32 if rows <= 64 * GRID else 64
    panel = 32 if tile == 64 else 64
    widths = {"CI": CI, "CH": CH}
    if cin != ci:
        widths["CN"] = CN
    panels = {k: (-(-v // panel), v - (-(-v // panel) - 1) * panel) for k, v in widths.items()}
    tiles = Rp // tile
    S0 = min(-(-Rp // SPLIT_ROWS), MAX_SPLITS)
    chunk = -(-(Rp // 64) // S0) * 64
    S = -(-Rp // chunk)
    has_init = cin != ci
    PI = ci * cin + ci if has_init else 0
    PB = 2 * ch * ci + ch * ch + 2 * ch + ci
    image = (CN * CI + CI if has_init else 0) + nb * (4 * CI * CH + 2 * CH * CH + 2 * CH + CI)
    training = image + (nb + 1) * Rp * CI + 2 * Rp * CI + 4 * Rp * CH + (S * max(PB, PI) if S > 1 else 0)
    return dict(Rp=Rp, tile=tile, panel_rows=panel, panels=panels, widths=widths, tiles=tiles,
                tiles_per_workgroup=-(-tiles // GRID), real_rows_last_tile=rows - (-(-rows // tile) - 1) * tile,
                S=S, chunk=chunk, last_split=Rp - (S - 1) * chunk, lds_bytes=4 * (3 * tile * 132 + 2 * panel * 144),
                workspace_floats=(image, training), trunk_params=PI + nb * PB)


# ---------------------------------------------------------------------------------------------------------- the cases
GPU_CASES = [
    ((4096, 5, 3, 2, 2), "256 tiles of 16: tile 16 fills the grid exactly; 4 splits of 1024"),
    ((4097, 113, 97, 2, 65), "the first tile-32 call; CI 128, CH 112 = 64 + 48, CN 80 = 64 + 16: short last panels"),
    ((16384, 33, 65, 2, "id"), "512 tiles of 32, two per workgroup; CI 48, CH 80 = 64 + 16"),
    ((16385, 97, 33, 2, 17), "the first tile-64 call: 257 tiles, the last with one real row; panels of 32: "
                             "CI 112 = 3 x 32 + 16, CH 48 = 32 + 16; 17 splits, the last of 64 rows"),
    ((16385, 128, 128, 1, "id"), "tile 64 with all 8 column tiles of a wave live; four full panels"),
    ((1024, 15, 31, 2, 3), "one split"),
    ((1025, 15, 31, 2, 3), "two splits: chunk 576, then a short split of 512"),
    ((2048, 17, 4, 3, "id"), "two splits of 1024"),
    ((2049, 17, 4, 3, "id"), "three splits of 704"),
    ((65535, 3, 5, 2, 2), "the last row count the module sends to the kernels: 64 splits, a 64-term chain in "
                          "rn_reduce_kernel"),
    ((64, 127, 112, 2, 113), "CI 128, CH 112, CN 128 at tile 16"),
    ((63, 112, 113, 2, 127), "CI 112, CH 128, CN 128"),
    ((65, 64, 65, 3, 63), "CI 64: one full panel; CH 80: a 16-row last panel; CN 64"),
    ((16, 65, 64, 3, "id"), "CI 80, CH 64, no initial Linear"),
    ((17, 80, 81, 2, 79), "CI 80, CH 96, CN 80"),
    ((1, 128, 128, 64, 128), "the widest and deepest trunk of the envelope on one row"),
    ((2, 1, 1, 64, "id"), "the narrowest trunk at the deepest"),
]
ABI_CASES = [(200, 50, 17, 3, 10), (1025, 15, 31, 2, 3), (65537, 3, 5, 2, 2), (131072, 3, 5, 2, 2)]
DEAD_UNIT = (33, 17, 20, 3, 7)                 # the dead-unit net
DEAD_UNIT_J = 11
SEEDED_ROWS = (1025, 15, 31, 2, 3)             # the seeded row defects (CPU)
SEEDED_DEEP = (33, 16, 16, 64, "id")           # the seeded relative defect (CPU)
SCALE_CASE = (9, 6, 5, 2, 3)                   # the outer-product scale against per-row autograd (CPU)
ALL_CASES = list(dict.fromkeys([c for c, _ in GPU_CASES] + ABI_CASES + [DEAD_UNIT, SEEDED_DEEP, SCALE_CASE]))


def build(case):
    """(net on the host, x): the recipe of tests/test_resnet_embedding_gpu.py's `draw`, seed 0"""
    from tests.test_resnet_embedding_gpu import make, spread

    kw = kwargs_of(case)
    torch.manual_seed(0)
    net = spread(make(kw), 0)
    g = torch.Generator().manual_seed(1000)
    x = torch.randn(case[0], kw["c_in"], generator=g) * 1.3 + 0.2
    wts = torch.randn(case[0], kw["c_out"], generator=g)
    return net, x, wts


def oracle(net, x, wts):
    """(near-kink rows, wts with those rows zeroed, (trunk, out, grad) in fp64, scale): everything the oracle decides"""
    sd = net.state_dict()
    near = O.near_kink_rows(sd, x, {})
    wts = wts.clone()
    wts[near] = 0
    trunk, out, grad, operands = O.reference_with_operands(sd, x, wts, {})
    return near, wts, (trunk, out, grad), scale_of(sd, operands)


@functools.lru_cache(maxsize=None)
def draw(case):
    """(net, x, wts with the near-kink rows zeroed, those rows, the oracle's (trunk, out, grad), scale)"""
    net, x, wts = build(case)
    near, wts, ref, scale = oracle(net, x, wts)
    return net, x, wts, near, ref, scale


def dead_unit_net(variant):
    """the DEAD_UNIT net with blocks.0.f.0.bias[j] = -1e3 ("unit") or all of blocks.1.f.4.bias = -1e3 ("stream"), its
    inputs and oracle as `draw`, and the ranges that are exactly zero on every route as (label, start, stop, step)"""
    net, x, wts = build(DEAD_UNIT)
    sizes = sizes_of(DEAD_UNIT)
    j = DEAD_UNIT_J
    with torch.no_grad():
        if variant == "unit":
            net.blocks[0].f[0].bias[j] = -1e3
        else:
            net.blocks[1].f[4].bias.fill_(-1e3)
    zero = []
    if variant == "unit":
        o, rows, cols = slot_of(sizes, "blocks.0.f.0.weight")
        zero.append((f"blocks.0.f.0.weight row {j}", o + j * cols, o + (j + 1) * cols, 1))
        o, rows, cols = slot_of(sizes, "blocks.0.f.0.bias")
        zero.append((f"blocks.0.f.0.bias entry {j}", o + j, o + j + 1, 1))
        o, rows, cols = slot_of(sizes, "blocks.0.f.2.weight")
        zero.append((f"blocks.0.f.2.weight column {j}", o + j, o + rows * cols, cols))
    else:
        for name, lo, hi in slot_table(sizes):
            if name.startswith(("initial.", "blocks.0.", "blocks.1.")):
                zero.append((name, lo, hi, 1))
    near, wts, ref, scale = oracle(net, x, wts)
    return net, x, wts, near, ref, scale, zero


# ------------------------------------------------------------------------------------------------------- the scale
def scale_of(state_dict, operands):
    """sum_r |g_r| over the flat gradient in state_dict order, from the oracle's (A, D) of every Linear"""
    parts = []
    for key in state_dict:
        name, kind = key.rsplit(".", 1)
        a, d = operands[name]
        parts.append((d.abs().T @ a.abs() if kind == "weight" else d.abs().sum(0)).reshape(-1))
    return torch.cat(parts)


# ---------------------------------------------------------------------------------------------------- the slot check
def worst(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


def flat_bound(eager, ref):
    """the bound of tests/test_resnet_embedding_gpu.py's `check` on the whole flat gradient, restated"""
    return max(4 * worst(eager, ref), 16 * ULP * ref.abs().max().item())


def slot_figures(sizes, kernel, eager, ref, scale):
    """{slot: dict(kernel_err, eager_err, scale, ratio, bound)}"""
    e_k = (kernel.detach().double().cpu() - ref).abs()
    e_e = (eager.detach().double().cpu() - ref).abs()
    out = {}
    for name, lo, hi in slot_table(sizes):
        k, e, s = e_k[lo:hi].max().item(), e_e[lo:hi].max().item(), scale[lo:hi].max().item()
        ratio = k / e if e > 0 else float("inf") if k > 0 else 0.0
        out[name] = dict(kernel_err=k, eager_err=e, scale=s, ratio=ratio, bound=max(4 * e, 16 * ULP * s))
    return out


def slot_check(test, case, kernel, eager, ref, scale, tag="", exact_zero=()):
    """The bound of the module docstring in every slot of the flat gradient of `case`.  Prints and records every slot
    before it asserts, and names every failing slot at once.  `exact_zero`: (label, start, stop, step) ranges of the
    flat gradient that have to be exactly 0.0 on both routes.  `case`: a case tuple, or (label, sizes) of a net that is
    not in the table."""
    if isinstance(case[1], tuple):
        label, sizes = case
    else:
        label, sizes = case_id(case), sizes_of(case)
    label += ":" + tag if tag else ""
    P = param_count(sizes)
    assert kernel.numel() == eager.numel() == ref.numel() == scale.numel() == P, (kernel.numel(), P)
    figures = slot_figures(sizes, kernel, eager, ref, scale)
    for name, f in figures.items():
        print(f"{test}[{label}] {name}: kernel {f['kernel_err']:.3e} eager {f['eager_err']:.3e} "
              f"scale {f['scale']:.3e} bound {f['bound']:.3e} ratio {f['ratio']:.2f}")
    parity_log.record(test, label, **{name: {k: f[k] for k in ("kernel_err", "eager_err", "scale", "ratio")}
                                      for name, f in figures.items()})
    failing = {name: (f["kernel_err"], f["bound"]) for name, f in figures.items()
               if not f["kernel_err"] <= f["bound"]}
    for what, lo, hi, step in exact_zero:
        for route, g in (("kernel", kernel), ("eager", eager)):
            largest = g[lo:hi:step].detach().abs().max().item()
            if not largest == 0.0:
                failing[f"{what} ({route} route, not exactly zero)"] = (largest, 0.0)
    if failing:
        raise AssertionError((label, failing))
    return figures
