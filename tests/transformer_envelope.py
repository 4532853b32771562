"""Cases, slot table, LDS images and the per-slot bound of the TransformerEmbedding envelope tests
(tests/test_transformer_envelope_cpu.py, test_transformer_envelope_gpu.py; also the gradient of
tests/test_transformer_embedding_gpu.py's test_parity and golden series test).  Importable without a GPU; no test
functions here.

A case is the tuple of tests/test_transformer_embedding_gpu.py, (B, T, (F, heads, kv heads), I, L, pos_emb, is_causal,
activation, input), optionally followed by one tuple of (name, value) pairs: the constructor's `final_emb_dimension`,
`rms_norm_eps`, `pos_emb_base`, and what `inputs` does to the draw (`seed`, `zero_sequence`, `peaked`).

The per-slot bound.  The flat gradient (state_dict order, include/sbi_amd_tr.h) is cut into the slots different code
writes: scalar_projection.weight and .bias; per layer o_proj, the q, k and v rows of qkv_proj, the gate and the up rows
of gate_up_proj, down_proj and both layernorm weights; norm.weight, aggregator.weight and .bias: 9 L + 5 slots.  In
every slot
    kernel error <= max(4 x eager error, 16 x 2^-24 x scale),
errors against the fp64 oracle, worst entry of the slot; factor and floor are those of tests/test_embedding_nets_gpu.py.
`scale` is the slot's largest entry of sum_b |g_b|, g_b the fp64 gradient of sequence b alone: an fp32 sum over the
batch is accurate relative to the sum of the magnitudes of its terms, not to a total they may cancel in.  It is max|ref|
at B = 1.  Batches above 17 repeat 17 distinct sequences and weight rows (x[b] = x17[b % 17]), so their oracle is 17
calls and a weighted sum.  For a (B, T, F) input the two scalar-projection slots are exactly zero on both routes."""
import torch

from tests import parity_log
from tests import transformer_embedding_oracle as O

ULP = 2.0**-24
KIB = 1024
LDS_LIMIT_BYTES = 160 * KIB
DISTINCT = 17                                  # distinct sequences of a repeated batch
TOK = 8                                        # tokens of a tile (SBI_AMD_TR_TOK)
WAVES = 4                                      # attention rows of a workgroup
MAX_PARTIALS = 256                             # SBI_AMD_TR_MAX_PARTIALS
KEY_STEP = 64                                  # keys one wave takes per step
KWARG_EXTRAS = ("final_emb_dimension", "rms_norm_eps", "pos_emb_base")
INPUT_EXTRAS = ("seed", "zero_sequence", "peaked")
LDS_NAMES = ("qkv", "attention", "tail", "tail_backward", "attention_backward", "qkv_backward")


def extras_of(case):
    return dict(case[9]) if len(case) > 9 else {}


def case_id(c):
    parts = ["x".join(str(u) for u in v) if isinstance(v, tuple) else str(v) for v in c[:9]]
    return "-".join(parts + [f"{k}={v}" for k, v in (c[9] if len(c) > 9 else ())])


def kwargs_of(case):
    """the constructor's keywords: those of tests/test_transformer_embedding_gpu.py's `kwargs_of`, and the extras"""
    _, _, (F, H, KV), inter, layers, pos, causal, act, _ = case[:9]
    kw = dict(feature_space_dim=F, num_attention_heads=H, num_key_value_heads=KV, intermediate_size=inter,
              num_hidden_layers=layers, pos_emb=pos, is_causal=causal, mlp_activation=act)
    kw.update({k: v for k, v in extras_of(case).items() if k in KWARG_EXTRAS})
    return kw


def sizes_of(case):
    """(F, H, KV, hd, I, L, E)"""
    (F, H, KV), I, L = case[2], case[3], case[4]
    return F, H, KV, F // H, I, L, extras_of(case).get("final_emb_dimension", F // 2)


def sizes_of_kwargs(kwargs):
    """(F, H, KV, hd, I, L, E) of the constructor's keywords"""
    cfg = O.full_config(kwargs)
    F = cfg["feature_space_dim"]
    E = cfg["final_emb_dimension"] if cfg["final_emb_dimension"] is not None else F // 2
    return (F, cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["intermediate_size"],
            cfg["num_hidden_layers"], E)


# ---------------------------------------------------------------------------- the flat image, restated from the header
def tensor_table(sizes):
    """[(name, offset, rows, columns)] of the flat fp32 image: scalar_projection.weight (F, 1), .bias (F); per layer
    self_attn.o_proj.weight (F, F), self_attn.qkv_proj.weight (OP, F), ffn.gate_up_proj.weight (2 I, F),
    ffn.down_proj.weight (F, I), input_layernorm.weight (F), post_attention_layernorm.weight (F); norm.weight (F),
    aggregator.weight (E, F), aggregator.bias (E).  A vector has columns 0."""
    F, H, KV, hd, I, L, E = sizes
    OP = (H + 2 * KV) * hd
    shapes = [("scalar_projection.weight", F, 1), ("scalar_projection.bias", F, 0)]
    for l in range(L):
        pre = f"layers.{l}."
        shapes += [(pre + "self_attn.o_proj.weight", F, F), (pre + "self_attn.qkv_proj.weight", OP, F),
                   (pre + "ffn.gate_up_proj.weight", 2 * I, F), (pre + "ffn.down_proj.weight", F, I),
                   (pre + "input_layernorm.weight", F, 0), (pre + "post_attention_layernorm.weight", F, 0)]
    shapes += [("norm.weight", F, 0), ("aggregator.weight", E, F), ("aggregator.bias", E, 0)]
    table, o = [], 0
    for name, rows, cols in shapes:
        table.append((name, o, rows, cols))
        o += rows * max(cols, 1)
    return table


def param_count(sizes):
    name, o, rows, cols = tensor_table(sizes)[-1]
    return o + rows * max(cols, 1)


def slot_table(sizes):
    """[(name, start, stop)]: the 9 L + 5 slots of the module docstring, contiguous ranges of the flat image.  qkv_proj
    splits by rows into q [0, H hd), k [H hd, (H + KV) hd) and v; gate_up_proj into its gate rows [0, I) and up rows."""
    F, H, KV, hd, I, L, E = sizes
    slots = []
    for name, o, rows, cols in tensor_table(sizes):
        width = max(cols, 1)
        if name.endswith("qkv_proj.weight"):
            cuts = (("q", 0, H * hd), ("k", H * hd, (H + KV) * hd), ("v", (H + KV) * hd, (H + 2 * KV) * hd))
        elif name.endswith("gate_up_proj.weight"):
            cuts = (("gate", 0, I), ("up", I, 2 * I))
        else:
            cuts = ((None, 0, rows),)
        for part, r0, r1 in cuts:
            slots.append((name if part is None else f"{name}.{part}", o + r0 * width, o + r1 * width))
    return slots


# -------------------------------------------------------------------------------- the LDS images, from the header
def lds_floats(F, H, KV, hd, I, T):
    """the six images in floats, in the plan's order (LDS_NAMES)"""
    OP = (H + 2 * KV) * hd
    return (TOK * (F + OP) + TOK, WAVES * (T + hd), TOK * (3 * F + 2 * I) + TOK, TOK * (5 * F + 3 * I) + 2 * TOK,
            WAVES * (2 * T + 2 * hd), TOK * (4 * F + OP) + 2 * TOK)


def lds_bytes(case):
    F, H, KV, hd, I, _, _ = sizes_of(case)
    return tuple(4 * n for n in lds_floats(F, H, KV, hd, I, case[1]))


def tail_backward_bytes(F, I):
    return 4 * lds_floats(F, 1, 1, 2, I, 1)[3]


def attention_backward_bytes(T, hd):
    return 4 * lds_floats(hd, 1, 1, hd, 1, T)[4]


def last_inter_within(F, limit_bytes):
    """the largest intermediate_size of the envelope (1..512) whose tail-backward image is at most `limit_bytes`"""
    return max(I for I in range(1, 513) if tail_backward_bytes(F, I) <= limit_bytes)


def last_steps_within(hd, limit_bytes):
    """the largest T of the envelope (1..4096) whose attention-backward image is at most `limit_bytes`"""
    return max(T for T in range(1, 4097) if attention_backward_bytes(T, hd) <= limit_bytes)


def partition(B, T):
    """(tiles, per, G) of the weight-gradient partition: per = ceil(tiles / 256), G = ceil(tiles / per)"""
    tiles = -(-B * T // TOK)
    per = -(-tiles // MAX_PARTIALS)
    return tiles, per, -(-tiles // per)


# ---------------------------------------------------------------------------------------------------------- the cases
BASE = (3, 17, (36, 6, 3), 17, 2, "rotary", True, "gelu", "scalar")
NAMES = ("B", "T", "heads", "I", "L", "pos", "causal", "act", "input")
POS = ("rotary", "positional", "none")


def vary(**kw):
    assert set(kw) <= set(NAMES) | set(KWARG_EXTRAS) | set(INPUT_EXTRAS), kw
    extras = tuple((k, kw[k]) for k in KWARG_EXTRAS + INPUT_EXTRAS if k in kw)
    return tuple(kw.get(n, v) for n, v in zip(NAMES, BASE)) + ((extras,) if extras else ())


INTER = [(vary(I=1), "one gate and one up row; K = 1 of the down product: only the remainder loop runs"),
         (vary(I=2), "K % 4 = 2 of tr_tile_linear (down) and of tr_tile_linear_t (J = 2 I = 4)"),
         (vary(I=3), "K % 4 = 3"),
         (vary(I=5), "K % 4 = 1 past one full step"),
         (vary(I=511), "one short of the envelope, K % 4 = 3"),
         (vary(I=512), "the envelope's widest feed-forward block")]
# F = 128: the tail-backward image 8 (5 F + 3 I) + 16 floats around the default dynamic-LDS limit and around 64 KiB
WIDE = dict(B=2, T=9, heads=(128, 2, 2))
I48, I64 = last_inter_within(128, 48 * KIB), last_inter_within(128, 64 * KIB)
INTER_LDS = [(vary(I=I48, **WIDE), "the last tail-backward image within 48 KiB: the limit is not raised"),
             (vary(I=I48 + 1, **WIDE), "the first tail-backward image over 48 KiB: the limit has to be raised"),
             (vary(I=I64, **WIDE), "the last tail-backward image within 64 KiB"),
             (vary(I=I64 + 1, **WIDE), "the first tail-backward image over 64 KiB"),
             (vary(I=512, **WIDE), "the largest tail-backward image of the envelope; tr_tile_wgrad walks 2 I F = "
                                   "131072 elements per tile")]
FINAL = [(vary(final_emb_dimension=1), "E = 1: one output thread, a one-term stride-F dot in the backward"),
         (vary(final_emb_dimension=2), "E = 2"),
         (vary(final_emb_dimension=35), "E = F - 1"),
         (vary(final_emb_dimension=36), "E = F"),
         (vary(heads=(128, 2, 2), final_emb_dimension=128), "E = F = 128: every thread of the 128-thread blocks live")]
LAYERS = [(vary(L=1), "one layer: only the last query carries dO"),
          (vary(L=8), "the envelope's deepest stack")]
HEADS = [(vary(heads=(2, 1, 1)), "F = 2: the narrowest model, one head of two columns"),
         (vary(heads=(4, 2, 1)), "F = 4, hd = 2, both heads share one key / value head"),
         (vary(heads=(128, 64, 1)), "hd = 2, 64 query heads on one key / value head"),
         (vary(heads=(128, 2, 1)), "hd = 64: a full wave of columns, two heads share"),
         (vary(heads=(126, 3, 3)), "hd = 42, F % 4 = 2")]
STEP_VALUES = (7, 8, 9, 63, 64, 65, 127, 128, 129)
STEPS = [(vary(T=_T, causal=_i % 2 == 0, pos=POS[_i % 3]),
          f"T = {_T}: {-(-_T // KEY_STEP)} key steps, {-(-3 * _T // TOK)} tiles, the last with {(3 * _T - 1) % TOK + 1}")
         for _i, _T in enumerate(STEP_VALUES)]
# F = 4, hd = 2: the attention-backward image 4 (2 T + 2 hd) floats at exactly 64 KiB and the first over, then T = 4096
LONG = dict(B=1, heads=(4, 2, 1), I=4, L=2)
T64 = last_steps_within(2, 64 * KIB)
LONG_ROWS = [(vary(T=T64, **LONG), "attention backward exactly 64 KiB, causal rotary"),
             (vary(T=T64, causal=False, pos="positional", **LONG), "attention backward exactly 64 KiB, every key"),
             (vary(T=T64 + 1, **LONG), "the first attention-backward image over 64 KiB, causal rotary"),
             (vary(T=T64 + 1, causal=False, pos="positional", **LONG), "the first over 64 KiB, every key"),
             (vary(T=4096, **LONG), "the longest row with two layers: every query carries dO in layer 0"),
             (vary(T=4096, B=1, heads=(4, 1, 1), I=4, L=2, causal=False, pos="positional"),
              "hd = 4, every key: angles up to 4095 rad through sincosf")]
# repeated batches (x[b] = x17[b % 17]) around the 256 weight-gradient workgroups
PART = dict(T=3, heads=(12, 6, 6), I=4, L=2)
PARTITION = [(vary(B=682, **PART), "256 tiles: per = 1, every workgroup one tile"),
             (vary(B=683, **PART), "257 tiles: per = 2, G = 129, the last workgroup owns one tile holding one token"),
             (vary(B=1365, **PART), "512 tiles: per = 2, G = 256, every workgroup two tiles"),
             (vary(B=1366, **PART), "513 tiles: per = 3, G = 171")]
SCALARS = [(vary(rms_norm_eps=1e-2), "an epsilon that matters next to mean(h^2)"),
           (vary(pos_emb_base=100.0), "another div_term buffer"),
           (vary(input="features", zero_sequence=1), "features input, sequence 1 all zero: 1 / sqrt(eps) rows")]
RELU = [(vary(B=2, T=9, I=1, act="relu"), "relu, one unit"),
        (vary(B=2, T=9, I=512, act="relu"), "relu, the widest block")]
PEAKED = vary(peaked=3.0)                       # the q and k rows of every qkv_proj times 3
PEAKED_SCORES = (30.0, 100.0)                   # the oracle's max|S| has to lie here

GPU_CASES = (INTER + INTER_LDS + FINAL + LAYERS + HEADS + STEPS + LONG_ROWS + SCALARS + RELU
             + [(BASE, "the base case"), (PEAKED, "peaked attention: exp(S - lse) is limited by the rounding of lse")])
SEEDED = (3, 65, (72, 4, 4), 64, 3, "positional", False, "gelu", "features")       # the seeded-defect case (CPU)
ABI_CASES = [vary(B=5, T=37), PARTITION[1][0], vary(B=5, T=37, input="features"),
             vary(B=683, input="features", **PART)]
SMALL_NET = vary(B=5, T=37, heads=(12, 6, 6), I=4)     # the attribute-order test
DROPOUT = [(vary(B=4, T=65, heads=(64, 4, 1), causal=False, pos="positional"), 0.5),
           (vary(B=4, T=129), 0.9)]
ALL_CASES = ([c for c, _ in GPU_CASES + PARTITION] + ABI_CASES + [SMALL_NET, SEEDED] + [c for c, _ in DROPOUT])
ALL_CASES = list(dict.fromkeys(ALL_CASES))


def inputs(case):
    """(net on the host in eval mode, x (B, T) or (B, T, F), wts (B, E), distinct): the recipe of
    tests/test_transformer_embedding_gpu.py (`draw`) for min(B, 17) sequences, repeated to B"""
    from sbi_amd.neural_nets import TransformerEmbedding
    from tests.test_transformer_embedding_gpu import spread

    B, T = case[0], case[1]
    F, H, KV, hd, I, L, E = sizes_of(case)
    extras = extras_of(case)
    seed = extras.get("seed", 0)
    n = min(B, DISTINCT)
    torch.manual_seed(seed)
    net = spread(TransformerEmbedding(**kwargs_of(case)), seed).eval()
    if "peaked" in extras:
        with torch.no_grad():
            for layer in net.layers:
                layer.self_attn.qkv_proj.weight[:(H + KV) * hd] *= extras["peaked"]
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(*((n, T) if case[8] == "scalar" else (n, T, F)), generator=g) * 1.3 + 0.2
    wts = torch.randn(n, E, generator=g)
    if "zero_sequence" in extras:
        x[extras["zero_sequence"]] = 0.0
    rows = torch.arange(B) % n
    return net, x[rows].contiguous(), wts[rows].contiguous(), n


# ------------------------------------------------------------------------------------------------------- the oracle
def per_sequence(net, x, wts, case, distinct=None, positive=None, keep_masks=None):
    """fp64 (out (B, E), flat gradient (P), sum_b |g_b| (P)) of loss = sum(wts * out), one oracle call per distinct
    sequence; rows b >= distinct repeat row b % distinct.  `positive` / `keep_masks`: per layer, sliced per sequence."""
    B = x.shape[0]
    n = B if distinct is None else distinct
    state, kw = net.state_dict(), kwargs_of(case)
    if keep_masks is not None:
        kw = dict(kw, attention_dropout=net.config["attention_dropout"])
    outs, grad, mag = [], 0.0, 0.0
    for b in range(n):
        count = len(range(b, B, n))
        out, g = O.reference(state, x[b:b + 1], wts[b:b + 1], kw,
                             keep_masks=None if keep_masks is None else [m[b:b + 1] for m in keep_masks],
                             positive=None if positive is None else [m[b:b + 1] for m in positive])
        outs.append(out)
        grad = grad + count * g
        mag = mag + count * g.abs()
    return torch.cat(outs)[torch.arange(B) % n], grad, mag


def kink_references(net, x, wts, case, distinct=None):
    """(number of near-kink relu units, [(out, grad)] on the other sides of them): `kink_candidates` asserts <= 6"""
    near, candidates = O.kink_candidates(net.state_dict(), x, kwargs_of(case))
    return near, [per_sequence(net, x, wts, case, distinct, positive=c)[:2] for c in candidates[1:]]


def max_score(net, x, case):
    """the oracle's largest |S| over the open keys, per layer"""
    scores = []
    with torch.no_grad():
        O.forward({k: v.detach().double().cpu() for k, v in net.state_dict().items()}, x.detach().double().cpu(),
                  kwargs_of(case), scores=scores)
    return [s.abs().max().item() for s in scores]


# ---------------------------------------------------------------------------------------------------- the slot check
def worst(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


def nearest(got, ref, others):
    """the reference nearest `got` over the whole vector: fp64's own sides of the kinks, or one of `others`"""
    return min((ref, *others), key=lambda r: worst(got, r))


def slot_figures(sizes, kernel, eager, ref, per_seq_abs, others=()):
    """{slot: dict(kernel_err, eager_err, scale, ratio, bound)}; each route against its nearest reference, chosen once
    for the whole vector"""
    e_k = (kernel.detach().double().cpu() - nearest(kernel, ref, others)).abs()
    e_e = (eager.detach().double().cpu() - nearest(eager, ref, others)).abs()
    out = {}
    for name, lo, hi in slot_table(sizes):
        k, e, scale = e_k[lo:hi].max().item(), e_e[lo:hi].max().item(), per_seq_abs[lo:hi].max().item()
        ratio = k / e if e > 0 else float("inf") if k > 0 else 0.0
        out[name] = dict(kernel_err=k, eager_err=e, scale=scale, ratio=ratio, bound=max(4 * e, 16 * ULP * scale))
    return out


def slot_check(test, case, kernel, eager, ref, per_seq_abs, tag="", others=()):
    """The bound of the module docstring in every slot of the flat gradient of `case`.  Prints and records every slot
    before it asserts, and names every failing slot at once.  `others`: the fp64 gradients on the other sides of the
    relu kinks within the margin (`kink_references`).  `case`: a case tuple, or (label, sizes, input) of a net that
    is not in the table."""
    if isinstance(case[1], tuple):
        label, sizes, kind = case
    else:
        label, sizes, kind = case_id(case), sizes_of(case), case[8]
    label += ":" + tag if tag else ""
    P = param_count(sizes)
    assert kernel.numel() == eager.numel() == ref.numel() == per_seq_abs.numel() == P
    figures = slot_figures(sizes, kernel, eager, ref, per_seq_abs, others)
    for name, f in figures.items():
        print(f"{test}[{label}] {name}: kernel {f['kernel_err']:.3e} eager {f['eager_err']:.3e} "
              f"scale {f['scale']:.3e} bound {f['bound']:.3e} ratio {f['ratio']:.2f}")
    parity_log.record(test, label, **{name: {k: f[k] for k in ("kernel_err", "eager_err", "scale", "ratio")}
                                      for name, f in figures.items()})
    failing = {name: (f["kernel_err"], f["bound"]) for name, f in figures.items()
               if not f["kernel_err"] <= f["bound"]}
    if kind == "features":
        for name, lo, hi in slot_table(sizes)[:2]:
            for route, g in (("kernel", kernel), ("eager", eager)):
                if g[lo:hi].abs().max().item() != 0.0:
                    failing[f"{name} ({route} route, not exactly zero)"] = (g[lo:hi].abs().max().item(), 0.0)
    if failing:
        raise AssertionError((label, failing))
    return figures
