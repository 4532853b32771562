"""``TransformerEmbedding`` -- sbi/neural_nets/embedding_nets/transformer.py (a decoder-style transformer for time series
and, through ViT patches, images) on the tr_embed HIP kernels.

Same keyword-only signature, defaults, messages, ``config`` dict, non-persistent ``div_term`` buffers and ``state_dict``
keys as the reference: every block is RMSNorm -> attention (one fused ``qkv_proj``, grouped key/value heads, a rotary
or additive position term on the per-head queries and keys, scores / sqrt(head_dim), an additive ``finfo.min`` causal
mask, dropout on the attention weights) -> residual -> RMSNorm -> gated MLP (or a mixture of experts) -> residual; the
last token of the final RMSNorm goes through ``aggregator``.  Two routes with the same semantics:

* the eager route: the whole class surface (ViT mode, ``ffn="moe"``, ``attention_mask``, ``position_ids``, any dtype,
  host tensors) -- a fallback, never a refusal;
* the kernel route: a ``torch.autograd.Function`` on ``sbi_amd_tr_forward`` / ``_backward`` (include/sbi_amd_tr.h).  It
  is taken for ``vit=False``, ``ffn="mlp"``, no ``attention_mask`` / ``position_ids``, an fp32 input (B, T) or
  (B, T, feature_space_dim) on a ROCm device that does not require grad (the kernels have no d/dx), fp32 parameters on
  that device, ``num_attention_heads * head_dim == feature_space_dim`` and a shape the host-side plan accepts within
  ``MAX_WORKSPACE_BYTES``; a call that needs gradients also has to stay below ``MAX_TRAINING_WORK``, where eager torch
  measured faster.  ``module.kernel_route(x)`` tells which and why; ``module.force_eager = True`` pins eager.

Attention dropout runs inside the kernel route: the keep decision of (layer, b, head, q, k) is a Philox-4x32-10 uniform
keyed with a 64-bit seed, drawn once per forward call from torch's default host generator (``torch.manual_seed`` makes
a run reproducible) or pinned with ``module.dropout_seed = <int>``.  The backward regenerates the masks.  The eager
route keeps ``F.dropout``: the two routes draw different streams.

Departure from the reference: a second causal call with the same ``attention_mask`` tensor raises "Boolean value of
Tensor ... is ambiguous" there (its mask cache compares tensors with ``==``); this module keeps no cache and returns the
first call's numbers.
"""

from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets.fully_connected import flat_image, split_like

MAX_WORKSPACE_BYTES = 1 << 30
# A call that needs gradients with B * T * feature_space_dim * num_hidden_layers at or above this runs eager.  Measured
# forward + backward at feature_space_dim 96, 4 layers, T = 100 (profiles/transformer_embed_bench.json): the kernels
# win at B = 4, 16, 32 (4.5 x, 3.1 x, 1.7 x: eager is bound by its launches there) and lose from B = 64 on (0.89 x,
# 0.55 x at 128, 0.41 x at 200); (200, 32) at 48 features and 2 layers, below the threshold, wins 2.6 x.  The
# threshold is the first measured loss.
MAX_TRAINING_WORK = 64 * 100 * 96 * 4

_POS = {"rotary": 0, "positional": 1, "none": 2}
_ACT = {"gelu": 0, "relu": 1}

_PLAN_REASONS = {
    _lib.E_UNSUPPORTED: "shape outside the kernel envelope (feature_space_dim <= 128, even head_dim in 2..64, "
                        "intermediate_size <= 512, num_hidden_layers <= 8, final_emb_dimension <= 128, T <= 4096, "
                        "B T max(F, 2 I) < 2^31)",
    _lib.E_BADARG: "empty input",
    _lib.E_LDS: "a kernel's tile does not fit 160 KiB of LDS",
}


# ---- the formulas, written once: the modules below and `tr_functional` are thin wrappers over them ------------------
def _frequencies(head_dim: int, base: float) -> Tensor:
    """div_term[i] = base^(2 i / head_dim), i < head_dim / 2, in fp32"""
    return torch.pow(base, torch.arange(0, head_dim, 2) / head_dim)


def _angles(x: Tensor, div: Tensor, position_ids: Optional[Tensor]) -> Tensor:
    """(T, len(div)) angles position / div_term in x's dtype; positions 0 .. T-1 unless given"""
    T = x.shape[-2]
    pos = torch.arange(T, device=x.device) if position_ids is None else position_ids.reshape(-1)
    return pos.to(x.dtype)[:, None] / div.to(device=x.device, dtype=x.dtype)[None, :]


def _rotary(x: Tensor, div: Tensor, position_ids: Optional[Tensor] = None) -> Tensor:
    """Each pair (x[d], x[d + hd/2]) is turned by the angle of frequency d: (a, b) -> (a c - b s, b c + a s).
    `div` holds the hd / 2 frequencies twice, as the buffer of ``RotaryEncoder`` does."""
    angle = _angles(x, div, position_ids)
    c, s = torch.cos(angle), torch.sin(angle)
    half = x.shape[-1] // 2
    a, b = x[..., :half], x[..., half:]
    return torch.cat((a * c[:, :half] - b * s[:, :half], b * c[:, half:] + a * s[:, half:]), dim=-1)


def _additive(x: Tensor, div: Tensor, position_ids: Optional[Tensor] = None) -> Tensor:
    """x[2 i] + cos(angle_i), x[2 i + 1] + sin(angle_i)"""
    angle = _angles(x, div, position_ids)
    table = torch.stack((torch.cos(angle), torch.sin(angle)), dim=-1).flatten(-2)        # (T, hd), interleaved
    return x + table


def _rms(x: Tensor, w: Tensor, eps: float) -> Tensor:
    return w * (x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps))


def _blocked_mask(T: int, like: Tensor, attention_mask: Optional[Tensor] = None) -> Tensor:
    """(B or 1, 1, T, T) additive mask: finfo.min on the keys after the query and on the keys `attention_mask`
    (B, T) zeroes, 0 elsewhere.  With a single step the only key is masked too (a constant shift of the row)."""
    lowest = torch.finfo(like.dtype).min
    steps = torch.arange(T, device=like.device)
    blocked = (steps[None, :] > steps[:, None]) if T > 1 else torch.ones(1, 1, dtype=torch.bool, device=like.device)
    blocked = blocked[None, None]
    if attention_mask is not None:
        n = attention_mask.shape[-1]
        padded = torch.zeros(attention_mask.shape[0], 1, 1, T, dtype=torch.bool, device=like.device)
        padded[..., :n] = (attention_mask == 0)[:, None, None, :].to(like.device)
        blocked = blocked | padded
    return torch.zeros(blocked.shape, dtype=like.dtype, device=like.device).masked_fill(blocked, lowest)


def _attention(q: Tensor, k: Tensor, v: Tensor, mask: Optional[Tensor], p: float, training: bool,
               keep: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """q (B, H, T, hd), k / v (B, KV, T, hd) -> (output (B, H, T, hd), dropped weights (B, H, T, T)).  The H / KV query
    heads of a group read one shared key / value head.  `keep` replaces F.dropout's own draw."""
    B, H, T, hd = q.shape
    KV = k.shape[1]
    grouped = q.reshape(B, KV, H // KV, T, hd)
    scores = torch.einsum("bkgqd,bksd->bkgqs", grouped, k).reshape(B, H, T, -1) / math.sqrt(hd)
    if mask is not None:
        scores = scores + mask
    weights = torch.softmax(scores, dim=-1)
    if keep is not None:
        weights = weights * keep.to(weights.dtype) / (1.0 - p)
    else:
        weights = F.dropout(weights, p=p, training=training)
    out = torch.einsum("bkgqs,bksd->bkgqd", weights.reshape(B, KV, H // KV, T, -1), v)
    return out.reshape(B, H, T, hd), weights


def _heads(x: Tensor, heads: int, head_dim: int) -> Tensor:
    """(B, T, heads * head_dim) -> (B, heads, T, head_dim)"""
    return x.reshape(x.shape[0], x.shape[1], heads, head_dim).transpose(1, 2)


def _gated_mlp(x: Tensor, gate_up: Tensor, down: Tensor, act) -> Tensor:
    gate, up = F.linear(x, gate_up).split(gate_up.shape[0] // 2, dim=-1)
    return F.linear(up * act(gate), down)


_ACTIVATIONS = {"gelu": F.gelu, "relu": F.relu}


# ---- the modules: the reference's surface (names, parameters, buffers, messages) over the formulas above -------------
class PositionalEncoder(nn.Module):
    """Additive sine / cosine position term (Vaswani et al.) on (bsz, heads, seq_len, head_dim) queries or keys."""

    def __init__(self, head_dim: int, base: Optional[float] = 10e4):
        super().__init__()
        if head_dim % 2 != 0:
            raise ValueError(f"`head_dim`:{head_dim} must be even")
        self.base, self.head_dim = base, head_dim
        self.register_buffer("div_term", _frequencies(head_dim, base), persistent=False)

    def forward(self, x: Tensor, position_ids: Optional[Tensor] = None) -> Tensor:
        return _additive(x, self.div_term, position_ids)


class IdentityEncoder(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, x: Tensor, **kwargs) -> Tensor:
        return x


class RotaryEncoder(nn.Module):
    """Rotary position term (Su et al.) on (bsz, heads, seq_len, head_dim) queries or keys."""

    def __init__(self, head_dim: int, base: Optional[float] = 10e4):
        super().__init__()
        if head_dim % 2 != 0:
            raise ValueError(f"`head_dim`:{head_dim} must be even")
        self.base, self.head_dim = base, head_dim
        self.register_buffer("div_term", _frequencies(head_dim, base).repeat(2), persistent=False)

    def forward(self, x: Tensor, position_ids: Optional[Tensor] = None) -> Tensor:
        return _rotary(x, self.div_term, position_ids)


_ENCODERS = {"positional": PositionalEncoder, "rotary": RotaryEncoder, "none": IdentityEncoder}


class FullAttention(nn.Module):
    """Multi-head attention with one fused ``qkv_proj`` and ``num_key_value_heads`` shared key / value heads."""

    def __init__(self, config):
        super().__init__()
        Fd, H, KV = config["feature_space_dim"], config["num_attention_heads"], config["num_key_value_heads"]
        hd = config["head_dim"]
        if hd is None:
            if Fd % H != 0:
                raise ValueError("If not providing head_dim, ensure `feature_space_dim` is divisible by "
                                 "`num_attention_heads`")
            hd = Fd // H
        if H % KV != 0:
            raise ValueError("`num_attention_heads` must be divisible by `num_key_value_heads`")
        self.config = config
        self.feature_space_dim, self.head_dim, self.num_heads, self.num_key_value_heads = Fd, hd, H, KV
        self.num_key_value_groups = H // KV
        self.attention_dropout = config["attention_dropout"]
        self.o_proj = nn.Linear(H * hd, Fd, bias=False)
        self.qkv_proj = nn.Linear(Fd, (H + 2 * KV) * hd, bias=False)
        self.pos_emb = _ENCODERS[config["pos_emb"]](head_dim=hd, base=config["pos_emb_base"])

    def forward(self, hidden_states: Tensor, attention_mask: Optional[Tensor] = None,
                position_ids: Optional[Tensor] = None, output_attentions: bool = False
                ) -> Tuple[Tensor, Optional[Tensor]]:
        H, KV, hd = self.num_heads, self.num_key_value_heads, self.head_dim
        q, k, v = self.qkv_proj(hidden_states).split((H * hd, KV * hd, KV * hd), dim=-1)
        q = self.pos_emb(_heads(q, H, hd), position_ids=position_ids)
        k = self.pos_emb(_heads(k, KV, hd), position_ids=position_ids)
        out, weights = _attention(q, k, _heads(v, KV, hd), attention_mask, self.attention_dropout, self.training, None)
        # (B, H, T, hd) -> (B, T, feature_space_dim): torch's reshape error when H * hd != feature_space_dim
        out = out.transpose(1, 2).reshape(hidden_states.shape[0], hidden_states.shape[1], self.feature_space_dim)
        return self.o_proj(out), (weights if output_attentions else None)


class MLP(nn.Module):
    """Gated feed-forward block: down_proj(up * act(gate)) with (gate | up) = gate_up_proj(x)."""

    def __init__(self, config):
        super().__init__()
        if config["mlp_activation"] not in _ACTIVATIONS:
            raise ValueError("Unsupported activation function, currently supported: `gelu, relu`")
        self.config = config
        self.gate_up_proj = nn.Linear(config["feature_space_dim"], 2 * config["intermediate_size"], bias=False)
        self.down_proj = nn.Linear(config["intermediate_size"], config["feature_space_dim"], bias=False)
        self.activation_fn = _ACTIVATIONS[config["mlp_activation"]]

    def forward(self, hidden_states: Tensor) -> Tensor:
        return _gated_mlp(hidden_states, self.gate_up_proj.weight, self.down_proj.weight, self.activation_fn)


class RMSNorm(nn.Module):
    def __init__(self, feature_space_dim, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(feature_space_dim))
        self.variance_epsilon = eps

    def forward(self, hidden_states: Tensor) -> Tensor:
        return _rms(hidden_states, self.weight, self.variance_epsilon)


class MoeBlock(nn.Module):
    """Mixture of experts at full capacity: a token's output is the sum of its ``num_experts_per_tok`` best experts,
    weighted with their router probabilities renormalised to 1."""

    def __init__(self, config):
        super().__init__()
        self.hidden_dim, self.ffn_dim = config["feature_space_dim"], config["intermediate_size"]
        self.num_experts, self.top_k = config["num_local_experts"], config["num_experts_per_tok"]
        if self.top_k > self.num_experts:
            raise ValueError("Each token cannot be assigned to more that num_local_experts")
        self.gate = nn.Linear(self.hidden_dim, self.num_experts, bias=False)
        self.experts = nn.ModuleList([MLP(config) for _ in range(self.num_experts)])
        self.jitter_noise = config["router_jitter_noise"]

    def forward(self, hidden_states: Tensor) -> Tensor:
        tokens = hidden_states.reshape(-1, hidden_states.shape[-1])
        if self.training and self.jitter_noise > 0:
            tokens = tokens * (1.0 + self.jitter_noise * (2.0 * torch.rand_like(tokens) - 1.0))
        probs = torch.softmax(self.gate(tokens).float(), dim=-1)
        best, chosen = probs.topk(self.top_k, dim=-1)
        # (tokens, experts): the renormalised probability of a chosen expert, 0 for the others
        share = torch.zeros_like(probs).scatter(1, chosen, best / best.sum(dim=-1, keepdim=True)).to(tokens.dtype)
        out = torch.zeros_like(tokens)
        for e, expert in enumerate(self.experts):
            rows = torch.nonzero(share[:, e] > 0).squeeze(-1)
            if rows.numel():
                out = out.index_add(0, rows, share[rows, e:e + 1] * expert(tokens[rows]))
        return out.reshape(hidden_states.shape)


class TransformerBlock(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.feature_space_dim = config["feature_space_dim"]
        self.self_attn = FullAttention(config=config)
        self.ffn = {"mlp": MLP, "moe": MoeBlock}[config["ffn"]](config)
        self.input_layernorm = RMSNorm(config["feature_space_dim"], eps=config["rms_norm_eps"])
        self.post_attention_layernorm = RMSNorm(config["feature_space_dim"], eps=config["rms_norm_eps"])

    def forward(self, hidden_states: Tensor, attention_mask: Optional[Tensor] = None,
                position_ids: Optional[Tensor] = None, output_attentions: Optional[bool] = False, **kwargs
                ) -> Tuple[Tensor, Optional[Tensor]]:
        attn, weights = self.self_attn(self.input_layernorm(hidden_states), attention_mask=attention_mask,
                                       position_ids=position_ids, output_attentions=bool(output_attentions))
        hidden_states = hidden_states + attn
        return hidden_states + self.ffn(self.post_attention_layernorm(hidden_states)), weights


class ViTEmbeddings(nn.Module):
    """(batch, channels, height, width) pixels -> (batch, 1 + patches, feature_space_dim) tokens: a class token in
    front of the patch projections, plus a learned position table."""

    def __init__(self, config):
        super().__init__()
        self.image_size, self.patch_size = config["image_size"], config["patch_size"]
        self.num_channels = config["num_channels"]
        Fd = config["feature_space_dim"]
        patches = (self.image_size // self.patch_size) ** 2
        self.position_embeddings = nn.Parameter(torch.randn(1, patches + 1, Fd))
        self.projection = nn.Conv2d(self.num_channels, Fd, kernel_size=self.patch_size, stride=self.patch_size)
        self.cls_token = nn.Parameter(torch.randn(1, 1, Fd))
        self.dropout = nn.Dropout(config["vit_dropout"])

    def interpolate_pos_encoding(self, embeddings: Tensor, height: int, width: int) -> Tensor:
        """The position table on the patch grid of a (height, width) image: the class entry as it is, the patch
        entries read as a square image of feature_space_dim channels and resampled bicubically."""
        table = self.position_embeddings
        side = math.isqrt(table.shape[1] - 1)
        grid = table[0, 1:].T.reshape(1, table.shape[-1], side, side)
        grid = F.interpolate(grid, size=(height // self.patch_size, width // self.patch_size), mode="bicubic",
                             align_corners=False)
        return torch.cat((table[:, :1], grid.flatten(2).transpose(1, 2)), dim=1)

    def forward(self, pixel_values: Tensor) -> Tensor:
        channels = pixel_values.shape[1]
        if channels != self.num_channels:
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the "
                             f"configuration. Expected {self.num_channels} but got {channels}.")
        patches = self.projection(pixel_values).flatten(2).transpose(1, 2)
        tokens = torch.cat((self.cls_token.expand(patches.shape[0], -1, -1), patches), dim=1)
        return self.dropout(tokens + self.interpolate_pos_encoding(tokens, *pixel_values.shape[2:]))


# ---- the written formula on the flat parameter list -------------------------------------------------------------------
def tr_functional(x: Tensor, params: Sequence[Tensor], config: dict,
                  keep_masks: Optional[Sequence[Tensor]] = None) -> Tensor:
    """The formula the kernels implement (series mode, ``ffn="mlp"``), on the parameters in ``state_dict`` order.
    `keep_masks`: one (B, H, T, T) boolean tensor per layer; with it the dropped attention weights are
    softmax * keep / (1 - attention_dropout), without it there is no dropout."""
    Fd, H, KV = config["feature_space_dim"], config["num_attention_heads"], config["num_key_value_heads"]
    hd = config["head_dim"] if config["head_dim"] is not None else Fd // H
    L, eps, p = config["num_hidden_layers"], config["rms_norm_eps"], config["attention_dropout"]
    act = _ACTIVATIONS[config["mlp_activation"]]
    h = x.unsqueeze(-1) * params[0][:, 0] + params[1] if x.ndim == 2 else x
    B, T, _ = h.shape
    div = _frequencies(hd, config["pos_emb_base"])
    turn = {"rotary": lambda t: _rotary(t, div.repeat(2)), "positional": lambda t: _additive(t, div),
            "none": lambda t: t}[config["pos_emb"]]
    mask = _blocked_mask(T, h) if config["is_causal"] else None
    for l in range(L):
        ow, qkvw, guw, dw, ln1, ln2 = params[2 + 6 * l:8 + 6 * l]
        q, k, v = F.linear(_rms(h, ln1, eps), qkvw).split((H * hd, KV * hd, KV * hd), dim=-1)
        keep = keep_masks[l] if keep_masks is not None else None
        o, _ = _attention(turn(_heads(q, H, hd)), turn(_heads(k, KV, hd)), _heads(v, KV, hd), mask, p, False, keep)
        h = h + F.linear(o.transpose(1, 2).reshape(B, T, H * hd), ow)
        h = h + _gated_mlp(_rms(h, ln2, eps), guw, dw, act)
    nw, aw, ab = params[2 + 6 * L:5 + 6 * L]
    return F.linear(_rms(h[:, -1, :], nw, eps), aw, ab)


# ---- the kernel route -------------------------------------------------------------------------------------------------
def tr_config(config: dict, final_emb_dimension: int, div_term: Sequence[float], scalar_input: bool
              ) -> _lib.TRConfigC:
    cfg = _lib.TRConfigC()
    Fd, H = int(config["feature_space_dim"]), int(config["num_attention_heads"])
    cfg.feature_space_dim, cfg.num_attention_heads = Fd, H
    cfg.num_key_value_heads = int(config["num_key_value_heads"])
    cfg.head_dim = int(config["head_dim"]) if config["head_dim"] is not None else Fd // max(H, 1)
    cfg.intermediate_size = int(config["intermediate_size"])
    cfg.num_hidden_layers = int(config["num_hidden_layers"])
    cfg.final_emb_dimension = int(final_emb_dimension)
    cfg.pos_emb = _POS.get(config["pos_emb"], -1)
    cfg.activation = _ACT.get(config["mlp_activation"], -1)
    cfg.is_causal = int(bool(config["is_causal"]))
    cfg.scalar_input = int(bool(scalar_input))
    cfg.rms_norm_eps = float(config["rms_norm_eps"])
    for i, d in enumerate(list(div_term)[:32]):
        cfg.div_term[i] = float(d)
    return cfg


def plan(cfg: _lib.TRConfigC, batch: int, seq_len: int) -> Tuple[int, List[int], int, int]:
    """(rc, lds bytes of the six kernels, key tile, weight-gradient partials): a host-side answer"""
    lds = (ctypes.c_int32 * 6)()
    tile, parts = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = int(_lib.load().sbi_amd_tr_plan(ctypes.byref(cfg), batch, seq_len, lds, ctypes.byref(tile),
                                         ctypes.byref(parts)))
    return rc, [int(v) for v in lds], int(tile.value), int(parts.value)


def plan_reason(rc: int) -> str:
    return _PLAN_REASONS.get(rc, f"plan error {rc}")


def param_count(cfg: _lib.TRConfigC) -> Tuple[int, List[int]]:
    offsets = (ctypes.c_int64 * (6 * max(int(cfg.num_hidden_layers), 0) + 5))()
    n = int(_lib.load().sbi_amd_tr_param_count(ctypes.byref(cfg), offsets))
    return n, [int(o) for o in offsets]


def workspace_bytes(cfg: _lib.TRConfigC, batch: int, seq_len: int, training: bool) -> int:
    return int(_lib.load().sbi_amd_tr_workspace_bytes(ctypes.byref(cfg), batch, seq_len, int(training)))


def dropout_mask(cfg: _lib.TRConfigC, batch: int, seq_len: int, p: float, seed: int, layer: int, device) -> Tensor:
    """(B, H, T, T) boolean keep decisions of `layer`, written by the device function the attention kernels call"""
    keep = torch.empty(batch, int(cfg.num_attention_heads), seq_len, seq_len, dtype=torch.uint8, device=device)
    _lib.check(_lib.load().sbi_amd_tr_dropout_mask(ctypes.byref(cfg), batch, seq_len, float(p), int(seed), layer,
                                                   keep.data_ptr(), _lib.current_stream(keep.device)),
               "tr_dropout_mask")
    return keep.bool()


class _TREmbedFn(torch.autograd.Function):
    """out = module(x) on the kernels; x (B, T) or (B, T, F) contiguous fp32 on the device."""

    @staticmethod
    def forward(ctx, x: Tensor, meta, *params: Tensor) -> Tensor:
        cfg, config, p, seed = meta
        lib = _lib.load()
        B, T = x.shape[0], x.shape[1]
        training = any(ctx.needs_input_grad[2:])
        flat = flat_image(params)
        out = torch.empty(B, int(cfg.final_emb_dimension), dtype=torch.float32, device=x.device)
        nbytes = workspace_bytes(cfg, B, T, training)
        if nbytes < 0:
            _lib.check(nbytes, "tr_workspace_bytes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        _lib.check(lib.sbi_amd_tr_forward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                          B, T, p, seed, out.data_ptr(), ws.data_ptr(), int(training),
                                          _lib.current_stream(x.device)), "tr_forward")
        ctx.meta = meta
        ctx.stash = ws if training else None
        ctx.save_for_backward(x, flat, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        x, flat, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        cfg, config, p, seed = ctx.meta
        if torch.is_grad_enabled():
            # double backward (create_graph=True): differentiate the written formula instead, with the same masks
            with torch.enable_grad():
                keep = None
                if p > 0:
                    keep = [dropout_mask(cfg, x.shape[0], x.shape[1], p, seed, l, x.device)
                            for l in range(int(cfg.num_hidden_layers))]
                wanted = [t for t, n in zip(params, need[2:]) if n]
                got = iter(torch.autograd.grad(tr_functional(x, params, config, keep), wanted, grad_out,
                                               create_graph=True, allow_unused=True))
            return (None, None, *[next(got) if n else None for n in need[2:]])
        lib = _lib.load()
        grad_out = grad_out.contiguous()
        grad_flat = torch.empty_like(flat)
        _lib.check(lib.sbi_amd_tr_backward(ctypes.byref(cfg), flat.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
                                           x.shape[0], x.shape[1], p, seed, grad_out.data_ptr(), grad_flat.data_ptr(),
                                           ctx.stash.data_ptr(), _lib.current_stream(x.device)), "tr_backward")
        grads = [g if n else None for g, n in zip(split_like(grad_flat, params), need[2:])]
        return (None, None, *grads)


class TransformerEmbedding(nn.Module):
    r"""sbi's ``TransformerEmbedding``: a transformer embedding for time series and, with ``vit=True``, images.

    Args:
        pos_emb: position term on the queries and keys, one of {"rotary", "positional", "none"}.
        pos_emb_base: base of the position term's frequencies.
        rms_norm_eps: epsilon of every RMSNorm.
        router_jitter_noise: multiplicative noise before the MoE router (training, ``ffn="moe"``).
        vit_dropout: dropout on the patch embeddings (``vit=True``).
        mlp_activation: activation of the gated feed-forward block, "gelu" or "relu".
        is_causal: apply a causal mask (series mode only).
        vit: patchify (batch, channels, height, width) images instead of reading a series.
        num_hidden_layers, num_attention_heads, num_key_value_heads, intermediate_size: the blocks' sizes.
        ffn: "mlp" or "moe".
        head_dim: per-head dimension, feature_space_dim // num_attention_heads when None.
        attention_dropout: dropout on the attention weights.
        feature_space_dim: the model dimension.
        final_emb_dimension: output dimension, feature_space_dim // 2 when None.
        image_size, patch_size, num_channels: ViT mode.
        num_local_experts, num_experts_per_tok: MoE mode.

    Input (batch, seq_len) (a scalar series, lifted by ``scalar_projection``), (batch, seq_len, feature_space_dim), or
    (batch, channels, height, width) with ``vit=True``; output (batch, final_emb_dimension).

    ``force_eager = True`` on an instance pins the eager route; ``dropout_seed = <int>`` pins the kernel route's
    dropout seed for every call.
    """

    force_eager = False
    dropout_seed: Optional[int] = None

    def __init__(
        self,
        *,
        pos_emb: str = "rotary",
        pos_emb_base: float = 10e4,
        rms_norm_eps: float = 1e-05,
        router_jitter_noise: float = 0.0,
        vit_dropout: float = 0.5,
        mlp_activation: str = "gelu",
        is_causal: bool = True,
        vit: bool = False,
        num_hidden_layers: int = 4,
        num_attention_heads: int = 12,
        num_key_value_heads: int = 12,
        intermediate_size: int = 256,
        ffn: str = "mlp",
        head_dim: Optional[int] = None,
        attention_dropout: float = 0.5,
        feature_space_dim: int,
        final_emb_dimension: Optional[int] = None,
        image_size: Optional[int] = None,
        patch_size: Optional[int] = None,
        num_channels: Optional[int] = None,
        num_local_experts: Optional[int] = None,
        num_experts_per_tok: Optional[int] = None,
    ):
        super().__init__()
        self.config = dict(
            pos_emb=pos_emb,
            pos_emb_base=pos_emb_base,
            rms_norm_eps=rms_norm_eps,
            router_jitter_noise=router_jitter_noise,
            vit_dropout=vit_dropout,
            mlp_activation=mlp_activation,
            is_causal=is_causal,
            vit=vit,
            num_hidden_layers=num_hidden_layers,
            num_attention_heads=num_attention_heads,
            num_key_value_heads=num_key_value_heads,
            intermediate_size=intermediate_size,
            ffn=ffn,
            head_dim=head_dim,
            attention_dropout=attention_dropout,
            feature_space_dim=feature_space_dim,
            image_size=image_size,
            patch_size=patch_size,
            num_channels=num_channels,
            num_local_experts=num_local_experts,
            num_experts_per_tok=num_experts_per_tok,
        )
        self.preprocess = ViTEmbeddings(self.config) if vit else IdentityEncoder()
        self._supports_scalar_series = not vit
        if self._supports_scalar_series:
            self.scalar_projection = nn.Linear(1, feature_space_dim)
        self.layers = nn.ModuleList([TransformerBlock(self.config) for _ in range(num_hidden_layers)])
        self.is_causal = is_causal and not vit
        self.norm = RMSNorm(feature_space_dim, eps=rms_norm_eps)
        if final_emb_dimension is None:
            final_emb_dimension = feature_space_dim // 2
        if not vit and final_emb_dimension > feature_space_dim:
            raise ValueError("The final embedding dimension should be equal or smaller than the input dimension")
        self.aggregator = nn.Linear(feature_space_dim, final_emb_dimension)
        self._div_cache = None

    def causal_mask(self, sequence_length: int, batch_size: int, dtype: torch.dtype, device: torch.device,
                    min_dtype: float, attention_mask: Optional[Tensor] = None, **kwargs) -> Tensor:
        """(batch, 1, T, T) additive mask: the lowest finite value on the keys after the query and on the keys
        `attention_mask` zeroes, 0 elsewhere"""
        like = torch.empty(0, dtype=dtype, device=device)
        return _blocked_mask(sequence_length, like, attention_mask).expand(batch_size, 1, -1, -1)

    # -- routing --
    def _head_dim(self) -> int:
        return int(self.layers[0].self_attn.head_dim) if len(self.layers) else 0

    def _div_values(self) -> List[float]:
        """The position encoder's own fp32 buffer, hd / 2 values, as the kernels' config carries it."""
        div = getattr(self.layers[0].self_attn.pos_emb, "div_term", None)
        if div is None:
            return []
        key = (id(div), div._version)          # a replaced or edited buffer is read again
        if self._div_cache is None or self._div_cache[0] != key:
            self._div_cache = (key, [float(v) for v in div[: self._head_dim() // 2].cpu()])
        return self._div_cache[1]

    def kernel_config(self, scalar_input: bool) -> _lib.TRConfigC:
        return tr_config(dict(self.config, head_dim=self._head_dim()), self.aggregator.out_features,
                         self._div_values(), scalar_input)

    def kernel_parameters(self) -> List[Tensor]:
        """Every parameter in ``state_dict`` order, the kernels' flat image."""
        return list(self.parameters())

    def kernel_route(self, x: Tensor, attention_mask: Optional[Tensor] = None,
                     position_ids: Optional[Tensor] = None) -> Tuple[bool, str]:
        if self.force_eager:
            return False, "force_eager is set"
        if self.config["vit"]:
            return False, "vit=True runs eager"
        if self.config["ffn"] != "mlp":
            return False, 'ffn="moe" runs eager'
        if attention_mask is not None or position_ids is not None:
            return False, "attention_mask / position_ids run eager"
        if not isinstance(x, Tensor) or x.dtype != torch.float32:
            return False, "input is not float32"
        if not x.is_cuda:
            return False, "input is not on a ROCm device"
        Fd = int(self.config["feature_space_dim"])
        if x.ndim not in (2, 3) or (x.ndim == 3 and x.shape[-1] != Fd):
            return False, "input shape is neither (batch, seq_len) nor (batch, seq_len, feature_space_dim)"
        if x.requires_grad and torch.is_grad_enabled():
            return False, "input requires grad (the kernel backward has no d/dx)"
        if not all(p.device == x.device and p.dtype == torch.float32 for p in self.parameters()):
            return False, "parameters are not float32 on the input's device"
        if len(self.layers) == 0 or int(self.config["num_attention_heads"]) * self._head_dim() != Fd:
            return False, "num_attention_heads * head_dim != feature_space_dim"
        p = float(self.config["attention_dropout"]) if self.training else 0.0
        if not 0.0 <= p < 1.0:
            return False, "attention_dropout outside [0, 1)"
        cfg = self.kernel_config(x.ndim == 2)
        rc = plan(cfg, x.shape[0], x.shape[1])[0]
        if rc != 0:
            return False, plan_reason(rc)
        training = torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters())
        nbytes = workspace_bytes(cfg, x.shape[0], x.shape[1], training)
        if nbytes > MAX_WORKSPACE_BYTES:
            return False, (f"workspace of {nbytes} bytes passes MAX_WORKSPACE_BYTES = {MAX_WORKSPACE_BYTES} "
                           "(the stash of a call that needs gradients grows with B T num_hidden_layers)")
        work = x.shape[0] * x.shape[1] * Fd * len(self.layers)
        if training and work >= MAX_TRAINING_WORK:
            return False, (f"a call that needs gradients with B T F L = {work} >= {MAX_TRAINING_WORK}: eager torch "
                           "measured faster there (profiles/transformer_embed_bench.json)")
        return True, "kernel"

    def _seed(self) -> int:
        if self.dropout_seed is not None:
            return int(self.dropout_seed) & 0xFFFFFFFFFFFFFFFF
        return int(torch.randint(0, 2**62, (1,)).item())

    def forward(self, input: Tensor, attention_mask: Optional[Tensor] = None,
                position_ids: Optional[Tensor] = None, cache_attention_mask: Optional[bool] = True, **kwargs
                ) -> Tensor:
        """(batch, seq_len), (batch, seq_len, feature_space_dim) or, with ``vit=True``, (batch, channels, height,
        width) -> (batch, final_emb_dimension).  `attention_mask` (batch, seq_len): 0 on padded keys (causal mode)."""
        if self.kernel_route(input, attention_mask, position_ids)[0]:
            p = float(self.config["attention_dropout"]) if self.training else 0.0
            seed = self._seed() if p > 0 else 0
            meta = (self.kernel_config(input.ndim == 2), dict(self.config, head_dim=self._head_dim()), p, seed)
            return _TREmbedFn.apply(input.contiguous(), meta, *self.parameters())
        h = self.preprocess(input)
        if h.ndim == 2 and self._supports_scalar_series:
            h = self.scalar_projection(h[..., None])
        mask = _blocked_mask(h.shape[1], h, attention_mask) if self.is_causal else None
        for layer in self.layers:
            h, _ = layer(h, attention_mask=mask, position_ids=position_ids)
        return self.aggregator(self.norm(h[:, -1, :]))
