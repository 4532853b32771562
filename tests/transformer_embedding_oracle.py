"""fp64 restatement of sbi's TransformerEmbedding (sbi/neural_nets/embedding_nets/transformer.py) from its formulas, on a
state_dict: series mode with the gated MLP or the mixture of experts, the ViT front end, an `attention_mask`, and
optional dropout keep masks (one (B, H, T, T) boolean tensor per layer: weights = softmax * keep / (1 - p)).  The
angle of the position term is position / float64(div_term) on the module's own fp32 buffer values (recomputed here in
fp32 exactly as the class builds them)."""
import math

import torch

DEFAULTS = dict(pos_emb="rotary", pos_emb_base=10e4, rms_norm_eps=1e-05, router_jitter_noise=0.0, vit_dropout=0.5,
                mlp_activation="gelu", is_causal=True, vit=False, num_hidden_layers=4, num_attention_heads=12,
                num_key_value_heads=12, intermediate_size=256, ffn="mlp", head_dim=None, attention_dropout=0.5,
                final_emb_dimension=None, image_size=None, patch_size=None, num_channels=None, num_local_experts=None,
                num_experts_per_tok=None)


def full_config(kwargs):
    cfg = dict(DEFAULTS, **kwargs)
    if cfg["head_dim"] is None:
        cfg["head_dim"] = cfg["feature_space_dim"] // cfg["num_attention_heads"]
    return cfg


def div_term(cfg):
    """the fp32 buffer of the position encoder, as float64"""
    hd = cfg["head_dim"]
    if cfg["pos_emb"] == "none":
        return None
    div = cfg["pos_emb_base"] ** (torch.arange(0, hd, 2) / hd)          # fp32, as the class computes it
    assert div.dtype == torch.float32
    return (div.repeat(2) if cfg["pos_emb"] == "rotary" else div).double()


def position_term(x, cfg, div, positions):
    if div is None:
        return x
    angle = positions.double().view(-1, 1) / div
    if cfg["pos_emb"] == "rotary":
        half = x.shape[-1] // 2
        return x * angle.cos() + torch.cat((-x[..., half:], x[..., :half]), dim=-1) * angle.sin()
    pe = torch.zeros_like(x)
    pe[..., 0::2] = pe[..., 0::2] + angle.cos()
    pe[..., 1::2] = pe[..., 1::2] + angle.sin()
    return x + pe


def rms(x, w, eps):
    return w * x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def mlp(x, gate_up, down, cfg, gates=None, positive=None):
    gu = x @ gate_up.T
    inter = gate_up.shape[0] // 2
    gate, up = gu[..., :inter], gu[..., inter:]
    if gates is not None:
        gates.append(gate.detach())
    if positive is not None:                # relu with the side of every kink given: gate where positive, else 0
        act = gate * positive.to(gate.dtype)
    else:
        act = gelu(gate) if cfg["mlp_activation"] == "gelu" else gate.clamp_min(0.0)
    return (up * act) @ down.T


def moe(x, p, prefix, cfg):
    shape = x.shape
    flat = x.reshape(-1, shape[-1])
    probs = torch.softmax(flat @ p[prefix + "gate.weight"].T, dim=1)
    top, idx = torch.topk(probs, cfg["num_experts_per_tok"], dim=-1)
    top = top / top.sum(-1, keepdim=True)
    out = torch.zeros_like(flat)
    for e in range(cfg["num_local_experts"]):
        weight = (top * (idx == e)).sum(-1, keepdim=True)               # 0 where the expert is not selected
        y = mlp(flat, p[f"{prefix}experts.{e}.gate_up_proj.weight"], p[f"{prefix}experts.{e}.down_proj.weight"], cfg)
        out = out + weight * y
    return out.reshape(shape)


def vit_tokens(x, p, cfg):
    F = torch.nn.functional
    patch = cfg["patch_size"]
    emb = F.conv2d(x, p["preprocess.projection.weight"], p["preprocess.projection.bias"], stride=patch)
    emb = emb.flatten(2).transpose(1, 2)
    emb = torch.cat((p["preprocess.cls_token"].expand(x.shape[0], -1, -1), emb), dim=1)
    table = p["preprocess.position_embeddings"]
    side = int((table.shape[1] - 1) ** 0.5)
    grid = table[:, 1:].reshape(1, side, side, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(x.shape[2] // patch, x.shape[3] // patch), mode="bicubic", align_corners=False)
    grid = grid.permute(0, 2, 3, 1).reshape(1, -1, table.shape[-1])
    return emb + torch.cat((table[:, :1], grid), dim=1)


def forward(p, x, kwargs, keep_masks=None, attention_mask=None, gates=None, positive=None, scores=None):
    """p: {key: fp64 tensor}; x fp64; returns out (B, E) in fp64.  `gates`: a list that receives every block's gate
    pre-activations (the arguments of the activation).  `positive`: one boolean (B, T, I) tensor per block, the side of
    the kink every relu unit is differentiated on (see `kink_candidates`).  `scores`: a list that receives every
    block's scaled scores S (B, H, T, T), 0 on the masked keys."""
    cfg = full_config(kwargs)
    H, KV, hd, eps = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"], cfg["rms_norm_eps"]
    if cfg["vit"]:
        h = vit_tokens(x, p, cfg)
    elif x.ndim == 2:
        h = x.unsqueeze(-1) * p["scalar_projection.weight"][:, 0] + p["scalar_projection.bias"]
    else:
        h = x
    B, T, _ = h.shape
    div = div_term(cfg)
    positions = torch.arange(T)
    allowed = torch.ones(B, 1, T, T, dtype=torch.bool)
    if cfg["is_causal"] and not cfg["vit"]:
        if T != 1:
            allowed = allowed & torch.tril(torch.ones(T, T, dtype=torch.bool))
        else:
            allowed = torch.zeros(B, 1, 1, 1, dtype=torch.bool)          # the class masks the only key: a constant shift
        if attention_mask is not None:
            # the class ADDS finfo.min on the padded keys that the causal mask leaves open
            allowed = allowed & (attention_mask[:, None, None, :] != 0)
    for l in range(cfg["num_hidden_layers"]):
        pre = f"layers.{l}."
        qkv = rms(h, p[pre + "input_layernorm.weight"], eps) @ p[pre + "self_attn.qkv_proj.weight"].T
        q = qkv[..., :H * hd].reshape(B, T, H, hd).transpose(1, 2)
        k = qkv[..., H * hd:(H + KV) * hd].reshape(B, T, KV, hd).transpose(1, 2)
        v = qkv[..., (H + KV) * hd:].reshape(B, T, KV, hd).transpose(1, 2)
        q, k = position_term(q, cfg, div, positions), position_term(k, cfg, div, positions)
        k = k.repeat_interleave(H // KV, dim=1)
        v = v.repeat_interleave(H // KV, dim=1)
        s = q @ k.transpose(2, 3) / math.sqrt(hd)
        rows_open = allowed.any(-1, keepdim=True)
        if scores is not None:
            scores.append(torch.where(allowed & rows_open, s, torch.zeros_like(s)).detach())
        # a masked score is s + finfo.min == finfo.min in fp32: weight 0 next to an open key, and a row masked
        # everywhere has equal scores, uniform weights over ALL keys
        s = torch.where(rows_open, s.masked_fill(~allowed, -math.inf), torch.zeros_like(s))
        w = torch.softmax(s, dim=-1)
        if keep_masks is not None:
            w = w * keep_masks[l].double() / (1.0 - cfg["attention_dropout"])
        o = (w @ v).transpose(1, 2).reshape(B, T, H * hd)
        h = h + o @ p[pre + "self_attn.o_proj.weight"].T
        u = rms(h, p[pre + "post_attention_layernorm.weight"], eps)
        if cfg["ffn"] == "moe":
            h = h + moe(u, p, pre + "ffn.", cfg)
        else:
            h = h + mlp(u, p[pre + "ffn.gate_up_proj.weight"], p[pre + "ffn.down_proj.weight"], cfg, gates,
                        None if positive is None else positive[l])
    y = rms(h, p["norm.weight"], eps)[:, -1, :]
    return y @ p["aggregator.weight"].T + p["aggregator.bias"]


def reference(state_dict, x, wts, kwargs, keep_masks=None, attention_mask=None, positive=None):
    """(out, flat parameter gradient of sum(out * wts)) in fp64, the gradient in state_dict order"""
    p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in state_dict.items()}
    masks = None if keep_masks is None else [m.cpu() for m in keep_masks]
    am = None if attention_mask is None else attention_mask.cpu()
    out = forward(p, x.detach().double().cpu(), kwargs, masks, am, positive=positive)
    grads = torch.autograd.grad((out * wts.detach().double().cpu()).sum(), list(p.values()), allow_unused=True)
    flat = torch.cat([(g if g is not None else torch.zeros_like(v)).reshape(-1) for g, v in zip(grads, p.values())])
    return out.detach(), flat


def flat_grad(module):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                      for p in module.parameters()])


def golden_net(cls, case):
    net = cls(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    return net.train(case["mode"] == "train")


def kink_candidates(state_dict, x, kwargs, limit=6):
    """The kink.  A relu unit whose fp64 pre-activation lies within 64 * 2^-24 * max|gate| of 0 may fall on either
    side in fp32 (the rounding of a dot product of at most 128 terms stays far inside that margin), and the gradient
    jumps there.  Returns (number of such units, [positive masks]): every assignment of sides that differs from
    fp64's only at those units, fp64's own first.  A route whose gradient matches none of them sits on the other
    side of a kink somewhere else."""
    import itertools

    gates = []
    with torch.no_grad():
        forward({k: v.detach().double().cpu() for k, v in state_dict.items()}, x.detach().double().cpu(), kwargs,
                gates=gates)
    margin = 64 * 2.0**-24 * max(g.abs().max().item() for g in gates)
    base = [g > 0 for g in gates]
    near = [(l, idx) for l, g in enumerate(gates) for idx in torch.nonzero(g.abs() <= margin).tolist()]
    assert len(near) <= limit, f"{len(near)} pre-activations within the margin of a kink"
    candidates = []
    for flips in itertools.product((False, True), repeat=len(near)):
        masks = [b.clone() for b in base]
        for flip, (l, idx) in zip(flips, near):
            if flip:
                masks[l][tuple(idx)] = ~masks[l][tuple(idx)]
        candidates.append(masks)
    return len(near), candidates


