#!/usr/bin/env python
"""Generate tests/golden/transformer_embedding_reference.pt: state_dict, inputs, outputs and flat parameter gradients of
the REAL sbi class `TransformerEmbedding` (sbi/neural_nets/embedding_nets/transformer.py), plus its error messages and a
few recorded facts (entry order and parameter count at feature_space_dim=96, the failure of the docstring example and of
a second masked call).  Every parameter is moved by 0.2 randn so that every term matters.  Recorded in eval mode, one
case in training mode with both dropouts 0.  The gradient is flat in state_dict order.  Sizes are kept small (the file
must stay under 1 MB): intermediate_size is 16 or 8 instead of 256 everywhere, and only the first case runs at
feature_space_dim=48.  Data only; runs on the CPU, where the reference works; build container only."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(feature_space_dim=24, intermediate_size=8)

# name: (kwargs, input shape, mode: "eval" / "train", attention_mask: bool)
CASES = {
    "default_scalar": (dict(feature_space_dim=48, num_hidden_layers=2, intermediate_size=16), (3, 20), "eval", False),
    "features": (dict(SMALL, num_hidden_layers=2), (3, 20, 24), "eval", False),
    "positional": (dict(SMALL, num_hidden_layers=2, pos_emb="positional"), (3, 20), "eval", False),
    "none": (dict(SMALL, num_hidden_layers=2, pos_emb="none"), (3, 20), "eval", False),
    "kv_4_2": (dict(SMALL, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2), (3, 20), "eval", False),
    "kv_4_1": (dict(SMALL, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=1), (3, 20), "eval", False),
    "relu": (dict(SMALL, num_hidden_layers=1, mlp_activation="relu"), (3, 20), "eval", False),
    "not_causal": (dict(SMALL, num_hidden_layers=1, is_causal=False), (3, 20), "eval", False),
    "one_step": (dict(SMALL, num_hidden_layers=1), (3, 1), "eval", False),
    "head_dim_6": (dict(feature_space_dim=36, intermediate_size=8, num_hidden_layers=2, num_attention_heads=6,
                        num_key_value_heads=6), (3, 20), "eval", False),
    "final_emb": (dict(SMALL, num_hidden_layers=1, final_emb_dimension=7), (3, 20), "eval", False),
    "moe": (dict(SMALL, num_hidden_layers=2, ffn="moe", num_local_experts=3, num_experts_per_tok=2), (3, 20), "eval",
            False),
    "vit": (dict(SMALL, num_hidden_layers=1, vit=True, image_size=16, patch_size=4, num_channels=2, vit_dropout=0.0,
                 attention_dropout=0.0), (2, 2, 16, 16), "train", False),
    "mask": (dict(SMALL, num_hidden_layers=1), (3, 20), "eval", True),
    "train_no_dropout": (dict(SMALL, num_hidden_layers=1, attention_dropout=0.0, vit_dropout=0.0), (3, 20), "train",
                         False),
}


def record(cls, kwargs, shape, mode, masked, seed):
    torch.manual_seed(100 + seed)
    net = cls(**kwargs)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
    net.train(mode == "train")
    x = torch.randn(*shape, generator=g) * 1.3 + 0.2
    attention_mask = None
    if masked:
        attention_mask = torch.ones(shape[0], shape[1])
        attention_mask[0, :3] = 0
        attention_mask[2, 5:9] = 0
    out = net(x.clone(), attention_mask=attention_mask)
    wts = torch.randn(out.shape, generator=g)
    net.zero_grad()
    (out * wts).sum().backward()
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in net.parameters()])
    return {"kwargs": kwargs, "seed": seed, "mode": mode, "attention_mask": attention_mask,
            "state_dict": {k: v.clone() for k, v in net.state_dict().items()},
            "x": x.clone(), "out": out.detach().clone(), "wts": wts, "grad_flat": flat}


def message(fn, kind):
    try:
        fn()
    except kind as e:
        return str(e)
    raise RuntimeError("no error raised")


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # installs the third-party stubs and puts the reference on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.neural_nets.embedding_nets.transformer import MLP, MoeBlock, TransformerEmbedding

    T = TransformerEmbedding
    out = {"cases": {name: record(T, *case, i) for i, (name, case) in enumerate(CASES.items())}}
    vit = dict(SMALL, num_hidden_layers=1, vit=True, image_size=16, patch_size=4, num_channels=2)
    out["messages"] = {
        "odd_head_dim": message(lambda: T(feature_space_dim=36, head_dim=3), ValueError),
        "odd_head_dim_positional": message(lambda: T(feature_space_dim=36, head_dim=3, pos_emb="positional"),
                                           ValueError),
        "heads_divide_features": message(lambda: T(feature_space_dim=64), ValueError),
        "kv_divide_heads": message(lambda: T(feature_space_dim=24, num_key_value_heads=5), ValueError),
        "final_emb": message(lambda: T(feature_space_dim=24, final_emb_dimension=25), ValueError),
        "activation": message(lambda: T(feature_space_dim=24, mlp_activation="tanh"), ValueError),
        "top_k": message(lambda: T(feature_space_dim=24, ffn="moe", num_local_experts=2, num_experts_per_tok=3),
                         ValueError),
        "vit_channels": message(lambda: T(**vit)(torch.zeros(2, 3, 16, 16)), ValueError),
    }
    big = T(feature_space_dim=96)
    mism = T(feature_space_dim=24, num_attention_heads=4, num_key_value_heads=4, head_dim=4, num_hidden_layers=1)
    masked = T(**dict(SMALL, num_hidden_layers=1)).eval()
    am = torch.ones(2, 5)
    masked(torch.zeros(2, 5), attention_mask=am)
    out["facts"] = {
        "keys_96": list(big.state_dict().keys()),
        "shapes_96": [tuple(v.shape) for v in big.state_dict().values()],
        "param_count_96": sum(p.numel() for p in big.parameters()),
        "buffers_96": [(k, tuple(v.shape)) for k, v in big.named_buffers()],
        "div_term_rotary_hd8": big.layers[0].self_attn.pos_emb.div_term.clone(),
        "div_term_positional_hd8": T(feature_space_dim=96, pos_emb="positional").layers[0].self_attn.pos_emb
        .div_term.clone(),
        "config_96": dict(big.config),
        "head_dim_mismatch_forward": message(lambda: mism(torch.zeros(2, 5)), RuntimeError),
        "second_masked_call": message(lambda: masked(torch.zeros(2, 5), attention_mask=am), RuntimeError),
    }
    path = os.path.join(ROOT, "tests", "golden", "transformer_embedding_reference.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path))
    print(out["messages"])
    print({k: v for k, v in out["facts"].items() if k.startswith(("param", "head", "second"))})


if __name__ == "__main__":
    main()
