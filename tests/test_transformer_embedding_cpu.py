"""TransformerEmbedding without a GPU: the class surface against the recording of the real sbi class
(tests/golden/transformer_embedding_reference.pt), the eager route and the fp64 oracle on every recorded case, routing
reasons on the host, and the host-side answers of the C ABI (parameter image, plan, workspace, envelope)."""
import copy
import ctypes
import inspect
import os

import pytest
import torch

import sbi_amd.neural_nets as NN
from sbi_amd import _lib
from sbi_amd.neural_nets.embedding_nets import transformer as TR
from sbi_amd.neural_nets.embedding_nets.transformer import TransformerEmbedding
from tests import transformer_embedding_oracle as O

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "transformer_embedding_reference.pt"),
                    weights_only=False)
CASES = GOLDEN["cases"]
TOK = 8


def message(fn, kind):
    with pytest.raises(kind) as e:
        fn()
    return str(e.value)


# ---- the class surface ------------------------------------------------------------------------------------------------
def test_signature_defaults_and_config():
    sig = inspect.signature(TransformerEmbedding.__init__)
    params = [p for n, p in sig.parameters.items() if n != "self"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params)
    facts = GOLDEN["facts"]
    assert [p.name for p in params if p.name != "final_emb_dimension"] == list(facts["config_96"])
    given = {p.name: p.default for p in params if p.default is not inspect.Parameter.empty}
    assert given == {k: v for k, v in dict(O.DEFAULTS).items()}
    assert sig.parameters["feature_space_dim"].default is inspect.Parameter.empty
    net = TransformerEmbedding(feature_space_dim=96)
    assert net.config == facts["config_96"] and list(net.config) == list(facts["config_96"])


def test_state_dict_keys_shapes_order_and_buffers():
    facts = GOLDEN["facts"]
    net = TransformerEmbedding(feature_space_dim=96)
    sd = net.state_dict()
    assert list(sd) == facts["keys_96"] and len(sd) == 29
    assert [tuple(v.shape) for v in sd.values()] == facts["shapes_96"]
    assert sum(p.numel() for p in net.parameters()) == facts["param_count_96"] == 448080
    assert [(k, tuple(v.shape)) for k, v in net.named_buffers()] == facts["buffers_96"]
    assert not any("div_term" in k for k in sd)
    assert torch.equal(net.layers[0].self_attn.pos_emb.div_term, facts["div_term_rotary_hd8"])
    pos = TransformerEmbedding(feature_space_dim=96, pos_emb="positional")
    assert torch.equal(pos.layers[0].self_attn.pos_emb.div_term, facts["div_term_positional_hd8"])
    assert not any(k.endswith("bias") for k in sd if k.startswith("layers."))
    for name, case in CASES.items():
        ours = TransformerEmbedding(**case["kwargs"]).state_dict()
        assert list(ours) == list(case["state_dict"]), name
        assert [v.shape for v in ours.values()] == [v.shape for v in case["state_dict"].values()], name


def test_a_recorded_checkpoint_loads_strictly_and_ours_has_the_same_entries():
    for name, case in CASES.items():
        net = TransformerEmbedding(**case["kwargs"])
        result = net.load_state_dict(case["state_dict"], strict=True)
        assert not result.missing_keys and not result.unexpected_keys
        back = net.state_dict()
        assert all(torch.equal(back[k], v) for k, v in case["state_dict"].items()), name


def test_messages_equal_the_recording():
    T, m = TransformerEmbedding, GOLDEN["messages"]
    small = dict(feature_space_dim=24, intermediate_size=8, num_hidden_layers=1)
    vit = dict(small, vit=True, image_size=16, patch_size=4, num_channels=2)
    assert message(lambda: T(feature_space_dim=36, head_dim=3), ValueError) == m["odd_head_dim"]
    assert message(lambda: T(feature_space_dim=36, head_dim=3, pos_emb="positional"), ValueError) \
        == m["odd_head_dim_positional"]
    assert message(lambda: T(feature_space_dim=64), ValueError) == m["heads_divide_features"]
    assert message(lambda: T(feature_space_dim=24, num_key_value_heads=5), ValueError) == m["kv_divide_heads"]
    assert message(lambda: T(feature_space_dim=24, final_emb_dimension=25), ValueError) == m["final_emb"]
    assert message(lambda: T(feature_space_dim=24, mlp_activation="tanh"), ValueError) == m["activation"]
    assert message(lambda: T(feature_space_dim=24, ffn="moe", num_local_experts=2, num_experts_per_tok=3),
                   ValueError) == m["top_k"]
    assert message(lambda: T(**vit)(torch.zeros(2, 3, 16, 16)), ValueError) == m["vit_channels"]
    # heads * head_dim != feature_space_dim constructs, and fails in forward with torch's reshape error
    mism = T(feature_space_dim=24, num_attention_heads=4, num_key_value_heads=4, head_dim=4, num_hidden_layers=1)
    assert message(lambda: mism(torch.zeros(2, 5)), RuntimeError) == GOLDEN["facts"]["head_dim_mismatch_forward"]
    assert mism.kernel_route(torch.zeros(2, 5))[0] is False


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_eager_route_and_the_oracle_reproduce_the_recorded_case(name):
    case = CASES[name]
    net = O.golden_net(TransformerEmbedding, case)
    out = net(case["x"].clone(), attention_mask=case["attention_mask"])
    (out * case["wts"]).sum().backward()
    grad = O.flat_grad(net)
    scale_o, scale_g = case["out"].abs().max().item(), case["grad_flat"].abs().max().item()
    assert out.shape == case["out"].shape and grad.shape == case["grad_flat"].shape
    assert (out - case["out"]).abs().max().item() <= 2e-5 * scale_o
    assert (grad - case["grad_flat"]).abs().max().item() <= 1e-4 * scale_g
    ref_o, ref_g = O.reference(case["state_dict"], case["x"], case["wts"], case["kwargs"],
                               attention_mask=case["attention_mask"])
    assert (ref_o - case["out"].double()).abs().max().item() <= 2e-5 * scale_o
    assert (ref_g - case["grad_flat"].double()).abs().max().item() <= 1e-4 * scale_g


def test_the_written_formula_reproduces_the_recorded_series_cases_and_takes_keep_masks():
    for name, case in CASES.items():
        kw = O.full_config(case["kwargs"])
        if kw["vit"] or kw["ffn"] != "mlp" or case["attention_mask"] is not None:
            continue
        params = list(case["state_dict"].values())
        out = TR.tr_functional(case["x"], params, dict(kw, head_dim=case["kwargs"].get("head_dim")))
        assert (out - case["out"]).abs().max().item() <= 2e-5 * case["out"].abs().max().item(), name
    case = CASES["kv_4_2"]
    kw = O.full_config(case["kwargs"])
    g = torch.Generator().manual_seed(3)
    keep = [torch.rand(3, 4, 20, 20, generator=g) >= 0.5 for _ in range(2)]
    out = TR.tr_functional(case["x"], list(case["state_dict"].values()), kw, keep)
    ref = O.reference(case["state_dict"], case["x"], case["wts"], case["kwargs"], keep_masks=keep)[0]
    assert (out.double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    assert (out - case["out"]).abs().max().item() > 1e-3          # the masks matter


def test_a_second_call_with_the_same_attention_mask_returns_the_first_numbers():
    assert "ambiguous" in GOLDEN["facts"]["second_masked_call"]      # what the real class does on the second call
    case = CASES["mask"]
    net = O.golden_net(TransformerEmbedding, case)
    with torch.no_grad():
        first = net(case["x"], attention_mask=case["attention_mask"])
        second = net(case["x"], attention_mask=case["attention_mask"])
    assert torch.equal(first, second)
    assert (first - case["out"]).abs().max().item() <= 2e-5 * case["out"].abs().max().item()


def test_a_double_module_runs_the_eager_route_in_fp64():
    case = CASES["mask"]
    net = O.golden_net(TransformerEmbedding, case).double()
    for am in (None, case["attention_mask"]):
        out = net(case["x"].double(), attention_mask=am)
        ref = O.reference(case["state_dict"], case["x"], case["wts"], case["kwargs"], attention_mask=am)[0]
        assert out.dtype == torch.float64 and (out - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


def test_routing_reasons_on_the_host_and_exported_symbols():
    net = TransformerEmbedding(feature_space_dim=24, intermediate_size=8, num_hidden_layers=1)
    x = torch.zeros(2, 5)
    assert net.kernel_route(x) == (False, "input is not on a ROCm device")
    assert net.kernel_route(x.double()) == (False, "input is not float32")
    assert net.kernel_route(x, attention_mask=torch.ones(2, 5)) == (False, "attention_mask / position_ids run eager")
    assert net.kernel_route(x, position_ids=torch.arange(5)) == (False, "attention_mask / position_ids run eager")
    net.force_eager = True
    assert net.kernel_route(x) == (False, "force_eager is set")
    moe = TransformerEmbedding(feature_space_dim=24, ffn="moe", num_local_experts=2, num_experts_per_tok=1,
                               num_hidden_layers=1, intermediate_size=8)
    assert moe.kernel_route(x) == (False, 'ffn="moe" runs eager')
    vit = TransformerEmbedding(feature_space_dim=24, vit=True, image_size=8, patch_size=4, num_channels=1,
                               num_hidden_layers=1, intermediate_size=8)
    assert vit.kernel_route(torch.zeros(2, 1, 8, 8)) == (False, "vit=True runs eager")
    for name in ("TransformerEmbedding", "PositionalEncoder", "RotaryEncoder", "IdentityEncoder", "FullAttention",
                 "MLP", "RMSNorm", "MoeBlock", "TransformerBlock", "ViTEmbeddings"):
        assert getattr(NN, name) is getattr(TR, name)
        assert getattr(NN.embedding_nets, name) is getattr(TR, name)
    assert TR.MAX_WORKSPACE_BYTES == 1 << 30
    lib = _lib.load()
    for sym in ("param_count", "plan", "workspace_bytes", "forward", "backward", "dropout_mask"):
        assert hasattr(lib, "sbi_amd_tr_" + sym)


# ---- the host side of the C ABI ---------------------------------------------------------------------------------------
def config(**kw):
    base = dict(feature_space_dim=96)
    base.update(kw)
    final = base.pop("final_emb_dimension", None)
    scalar = base.pop("scalar_input", True)
    cfg = O.full_config(base)
    final = cfg["feature_space_dim"] // 2 if final is None else final
    return TR.tr_config(cfg, final, [1.0] * (cfg["head_dim"] // 2), scalar)


def test_param_count_and_offsets_follow_the_state_dict():
    n, offsets = TR.param_count(config())
    net = TransformerEmbedding(feature_space_dim=96)
    sizes = [v.numel() for v in net.state_dict().values()]
    assert n == 448080 == sum(sizes) and len(offsets) == 29
    assert offsets == [sum(sizes[:i]) for i in range(len(sizes))]
    for name, case in CASES.items():
        kw = O.full_config(case["kwargs"])
        if kw["vit"] or kw["ffn"] != "mlp":
            continue
        net = TransformerEmbedding(**case["kwargs"])
        sizes = [v.numel() for v in case["state_dict"].values()]
        n, offsets = TR.param_count(net.kernel_config(True))
        assert n == sum(sizes) and offsets == [sum(sizes[:i]) for i in range(len(sizes))], name


@pytest.mark.parametrize("kw, B, T", [(dict(), 4, 100), (dict(feature_space_dim=36, num_attention_heads=6,
                                                            num_key_value_heads=3, intermediate_size=17,
                                                            num_hidden_layers=3), 3, 33),
                                      (dict(feature_space_dim=128, num_attention_heads=2, num_key_value_heads=2,
                                            intermediate_size=512, num_hidden_layers=8, final_emb_dimension=128), 5000,
                                       7)])
def test_plan_lds_and_workspace_bytes_equal_the_formulas_of_the_header(kw, B, T):
    cfg = config(**kw)
    rc, lds, key_tile, parts = TR.plan(cfg, B, T)
    F, H, KV, hd, I, L = (cfg.feature_space_dim, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim,
                          cfg.intermediate_size, cfg.num_hidden_layers)
    OP = (H + 2 * KV) * hd
    assert rc == 0 and key_tile == 64
    assert lds == [4 * v for v in (TOK * (F + OP) + TOK, 4 * (T + hd), TOK * (3 * F + 2 * I) + TOK,
                                   TOK * (5 * F + 3 * I) + 2 * TOK, 4 * (2 * T + 2 * hd),
                                   TOK * (4 * F + OP) + 2 * TOK)]
    assert max(lds) <= 160 * 1024
    N = B * T
    tiles = -(-N // TOK)
    per = -(-tiles // 256)
    G = -(-tiles // per)
    assert parts == G <= 256
    Q, K, S = N * F, N * KV * hd, B * H * T
    LS = 4 * Q + 2 * K + S
    PL = F * F + OP * F + 2 * I * F + F * I + 2 * F
    assert TR.workspace_bytes(cfg, B, T, False) == 4 * LS
    assert TR.workspace_bytes(cfg, B, T, True) == 4 * (L * LS + Q + 3 * Q + 2 * K + S + 2 * B * F + G * (PL + 2 * F))


def test_envelope_edges():
    ok = lambda **kw: TR.plan(config(**kw), kw.pop("B", 2), 16)[0]      # noqa: E731
    U, BAD = _lib.E_UNSUPPORTED, _lib.E_BADARG
    assert ok() == 0
    # feature_space_dim 128 / 132, head_dim 64 / 66 and 2, odd head_dim, heads * head_dim != F
    assert ok(feature_space_dim=128, num_attention_heads=2, num_key_value_heads=2) == 0
    assert ok(feature_space_dim=132, num_attention_heads=12) == U
    assert ok(feature_space_dim=66, num_attention_heads=1, num_key_value_heads=1) == U
    assert ok(feature_space_dim=24, num_attention_heads=12) == 0
    assert ok(feature_space_dim=36, num_attention_heads=12, head_dim=3) == U
    assert ok(feature_space_dim=96, head_dim=6) == U
    assert ok(num_key_value_heads=5) == U and ok(num_key_value_heads=4) == 0
    assert ok(intermediate_size=512) == 0 and ok(intermediate_size=513) == U
    assert ok(num_hidden_layers=8) == 0 and ok(num_hidden_layers=9) == U and ok(num_hidden_layers=0) == BAD
    assert ok(final_emb_dimension=128, feature_space_dim=128, num_attention_heads=2, num_key_value_heads=2) == 0
    assert ok(final_emb_dimension=129, feature_space_dim=128, num_attention_heads=2, num_key_value_heads=2) == U
    cfg = config()
    assert TR.plan(cfg, 1, 4096)[0] == 0 and TR.plan(cfg, 1, 4097)[0] == U
    assert TR.plan(cfg, 1, 1)[0] == 0 and TR.plan(cfg, 1, 0)[0] == BAD and TR.plan(cfg, 0, 5)[0] == BAD
    # B T max(F, 2 I) < 2^31 with 2 I = 512
    assert TR.plan(cfg, (2**31 - 1) // (512 * 16), 16)[0] == 0
    assert TR.plan(cfg, (2**31 - 1) // (512 * 16) + 1, 16)[0] == U
    for field, bad in (("pos_emb", 3), ("activation", 2), ("is_causal", 2)):
        cfg = config()
        setattr(cfg, field, bad)
        assert TR.plan(cfg, 2, 16)[0] == U, field
    lib = _lib.load()
    assert lib.sbi_amd_tr_plan(None, 2, 16, None, None, None) == BAD
    # dropout_p outside [0, 1): refused before anything is launched (the pointers are never read)
    cfg = config()
    fake = ctypes.c_void_p(64)
    assert lib.sbi_amd_tr_forward(ctypes.byref(cfg), fake, fake, 16, 1, 2, 16, 1.0, 0, fake, fake, 0, None) == U
    assert lib.sbi_amd_tr_forward(ctypes.byref(cfg), None, fake, 16, 1, 2, 16, 0.5, 0, fake, fake, 0, None) == BAD
    assert lib.sbi_amd_tr_dropout_mask(ctypes.byref(cfg), 2, 16, 0.5, 0, 4, fake, None) == BAD


def test_the_workspace_cap_routes_to_eager(monkeypatch):
    net = TransformerEmbedding(feature_space_dim=96)
    cfg = net.kernel_config(True)
    assert TR.workspace_bytes(cfg, 200, 100, True) < TR.MAX_WORKSPACE_BYTES < TR.workspace_bytes(cfg, 4096, 100, True)
    assert TR.workspace_bytes(cfg, 4096, 100, False) < TR.MAX_WORKSPACE_BYTES

    class OnDevice(torch.Tensor):       # a host tensor that claims a device: only the routing is looked at
        is_cuda = True

    # the measured rule: calls that need gradients lost to eager torch from (64, 100) on at these sizes
    assert TR.MAX_TRAINING_WORK == 64 * 100 * 96 * 4
    for B in (64, 200):
        took, reason = net.kernel_route(torch.zeros(B, 100).as_subclass(OnDevice))
        assert not took and "measured faster" in reason and "transformer_embed_bench.json" in reason
    assert net.kernel_route(torch.zeros(63, 100).as_subclass(OnDevice)) == (True, "kernel")
    with torch.no_grad():
        assert net.kernel_route(torch.zeros(200, 100).as_subclass(OnDevice)) == (True, "kernel")
    monkeypatch.setattr(TR, "MAX_WORKSPACE_BYTES", TR.workspace_bytes(cfg, 4, 50, True))
    fits = torch.zeros(4, 50).as_subclass(OnDevice)
    over = torch.zeros(4, 51).as_subclass(OnDevice)
    assert net.kernel_route(fits) == (True, "kernel")
    took, reason = net.kernel_route(over)
    assert not took and "MAX_WORKSPACE_BYTES" in reason
    with torch.no_grad():                 # nothing to stash: the inference workspace is smaller
        assert net.kernel_route(over) == (True, "kernel")
