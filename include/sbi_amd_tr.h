/* sbi_amd_tr.h -- C ABI of the MI355X-native TransformerEmbedding (sbi/neural_nets/embedding_nets/transformer.py) in
 * series mode with the gated MLP feed-forward block: x (B, T) or (B, T, F) -> out (B, E).
 *
 * Sizes.  F = feature_space_dim, H = num_attention_heads, KV = num_key_value_heads, hd = head_dim (H hd == F),
 * I = intermediate_size, L = num_hidden_layers, E = final_emb_dimension, OP = (H + 2 KV) hd, N = B T tokens.
 *   h_0[n]     = x[n] w_sp + b_sp (scalar series) or x[n, :]
 *   per block:   u = w_1 * h / sqrt(mean(h^2) + eps);   (q | k | v) = Wqkv u, split per head
 *                rotary:      q[d] <- q[d] cos(a_d) + rot(q)[d] sin(a_d),  a_d = t / div_term[d mod hd/2],
 *                             rot(q) = (-q[hd/2:], q[:hd/2]); k likewise
 *                positional:  q[2 i] += cos(t / div_term[i]), q[2 i + 1] += sin(t / div_term[i]); k likewise
 *                S = q k^T / sqrt(hd) (keys <= the query when causal), P = softmax(S) * keep / (1 - p),
 *                h' = h + Wo (P v);   u' = w_2 * h' / sqrt(mean(h'^2) + eps);   (gate | up) = Wgu u'
 *                h'' = h' + Wd (up * act(gate))
 *   out[b]     = Wagg (w_n * h_L[b, T-1] / sqrt(mean(.^2) + eps)) + b_agg
 * div_term is the module's own fp32 buffer (hd / 2 values), passed in the config: the angle is the correctly rounded
 * fp32 quotient t / div_term, its sine and cosine full-precision sincosf.
 *
 * Flat fp32 parameters in state_dict order: scalar_projection.weight (F, 1), .bias (F) (always present, unused for a
 * (B, T, F) input); per layer self_attn.o_proj.weight (F, F), self_attn.qkv_proj.weight (OP, F),
 * ffn.gate_up_proj.weight (2 I, F), ffn.down_proj.weight (F, I), input_layernorm.weight (F),
 * post_attention_layernorm.weight (F); norm.weight (F); aggregator.weight (E, F), aggregator.bias (E).
 * 6 L + 5 entries.
 *
 * Mapping (plain fp32 VALU kernels; see DESIGN.md 7v for why not MFMA yet).
 *   - Linear parts: one workgroup (256 threads) per tile of TR_TOK = 8 consecutive tokens of the flat (B T) index;
 *     every long sum is four interleaved chains (index mod 4, each ascending) joined as (c0 + c1) + (c2 + c3); one
 *     token never sees another one's values.
 *   - Attention: one wave per (b, head, query); the scores of the row live in LDS; max, then sum over the keys in
 *     lane-strided order with a fixed xor tree, then P v over the keys as four chains.  Grouped heads read the shared k / v.
 *   - Dropout: the keep decision of (layer, b, head, q, k) is word k & 3 of Philox-4x32-10 with key = seed and counter
 *     (k >> 2, q, b, layer H + head); kept when the uniform is >= p.
 *   - Forward: input kernel, then per block norm+qkv, attention, block tail; one final kernel on the last tokens.
 *   - Backward: final kernel, then per block in reverse: tail backward, attention backward (dq with D = sum_k P dP,
 *     taken as the P-weighted mean of dP around key 0's so that a one-key row gives dP - D = 0 exactly, dP = dO . v
 *     summed in fp64 and rounded once; then dk / dv
 *     per key, the query heads of a shared head as four chains), qkv backward.  Probabilities are rebuilt as
 *     exp(S - lse), the norms and the gated activation inside the tile.
 *   - Weight gradients: workgroup g of G = ceil(tiles / ceil(tiles / TR_MAX_PARTIALS)) walks a contiguous range of
 *     tiles and adds each tile's product into its own partial image in the workspace (thread-owned elements, no
 *     atomics); a second kernel adds the at most TR_MAX_PARTIALS = 256 partials as four chains over the workgroups;
 *     norm.weight and the aggregator's gradients are four chains over the sequences.
 *
 * Semantics.  No float atomics: every sum has an order fixed by (config, B, T).  A sequence's output row is bitwise the
 * same alone, anywhere in a batch and at any B (with dropout: at the same batch index and seed).  Two backward calls
 * give identical bits.  A NaN or Inf value stays in its own sequence's row.  No d/dx.
 *
 * Envelope: F <= 128; hd even, 2 <= hd <= 64; H hd == F; KV divides H; 1 <= I <= 512; 1 <= L <= 8; 1 <= E <= 128;
 * 1 <= T <= 4096; B T max(F, 2 I) < 2^31; pos_emb in {0 rotary, 1 positional, 2 none}; activation in {0 gelu (exact
 * erf), 1 relu}; is_causal, scalar_input in {0, 1}; 0 <= dropout_p < 1.  Outside it SBI_AMD_E_UNSUPPORTED; zero or
 * negative sizes and null pointers SBI_AMD_E_BADARG.
 *
 * LDS per workgroup in floats (TOK = TR_TOK, r1 = TOK):
 *     qkv        TOK (F + OP) + r1                    qkv backward   TOK (4 F + OP) + 2 r1
 *     tail       TOK (3 F + 2 I) + r1                 tail backward  TOK (5 F + 3 I) + 2 r1
 *     attention  4 (T + hd)                           attention backward  4 (2 T + 2 hd)
 * SBI_AMD_E_LDS when one passes 160 KiB (none does inside the envelope).
 *
 * Workspace in floats, with Q = N F, K = N KV hd, S = B H T, LS = 4 Q + 2 K + S:
 *     inference  LS                       (h, q, k, v, attention output, lse: one block's, reused)
 *     training   L LS + Q                 (the stash: per block its input, q, k, v after the position term, the
 *                                          attention output, lse and the post-attention stream; the last block's output)
 *                + 3 Q + 2 K + S + 2 B F  (backward: d h, d O, d q, d k, d v, D, the final norm's rows)
 *                + G (PL + 2 F)           (weight-gradient partials; PL = one block's parameters)
 * The forward of a call that needs gradients runs with training = 1 on the workspace the backward is given.
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.
 */
#ifndef SBI_AMD_TR_H
#define SBI_AMD_TR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBI_AMD_TR_MAX_PARTIALS 256
#define SBI_AMD_TR_TOK 8

typedef struct sbi_amd_tr_config {
  int32_t feature_space_dim;
  int32_t num_attention_heads;
  int32_t num_key_value_heads;
  int32_t head_dim;
  int32_t intermediate_size;
  int32_t num_hidden_layers;
  int32_t final_emb_dimension;
  int32_t pos_emb;      /* 0 rotary, 1 positional, 2 none */
  int32_t activation;   /* 0 gelu, 1 relu */
  int32_t is_causal;
  int32_t scalar_input; /* 1: x is (B, T); 0: x is (B, T, F) */
  float rms_norm_eps;
  float div_term[32]; /* the position encoder's buffer, head_dim / 2 values */
} sbi_amd_tr_config;

/* Host only.  Number of flat parameters P, or SBI_AMD_E_*.  `offsets` (HOST pointer, may be null) receives
 * 6 num_hidden_layers + 5 entries, the offset of every state_dict entry in order. */
int64_t sbi_amd_tr_param_count(const sbi_amd_tr_config* cfg, int64_t* offsets);

/* Host only.  0 or SBI_AMD_E_*.  lds_bytes (HOST pointer, may be null) receives 6 entries: qkv, attention, tail, tail
 * backward, attention backward, qkv backward.  key_tile: the keys one wave takes per step (64).  partials: G. */
int sbi_amd_tr_plan(const sbi_amd_tr_config* cfg, int64_t B, int64_t T, int32_t* lds_bytes, int32_t* key_tile,
                    int32_t* partials);

/* Host only.  Bytes of workspace (see above), or SBI_AMD_E_*. */
int64_t sbi_amd_tr_workspace_bytes(const sbi_amd_tr_config* cfg, int64_t B, int64_t T, int32_t training);

/* x[b, t(, f)] at x[b x_batch_stride + t x_time_stride (+ f)], strides in floats.  out (B, E).  training = 1 keeps the
 * stash in `workspace` (sbi_amd_tr_workspace_bytes(cfg, B, T, training) bytes). */
int sbi_amd_tr_forward(const sbi_amd_tr_config* cfg, const float* params, const float* x, int64_t x_batch_stride,
                       int64_t x_time_stride, int64_t B, int64_t T, float dropout_p, uint64_t seed, float* out,
                       void* workspace, int32_t training, void* stream);

/* grad_params (P) = d/dparams of sum(out * grad_out), on the workspace a training forward with the same arguments
 * filled. */
int sbi_amd_tr_backward(const sbi_amd_tr_config* cfg, const float* params, const float* x, int64_t x_batch_stride,
                        int64_t x_time_stride, int64_t B, int64_t T, float dropout_p, uint64_t seed,
                        const float* grad_out, float* grad_params, void* workspace, void* stream);

/* keep_u8 (B, H, T, T): the keep decisions of `layer`, through the device function the attention kernels call. */
int sbi_amd_tr_dropout_mask(const sbi_amd_tr_config* cfg, int64_t B, int64_t T, float dropout_p, uint64_t seed,
                            int32_t layer, uint8_t* keep_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif
