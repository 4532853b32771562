/* sbi_amd_embed.h -- C ABI of the MI355X-native embedding nets (sbi/neural_nets/embedding_nets: FCEmbedding and
 * PermutationInvariantEmbedding).
 *
 * FC net (FCEmbedding with ReLU, no layer norm): num_layers Linear layers, EACH followed by ReLU (the last one too, as
 * in the reference): in_dim -> hidden -> ... -> hidden -> out_dim.  Flat fp32 parameters in state_dict order:
 * net.0.weight (hidden, in_dim), net.0.bias, net.3.weight, net.3.bias, ..., last weight (out_dim, hidden), last bias.
 *
 * Permutation-invariant net: x (B, T, Dx); a NaN entry reads as 0; a trial (b, t) whose Dx entries are all NaN is
 * masked: it adds exactly +0 to the pooled sum and does not count.  pooled[b] = sum over t, in the order t = 0, 1, ...
 * (one sequential fp32 chain per (b, feature), whatever T, B, the grid or the place of b in the launch), divided by
 * count[b] under aggregation 1 (mean; count 0 gives NaN in that row only).  out = head([pooled | count]).
 *
 * Envelope: 1 <= in_dim <= 64, 1 <= hidden <= 128, 1 <= out_dim <= 64, 2 <= num_layers <= 4, T <= 65535, rows = B T <
 * 2^31 - 64; outside it SBI_AMD_E_UNSUPPORTED.  Inside it SBI_AMD_E_LDS when the padded weight image plus the row tiles
 * exceed 160 KiB.  Zero or negative sizes and null pointers are SBI_AMD_E_BADARG: nothing is launched.
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.  All sums have an order fixed by the shape: results are reproducible
 * bit for bit, no float atomics.
 */
#ifndef SBI_AMD_EMBED_H
#define SBI_AMD_EMBED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_fc_embed_config {
  int32_t in_dim, hidden, out_dim, num_layers;
} sbi_amd_fc_embed_config;

typedef struct sbi_amd_perminv_config {
  sbi_amd_fc_embed_config trial; /* per-trial net: Dx -> trial_net_output_dim */
  sbi_amd_fc_embed_config head;  /* fc_subnet: head.in_dim must equal trial.out_dim + 1 */
  int32_t aggregation;           /* 0 sum, 1 mean */
} sbi_amd_perminv_config;

/* Host only.  Number of flat parameters P, or SBI_AMD_E_*.  `offsets` (HOST pointer, may be null) receives
 * 2 * num_layers entries: offset of layer l's weight at [2 l], of its bias at [2 l + 1]. */
int64_t sbi_amd_embed_param_count(const sbi_amd_fc_embed_config* cfg, int64_t* offsets);

/* Host only.  Bytes of backward workspace for `rows` input rows (rows = B T for the trial net), or SBI_AMD_E_*. */
int64_t sbi_amd_embed_workspace_bytes(const sbi_amd_fc_embed_config* cfg, int64_t rows);

/* Host only.  0 and *waves (waves per workgroup), *lds_bytes (dynamic LDS per workgroup) for B x T rows through this
 * net (T = 1 for a plain FC net), or SBI_AMD_E_BADARG / _UNSUPPORTED / _LDS.  waves, lds_bytes: HOST pointers, may be
 * null. */
int sbi_amd_embed_plan(const sbi_amd_fc_embed_config* cfg, int64_t B, int64_t T, int32_t* waves, int32_t* lds_bytes);

/* out (N, out_dim) = net(x (N, in_dim)). */
int sbi_amd_fc_embed_forward(const sbi_amd_fc_embed_config* cfg, const float* params, const float* x, int64_t N,
                             float* out, void* stream);

/* grad_params (P) = d/dparams, grad_x (N, in_dim; may be null: not computed) = d/dx of sum(out * grad_out).  The
 * activations are recomputed from x.  workspace: sbi_amd_embed_workspace_bytes(cfg, N) bytes. */
int sbi_amd_fc_embed_backward(const sbi_amd_fc_embed_config* cfg, const float* params, const float* x, int64_t N,
                              const float* grad_out, float* grad_params, float* grad_x, void* workspace, void* stream);

/* out (B, head.out_dim); head_in (B, trial.out_dim + 1) = [pooled | count], kept for the backward. */
int sbi_amd_perminv_forward(const sbi_amd_perminv_config* cfg, const float* trial_params, const float* head_params,
                            const float* x, int64_t B, int64_t T, float* out, float* head_in, void* stream);

/* Parameter gradients of both nets.  The trial-net activations are recomputed from x; head_in is the forward's.
 * grad_head_in: (B, trial.out_dim + 1) scratch.  workspace: the larger of sbi_amd_embed_workspace_bytes(&cfg->trial,
 * B T) and sbi_amd_embed_workspace_bytes(&cfg->head, B) bytes. */
int sbi_amd_perminv_backward(const sbi_amd_perminv_config* cfg, const float* trial_params, const float* head_params,
                             const float* x, int64_t B, int64_t T, const float* head_in, const float* grad_out,
                             float* grad_trial_params, float* grad_head_params, float* grad_head_in, void* workspace,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
