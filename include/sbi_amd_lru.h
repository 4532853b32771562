/* sbi_amd_lru.h -- C ABI of the MI355X-native recurrent stack of sbi's LRUEmbedding
 * (sbi/neural_nets/embedding_nets/lru.py; Orvieto et al. 2023): input_layer (Linear input_dim -> hidden_dim), num_blocks
 * x LRUBlock, aggregation over time.  The output_layer behind it is an ordinary linear map and is not part of this ABI.
 *
 * One block, per sequence, with u_t (hidden_dim) its input at step t and S2 = state_dim x (2 if bidirectional else 1):
 *     lambda = exp(-exp(log_nu) + i exp(log_theta)),  gamma = exp(log_gamma)                       (S2 each)
 *     x_t = lambda x_{t-1} + (gamma B) u_t   for the states s < state_dim, ascending t, x_{-1} = 0;
 *     x_t = lambda x_{t+1} + (gamma B) u_t   for the states s >= state_dim (bidirectional), descending t, x_T = 0
 *     y_t = Re(C x_t) + D u_t;  a_t = GELU(y_t) (erf form);  out_t = a_t sigmoid(W a_t + b) + u_t
 * features = mean_t out_t of the last block (aggregation 0) or out_{T-1} (aggregation 1).
 *
 * Flat fp32 parameters in state_dict order, complex tensors through view_as_real (interleaved re, im):
 *     input_layer.weight (H, I), input_layer.bias (H), then per block
 *     log_nu (S2), log_theta (S2), B (S2, H, 2), C (H, S2, 2), D (H), log_gamma (S2), gate weight (H, H), gate bias (H).
 * grad_params has the same layout; the gradient of a complex entry is dL/dRe + i dL/dIm (torch's convention).
 *
 * Semantics.
 *   - A sequence's feature row depends on that sequence, the parameters and T only: one workgroup computes it, 16 time
 *     steps at a time, in an order that the configuration and T fix.  It is bitwise the same alone, anywhere in a batch
 *     and at any B.
 *   - Every sum has a fixed order: no float atomics.  The mean over t is one fp32 chain in ascending t, divided by T.
 *     In the backward a workgroup walks its sequences b = g, g + G, ... (G = min(B, 512)) and adds every 16-step tile's
 *     terms onto its own partial gradient; a second kernel adds the G partials in workgroup order.  Two calls give
 *     identical bits.
 *   - A NaN or Inf in one sequence stays in that sequence's feature row and reaches the gradient only through that
 *     sequence's terms.
 *   - lambda, gamma and gamma B are derived on the device with full-precision expf / sincosf; GELU is the erff form.
 *   - No d/dx: the backward gives the parameter gradients only.  No layer norm, no dropout.
 *
 * Envelope: 1 <= input_dim <= 64, 1 <= hidden_dim <= 128, 1 <= S2 <= 128, 1 <= num_blocks <= 8, 1 <= T <= 65535,
 * B T < 2^31 - 64, aggregation in {0, 1}; outside it SBI_AMD_E_UNSUPPORTED.  Zero or negative sizes and null pointers
 * are SBI_AMD_E_BADARG: nothing is launched.  Inside the envelope SBI_AMD_E_LDS when the backward kernel's image
 * exceeds 160 KiB.  The image in floats, one block resident at a time:
 *     2 S2 (lambda) + 4 S2 H (gamma B and C as real matrices) + H H + 2 H                      -- weights
 *   + 18 x 2 S2 (states of a tile and one halo step either side) + 4 x 16 H (u, y, a, gate)    -- the forward's tiles
 *   + 16 x 2 S2 (state gradients) + 3 x 16 H + 16 I                                            -- backward only.
 * This is tighter than the envelope above at its far corner (H = 128 fits only up to S2 = 17, H = 72 up to S2 = 76).
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.
 */
#ifndef SBI_AMD_LRU_H
#define SBI_AMD_LRU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_lru_config {
  int32_t input_dim;
  int32_t hidden_dim;
  int32_t state_dim;
  int32_t num_blocks;
  int32_t bidirectional;   /* 0 | 1 */
  int32_t aggregation;     /* 0 = mean over t, 1 = last step */
} sbi_amd_lru_config;

/* Host only.  Number of flat parameters P (input layer and blocks), or SBI_AMD_E_*.  `offsets` (HOST pointer, may be
 * null) receives 1 + num_blocks entries: offset of the input layer (0) and of every block's log_nu. */
int64_t sbi_amd_lru_param_count(const sbi_amd_lru_config* cfg, int64_t* offsets);

/* Host only.  0 and *lds_bytes (the backward's dynamic LDS per workgroup), *fwd_lds_bytes (the forward's) for B
 * sequences of T steps, or SBI_AMD_E_BADARG / _UNSUPPORTED / _LDS.  lds_bytes, fwd_lds_bytes: HOST pointers, may be
 * null; they are also written on SBI_AMD_E_LDS. */
int sbi_amd_lru_plan(const sbi_amd_lru_config* cfg, int64_t B, int64_t T, int32_t* lds_bytes, int32_t* fwd_lds_bytes);

/* Host only.  Bytes of workspace for B sequences of T steps (backward != 0: for sbi_amd_lru_backward), or
 * SBI_AMD_E_*.  The block-to-block maps (B, T, H) and the reversed-direction states go through it. */
int64_t sbi_amd_lru_workspace_bytes(const sbi_amd_lru_config* cfg, int64_t B, int64_t T, int32_t backward);

/* features (B, H) from x (B, T, input_dim): 1 + num_blocks launches, whatever T. */
int sbi_amd_lru_forward(const sbi_amd_lru_config* cfg, const float* params, const float* x, int64_t B, int64_t T,
                        float* features, void* workspace, void* stream);

/* grad_params (P) = d/dparams of sum(features * grad_features).  The block inputs are recomputed from x into the
 * workspace and the states from them, tile by tile; 2 num_blocks + 2 launches, whatever T. */
int sbi_amd_lru_backward(const sbi_amd_lru_config* cfg, const float* params, const float* x, int64_t B, int64_t T,
                         const float* grad_features, float* grad_params, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
