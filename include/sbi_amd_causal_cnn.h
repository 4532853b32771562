/* sbi_amd_causal_cnn.h -- C ABI of the MI355X-native causal stack of sbi's CausalCNNEmbedding
 * (sbi/neural_nets/embedding_nets/causal_cnn.py): num_conv_layers x [left zero-pad by dilation[l] (kernel_size - 1) ->
 * Conv1d(kernel_size, dilation[l], stride 1) -> LeakyReLU(negative_slope)], then AvgPool1d(pool_kernel_size: stride =
 * kernel, floor mode).  x (B, in_channels, T) -> pooled (B, out_channels[last], T / pool_kernel_size).  The aggregator
 * behind the pool is not part of it.
 *
 * Sizes.  C_0 = in_channels, C_{l+1} = out_channels[l]; every layer keeps T.  R = sum_l dilation[l] (kernel_size - 1)
 * is the receptive field, H_l = sum_{j >= l} dilation[j] (kernel_size - 1) what is left of it above map l (H_0 = R,
 * H_L = 0).  Flat fp32 parameters in state_dict order: conv 0 weight (C_1, C_0, k), conv 0 bias, conv 1 weight, ...
 *
 * Tiling.  Time is cut into segments of whole pooling windows (max(1, tile_steps / pool_kernel_size) of them); a
 * workgroup owns a (sequence, segment) pair and walks it in tiles [a, b) of at most tile_steps output steps.  For a tile
 * it loads x on [a - R, b) (zero left of t = 0: the causal pad) and keeps map l on [a - H_l, b) in LDS; no per-layer map
 * reaches global memory and only the pooled sums leave the chip.
 *
 * Semantics.
 *   - Convolution is torch's cross-correlation: u[co, t] = b[co] + sum_{ci, j} w[co, ci, j] y[ci, t - (k - 1 - j) d],
 *     y = 0 left of t = 0 in EVERY layer; one fp32 MFMA chain over (ci, j) in that order, the bias added last.
 *   - LeakyReLU(u) = u > 0 ? u : slope u, and LeakyReLU'(0) = negative_slope (the gradient is g where the output is
 *     > 0 and slope g elsewhere, torch's backward).  ReLU is slope 0.
 *   - Every sum, the pool included, has an order fixed by (config, T): a pooled value is the sum of its window's steps
 *     in ascending time, multiplied by 1 / pool_kernel_size once.  No float atomics.  The trailing T mod
 *     pool_kernel_size steps are never read.
 *   - A sequence's pooled row is bitwise the same alone, anywhere in a batch and at any B.
 *   - Backward: every (sequence, segment) tile recomputes its cone [a - R, b), seeds the last layer with grad_pooled /
 *     pool on [a, b) and backpropagates through its own cone; gradients are linear in the seeds, so the tiles'
 *     contributions add up to the full gradient.  A workgroup walks its pairs g, g + G, ... (G = min(pairs, 512)) and
 *     accumulates in LDS; a second kernel adds the G partials in workgroup order.  Two calls give identical bits.
 *   - A NaN or Inf step stays in its own sequence's row and reaches the gradient only through that sequence's terms.
 *   - No d/dx: the backward gives the parameter gradients only.
 *
 * Envelope: 1 <= in_channels <= 32, 1 <= out_channels[l] <= 32, 2 <= kernel_size <= 4, 1 <= num_conv_layers <= 16,
 * 1 <= pool_kernel_size <= T <= 2^20, 1 <= dilation[l] < T, 0 <= negative_slope finite, B in_channels T < 2^31; outside
 * it SBI_AMD_E_UNSUPPORTED.  Zero or negative sizes and null pointers are SBI_AMD_E_BADARG: nothing is launched.
 *
 * LDS.  tile_steps is the largest multiple of 16 (at most 2048) whose backward image fits 160 KiB = 40960 floats.  With
 * K_l = C_l kernel_size and s(n) = n | 1 (an odd row stride), the image in floats is
 *     sum_l C_{l+1} (s(K_l) + 1)                        weights and biases
 *   + sum_l C_{l+1} (K_l + 1)                           gradient accumulators
 *   + sum_{l = 0..L} C_l s(tile_steps + H_l)            every layer's cone map
 *   + max_{l odd} C_l s(tile_steps + H_l) + max_{l even, >= 2} C_l s(tile_steps + H_l)    two gradient maps.
 * The forward keeps two alternating maps instead of all, plus C_L pool sums per window of the segment.
 * SBI_AMD_E_LDS when no tile_steps >= max(16, R) fits: below that more than half of the work is halo recompute.
 *   - sbi's defaults (5 layers of 16 channels, k = 2, dilations 1 2 4 8 16, R = 31): 4400 floats of weights and
 *     accumulators, 2527 of halos, 113 per step: tile_steps = 288 (158332 bytes backward, 49728 forward) at every T.
 *   - the 10-layer cyclic WaveNet setting (16 channels, k = 2, dilations 1 .. 512, R = 1023): the halos alone are
 *     sum_l C_l H_l = 1023 + 16 x 8194 = 132127 floats, more than three times the budget: SBI_AMD_E_LDS, it runs eager.
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.
 */
#ifndef SBI_AMD_CAUSAL_CNN_H
#define SBI_AMD_CAUSAL_CNN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_ccnn_config {
  int32_t in_channels;
  int32_t T;
  int32_t num_conv_layers;
  int32_t out_channels[16];
  int32_t dilation[16];
  int32_t kernel_size;
  int32_t pool_kernel_size;
  float negative_slope;
} sbi_amd_ccnn_config;

/* Host only.  Number of flat parameters P, or SBI_AMD_E_*.  `offsets` (HOST pointer, may be null) receives
 * 2 * num_conv_layers entries: offset of layer l's weight at [2 l], of its bias at [2 l + 1]. */
int64_t sbi_amd_ccnn_param_count(const sbi_amd_ccnn_config* cfg, int64_t* offsets);

/* Host only.  0 and *tile_steps (the time-tile length, a function of cfg without T), *lds_bytes (the backward's dynamic
 * LDS per workgroup), *fwd_lds_bytes (the forward's) for a batch of B sequences, or SBI_AMD_E_BADARG / _UNSUPPORTED /
 * _LDS.  The three are HOST pointers and may be null; on SBI_AMD_E_LDS they describe the 16-step tile that did not
 * fit or fell below R. */
int sbi_amd_ccnn_plan(const sbi_amd_ccnn_config* cfg, int64_t B, int32_t* tile_steps, int32_t* lds_bytes,
                      int32_t* fwd_lds_bytes);

/* Host only.  Bytes of backward workspace, or SBI_AMD_E_*: 512 partials of P floats, whatever T and B. */
int64_t sbi_amd_ccnn_workspace_bytes(const sbi_amd_ccnn_config* cfg, int64_t B);

/* pooled (B, C_L, T / pool) = avg_pool(stack(x (B, in_channels, T))): one launch. */
int sbi_amd_ccnn_forward(const sbi_amd_ccnn_config* cfg, const float* params, const float* x, int64_t B, float* pooled,
                         void* stream);

/* grad_params (P) = d/dparams of sum(pooled * grad_pooled): one launch and the fixed-order reduction.  workspace:
 * sbi_amd_ccnn_workspace_bytes(cfg, B) bytes. */
int sbi_amd_ccnn_backward(const sbi_amd_ccnn_config* cfg, const float* params, const float* x, int64_t B,
                          const float* grad_pooled, float* grad_params, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
