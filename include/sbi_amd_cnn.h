/* sbi_amd_cnn.h -- C ABI of the MI355X-native convolution stack of sbi's CNNEmbedding
 * (sbi/neural_nets/embedding_nets/cnn.py): num_conv_layers x [Conv{1,2}d(kernel_size, stride 1, padding 1, dilation 1)
 * -> ReLU -> MaxPool{1,2}d(pool_kernel_size: stride = kernel, no padding, floor mode)], then a channel-major flatten.
 * The FCEmbedding head behind it is sbi_amd_embed.h's.
 *
 * Sizes.  A conv output extent is n + 3 - kernel_size, a pool output extent is n / pool_kernel_size (floor).  Layer l
 * maps (C_l, n_l...) to (out_channels[l], n_{l+1}...); C_0 = in_channels, n_0 = spatial.  F = out_channels[last] x
 * prod(final extents).  Flat fp32 parameters in state_dict order: conv 0 weight (C_out, C_in, k[, k]), conv 0 bias,
 * conv 1 weight, ...
 *
 * Semantics.
 *   - Convolution is torch's cross-correlation with zero padding: u[co, o] = b[co] + sum_{ci, t} w[co, ci, t] x[ci, o +
 *     t - 1], summed as ONE fp32 fma chain starting at the bias, in the order ci, then the taps in row-major order.
 *   - ReLU'(0) = 0.  A pool tie goes to the first element in row-major window order; a NaN in a window is passed on
 *     (the last NaN of the window is the selected element), as torch does.
 *   - A sample's feature row depends on that sample and the weights only: one workgroup computes it, in an order that
 *     the configuration fixes.  It is bitwise the same alone, anywhere in a batch and at any B.
 *   - Every sum has an order fixed by the shape: no float atomics.  In the backward a workgroup walks its samples b =
 *     g, g + G, ... (G = min(B, 512) workgroups) and adds each sample's weight-gradient terms, pooled position by pooled
 *     position, onto its partial; a second kernel adds the G partials in workgroup order.  Two calls give identical
 *     bits.
 *   - A NaN or Inf in one sample stays in that sample's feature row and reaches the gradient only through that
 *     sample's terms.
 *   - No d/dx: the backward gives the parameter gradients only.
 *
 * Envelope: ndim in {1, 2}, 1 <= in_channels <= 8, 1 <= out_channels[l] <= 32, 1 <= kernel_size <= 7, 2 <=
 * pool_kernel_size <= 4, 1 <= num_conv_layers <= 4, spatial extents <= 2^20, B <= 1024 (one sample per workgroup pays
 * at training batch sizes; at B = 4096 eager torch measured faster, so larger batches are left to it); outside it
 * SBI_AMD_E_UNSUPPORTED.  Zero or negative sizes, null pointers, ndim outside {1, 2} and a stack whose map shrinks to 0
 * anywhere are SBI_AMD_E_BADARG: nothing is launched.  Inside the envelope SBI_AMD_E_LDS when the backward kernel's
 * per-sample image exceeds 160 KiB.  The image, in floats (w = an extent + 2 rounded up to odd is a map's row stride;
 * a 2-D map has extent + 2 rows, a 1-D map one):
 *     P (weights) + sum_l C_l x rows_l x w_l (zero-bordered input map of every layer)       -- the forward's image
 *   + P (gradient accumulators) + sum_l out_channels[l] x pooled_l (selected element of every pool window)
 *   + max_l out_channels[l] x pooled_l (gated gradient) + max_{l >= 1} out_channels[l] x conv_l (dense conv gradient).
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.
 */
#ifndef SBI_AMD_CNN_H
#define SBI_AMD_CNN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_cnn_config {
  int32_t ndim;            /* 1 | 2 */
  int32_t in_channels;
  int32_t spatial[2];      /* (L, unused) or (H, W) */
  int32_t num_conv_layers;
  int32_t out_channels[4];
  int32_t kernel_size;
  int32_t pool_kernel_size;
} sbi_amd_cnn_config;

/* Host only.  Number of flat parameters P, or SBI_AMD_E_*.  `offsets` (HOST pointer, may be null) receives
 * 2 * num_conv_layers entries: offset of layer l's weight at [2 l], of its bias at [2 l + 1]. */
int64_t sbi_amd_cnn_param_count(const sbi_amd_cnn_config* cfg, int64_t* offsets);

/* Host only.  F, the width of a feature row, or SBI_AMD_E_*. */
int64_t sbi_amd_cnn_feature_count(const sbi_amd_cnn_config* cfg);

/* Host only.  0 and *lds_bytes (the backward's dynamic LDS per workgroup), *fwd_lds_bytes (the forward's) for a batch
 * of B samples, or SBI_AMD_E_BADARG / _UNSUPPORTED / _LDS.  lds_bytes, fwd_lds_bytes: HOST pointers, may be null; they
 * are also written on SBI_AMD_E_LDS (saturated at INT32_MAX). */
int sbi_amd_cnn_plan(const sbi_amd_cnn_config* cfg, int64_t B, int32_t* lds_bytes, int32_t* fwd_lds_bytes);

/* Host only.  Bytes of backward workspace for B samples, or SBI_AMD_E_*. */
int64_t sbi_amd_cnn_workspace_bytes(const sbi_amd_cnn_config* cfg, int64_t B);

/* features (B, F) = flatten(stack(x (B, in_channels, spatial...))): one launch, no intermediate map in global memory. */
int sbi_amd_cnn_forward(const sbi_amd_cnn_config* cfg, const float* params, const float* x, int64_t B, float* features,
                        void* stream);

/* grad_params (P) = d/dparams of sum(features * grad_features).  The activations, ReLU masks and pool selections are
 * recomputed from x.  workspace: sbi_amd_cnn_workspace_bytes(cfg, B) bytes. */
int sbi_amd_cnn_backward(const sbi_amd_cnn_config* cfg, const float* params, const float* x, int64_t B,
                         const float* grad_features, float* grad_params, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
