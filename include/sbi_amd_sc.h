/* sbi_amd_sc.h -- C ABI of the MI355X-native SpectralConvEmbedding (sbi/neural_nets/embedding_nets/SC_embedding.py): the
 * Fourier-neural-operator embedding for series on equispaced or arbitrary 1-D grids.  The WHOLE module, from fc0 to
 * fc_last: x (B, in_channels, n_points) [+ positions (B, n_points)] -> out (B, 2 modes out_channels).
 *
 * Sizes.  N = n_points, C = conv_channels, M = modes, L = num_layers.  theta[k, n] = 2 pi k t_n with t_n = n / N on the
 * equispaced grid and t_n = positions[b, n] otherwise.
 *   h_0[n, c]    = fc0.bias[c] + sum_i fc0.weight[c, i] x[i, n]
 *   Xhat[k, i]   = (1 / N) sum_n exp(-i theta[k, n]) h_l[n, i]                 k < M   (truncated forward transform)
 *   Yhat[k, o]   = sum_i Xhat[k, i] W_l[i, o, k]                               complex, per mode
 *   u_l[n, o]    = sum_k Re(exp(+i theta[k, n]) Yhat[k, o]) + sum_i w_l[o, i] h_l[n, i] + b_l[o]
 *   h_{l+1}      = gelu(u_l)                                                   exact erf, l < L
 *   Z[2 k + r, c] = (r ? Im : Re) Yhat_last[k, c]                              from h_L with conv_last
 *   out[(2 k + r) out_channels + o] = fc_last.bias[o] + sum_c fc_last.weight[o, c] Z[2 k + r, c]
 *
 * Flat fp32 parameters in state_dict order, a complex entry as a (re, im) pair: fc0.weight (C, in), fc0.bias (C),
 * conv_layers.l.weights1 (C, C, M, 2) for l < L, then w_layers.l.weight (C, C), w_layers.l.bias (C) for l < L,
 * conv_last.weights1 (C, C, M, 2), fc_last.weight (out, C), fc_last.bias (out).
 *
 * Mapping.  A workgroup (8 waves) owns whole samples b, b + G, ... with G = min(B, 512), forward and backward.  The twiddles are built in LDS
 * once per sample per launch; the dense operator exp(-i theta) never exists in global memory, and no per-layer map does.
 *   - positions: cos / sin(2 pi k t_n) for every (k, n), 2 M (N | 1) floats.  With p = fl(k t) and e = fma(k, t, -p) the
 *     phase fraction is (p - rint(p)) + e: e and the subtraction are exact for |k t| < 2^23 (|t| < 2^17 at M <= 64) and
 *     the addition rounds once, so the fraction is correctly rounded; then sincospif of twice it.
 *     Positions may be unsorted, differ per sample and lie outside [0, 1).
 *   - equispaced: one table cos / sin(2 pi j / N), j < N (2 N floats), indexed with (k n) mod N in integers.
 *   - both transforms and the pointwise convolution are v_mfma_f32_16x16x4_f32 chains with guarded operands (an element
 *     outside the matrix is an exact 0).  Sums over the points (the forward transform, the weight gradients of the
 *     pointwise layers and of fc0) are cut into `parts` contiguous ranges of 4 ceil(N / (4 parts)) points, one chain
 *     each, added in ascending order; parts = max(1, 8 / T1) with T1 = ceil(2 Mp / 16) ceil(C / 16) output tiles,
 *     Mp = 4 ceil(M / 4).  u_l is ONE chain of K = 2 Mp + C (cos rows, sin rows, pointwise), the bias added last.
 *   - the per-mode channel mix, GELU, fc0 and fc_last are VALU; the spectral weights are read through L2.
 *
 * Semantics.
 *   - Every sum has an order fixed by (config, n_points).  No float atomics.
 *   - A sample's output row is bitwise the same alone, anywhere in a batch and at any B.
 *   - Backward: recomputes every layer from x; h_0 and every u_l stay in LDS with two scratch maps (the running
 *     gradient and the layer's input gelu(u_{l-1})).  d Yhat is the un-normalised forward transform of the gradient,
 *     d h the inverse transform of d Xhat / N, dW[i, o, k] = conj(Xhat[k, i]) dYhat[k, o] in torch's convention
 *     (grad = dL/dRe + i dL/dIm).  Parameter gradients accumulate per workgroup in LDS over its samples in ascending
 *     order; a second kernel adds the G partials in workgroup order (compensated).  Two calls give identical bits.
 *   - A NaN or Inf value, or a NaN position, stays in its own sample's row and reaches the gradient only through that
 *     sample's terms.
 *   - No d/dx and no d/d positions.
 *
 * Envelope: 1 <= in_channels, conv_channels, out_channels <= 32, 1 <= modes <= 64, 1 <= num_layers <= 8,
 * 1 <= n_points <= 65535, modes <= n_points / 2 + 1, has_positions in {0, 1}, B in_channels n_points < 2^31; outside it
 * SBI_AMD_E_UNSUPPORTED.  Zero or negative sizes and null pointers are SBI_AMD_E_BADARG: nothing is launched.
 *
 * LDS.  With s(n) = n | 1, Cs = s(C), TW = has_positions ? 2 M s(N) : 2 N, T2 = ceil(C / 16) ceil((max(C, in) + 1) / 16)
 * and P the parameter count, the images in floats are
 *     forward    r4(TW) + 2 r4(N Cs)       + 2 (2 Mp) C + 256 parts T1            + r4(C Cs) + r4(C)
 *     backward   r4(TW) + (L + 3) r4(N Cs) + 3 (2 Mp) C + 256 parts (2 T1 + T2)   + r4(C Cs) + r4(C) + P
 * (r4 rounds up to a multiple of 4; twiddles; maps: h_0, every u_l and two scratch maps in the backward; spectra; the
 * partial sums of the split chains; one pointwise layer's weights and bias; every gradient accumulator).
 * SBI_AMD_E_LDS when the backward image passes 160 KiB = 40960 floats.
 *   - sbi's defaults (C = 5, M = 10, L = 3, one input and one output channel): P = 2106, 7616 floats besides the
 *     twiddles and maps, 30 floats per point of maps: n_points <= 1041 equispaced, <= 666 with positions.
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.
 */
#ifndef SBI_AMD_SC_H
#define SBI_AMD_SC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_sc_config {
  int32_t in_channels;
  int32_t conv_channels;
  int32_t out_channels;
  int32_t modes;
  int32_t num_layers;
  int32_t n_points;
  int32_t has_positions;
} sbi_amd_sc_config;

/* Host only.  Number of flat parameters P, or SBI_AMD_E_* (n_points and has_positions are not looked at).  `offsets`
 * (HOST pointer, may be null) receives 3 num_layers + 5 entries, the offset of every state_dict entry in order. */
int64_t sbi_amd_sc_param_count(const sbi_amd_sc_config* cfg, int64_t* offsets);

/* Host only.  0 and *lds_bytes (the backward's dynamic LDS per workgroup), *fwd_lds_bytes (the forward's), *parts (the
 * number of ranges the sums over the points are cut into) for a batch of B samples, or SBI_AMD_E_BADARG / _UNSUPPORTED /
 * _LDS.  The three are HOST pointers and may be null; on SBI_AMD_E_LDS they describe the image that did not fit. */
int sbi_amd_sc_plan(const sbi_amd_sc_config* cfg, int64_t B, int32_t* lds_bytes, int32_t* fwd_lds_bytes,
                    int32_t* parts);

/* Host only.  Bytes of backward workspace, or SBI_AMD_E_*: min(B, 512) partials of P floats. */
int64_t sbi_amd_sc_workspace_bytes(const sbi_amd_sc_config* cfg, int64_t B);

/* x and positions are strided views, strides in floats: x[b, i, n] at x[b x_batch_stride + i x_channel_stride + n],
 * positions[b, n] at positions[b pos_batch_stride + n] (null and 0 without positions).  out (B, 2 M out_channels). */
int sbi_amd_sc_forward(const sbi_amd_sc_config* cfg, const float* params, const float* x, int64_t x_batch_stride,
                       int64_t x_channel_stride, const float* positions, int64_t pos_batch_stride, int64_t B,
                       float* out, void* stream);

/* grad_params (P) = d/dparams of sum(out * grad_out): one launch and the fixed-order reduction.  workspace:
 * sbi_amd_sc_workspace_bytes(cfg, B) bytes. */
int sbi_amd_sc_backward(const sbi_amd_sc_config* cfg, const float* params, const float* x, int64_t x_batch_stride,
                        int64_t x_channel_stride, const float* positions, int64_t pos_batch_stride, int64_t B,
                        const float* grad_out, float* grad_params, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
