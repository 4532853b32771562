/*
 * sbi_amd_mdn.h -- C ABI of the MI355X (gfx950) mixture-density-network posterior estimator ("mdn").
 * Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_maf.h (device pointers, fp32 row-major,
 * asynchronous on `stream`, return 0 / SBI_AMD_E_* / hipError_t, condition row = x[i % x_rows]).
 *
 * Reference path replaced (pure Python): MixtureDensityEstimator(MultivariateGaussianMDN(...)).log_prob / loss /
 * sample of sbi (neural_nets/estimators/mixture_density_estimator.py, mog.py, net_builders/mdn.py).
 *
 * Network: h = relu(W2 relu(W1 c + b1) + b2), c = (x - mean_x) / std_x; four heads on h: logits (K), means (K*D),
 * unconstrained_diagonal (K*D), upper (K*U, U = D(D-1)/2, absent for D = 1).  Precision factor A_k: upper triangular,
 * diagonal softplus(unconstrained_diagonal) (identity above 20), strict upper triangle in np.triu_indices(D, 1) order.
 *     log N_k = -D/2 log 2pi + sum_i log A_k[i,i] - (|A_k d|^2 + epsilon |d|^2) / 2,   d = z - mu_k,
 *     log p(theta | x) = logsumexp_k(log_softmax(logits)_k + log N_k) - sum log scale,  z = (theta - shift) / scale.
 *
 * Flat parameter layout (`params`, torch order, each weight then bias):
 *     _hidden_net.0 (H, C) | _hidden_net.2 (H, H) | _logits_layer (K, H) | _means_layer (K*D, H)
 *     | _unconstrained_diagonal_layer (K*D, H) | _upper_layer (K*U, H; absent for D = 1)
 * zstats: [shift (D) | scale (D) | mean_x (C) | std_x (C)].
 */
#ifndef SBI_AMD_MDN_H
#define SBI_AMD_MDN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_mdn_config {
  int32_t D;        /* theta features (1..16) */
  int32_t C;        /* embedded condition features (1..64) */
  int32_t H;        /* hidden_features (1..64), two hidden layers */
  int32_t K;        /* num_components (1..16) */
  float epsilon;    /* added to the precision's diagonal (not to the log-determinant); sbi: 1e-4 */
} sbi_amd_mdn_config;

/* Floats in the flat parameter buffer / in the packed image; <0 = SBI_AMD_E_*.  Every entry point answers a
 * configuration outside the envelope above (any of D, C, H, K below 1 or above its bound) with SBI_AMD_E_UNSUPPORTED
 * before anything is launched; a NULL cfg, a negative epsilon, a missing pointer, n < 0 or x_rows < 1 are
 * SBI_AMD_E_BADARG.  n == 0 is a no-op that returns 0 whatever x_rows is (the training pass then zeroes grad_out). */
int64_t sbi_amd_mdn_param_count(const sbi_amd_mdn_config* cfg);
int64_t sbi_amd_mdn_packed_floats(const sbi_amd_mdn_config* cfg);
/* Float offset of linear `which` (0 hidden.0, 1 hidden.2, 2 logits, 3 means, 4 unconstrained_diagonal, 5 upper);
 * `bias` != 0 selects its bias vector.  which = 5 with D = 1: SBI_AMD_E_BADARG. */
int64_t sbi_amd_mdn_param_offset(const sbi_amd_mdn_config* cfg, int32_t which, int32_t bias);

/* flat params -> the image the kernels read: the two hidden layers and a K-row logits tile in the MFMA operand
 * layout, then one slice per component holding its logit, mean, diagonal and upper rows contiguously (R = 1 + 2D + U
 * rows padded to a multiple of 16, row stride 66 floats, then the slice's biases). */
int sbi_amd_mdn_pack(const sbi_amd_mdn_config* cfg, const float* params, float* packed, void* stream);

/* Device version of get_uncorrected_mog for n condition rows: logits_out (n, K) raw (not normalised), means_out
 * (n, K, D), factors_out (n, K, D + U): per component the D diagonal entries (softplus applied) followed by the U
 * strict-upper entries of the precision factor in np.triu_indices(D, 1) order. */
int sbi_amd_mdn_components(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats, const float* x,
                           int64_t n, float* logits_out, float* means_out, float* factors_out, void* stream);

/* logp_out[i] = log p(theta_i | x_{i % x_rows}).  x_rows == 1: every workgroup evaluates the network once and then
 * only the n x K quadratic forms (bit-identical to the paired kernel on repeated rows). */
int sbi_amd_mdn_log_prob(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats, const float* theta,
                         const float* x, int64_t n, int64_t x_rows, float* logp_out, void* stream);

/* theta_out (n, D) = (mu_k + A_k^{-1} zeta_i) * scale + shift, back-substitution.  k = comp[i] (int32) when `comp`
 * is non-NULL, otherwise the number of cumulative softmax weights <= u[i], clamped to K - 1.  zeta: (n, D) N(0, 1). */
int sbi_amd_mdn_sample(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats, const float* u,
                       const int32_t* comp, const float* zeta, const float* x, int64_t n, int64_t x_rows,
                       float* theta_out, void* stream);

/* Training pass: loss_out[i] = -log p_i (optional), grad_out (param_count) = d( sum_i w_i loss_i ) / d params with
 * w_i = row_weight[i] (or uniform_weight when row_weight is NULL), grad_theta_out (n, D) optional.
 * One row-parallel kernel (forward, then per component the head gradient and the back-propagation through the two
 * ReLU layers) leaves per-row layer gradients and activations in the workspace; the weight gradients are split-K
 * (K = rows) MFMA GEMMs into per-chunk partials summed in a fixed order (deterministic, no atomics).
 * Workspace floats, with npad = n rounded up to 512 rows and P(o) = ceil(o / 16):
 *     npad * 3 * 64                                         condition rows, h1, h2
 *   + npad * 16 * (8 + 1 + 2 P(K D) + P(K U))               gradient planes of the hidden layers and the four heads
 *   + (npad / 512) * param_count                            per-chunk partial gradients
 * (each term rounded up to a multiple of 4).  The head-gradient planes are the large term: n x ~(K (1 + 2D + U))
 * floats, 704 per row = 185 MB at 65 536 rows of the defaults. */
int64_t sbi_amd_mdn_train_workspace_floats(const sbi_amd_mdn_config* cfg, int64_t n);
int sbi_amd_mdn_loss_fwd_bwd(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats,
                             const float* theta, const float* x, int64_t n, int64_t x_rows, const float* row_weight,
                             float uniform_weight, float* loss_out, float* grad_out, float* grad_theta_out,
                             float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
