/*
 * sbi_amd_mnle.h -- C ABI of the MI355X (gfx950) mixed discrete / continuous likelihood estimator (MNLE).
 * Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_mdn.h (device pointers, fp32 row-major, asynchronous
 * on `stream`, return 0 / SBI_AMD_E_* / hipError_t, condition row = c[i % c_rows]).
 *
 * Reference path replaced (pure Python): MixedDensityEstimator(CategoricalMassEstimator(CategoricalMADE),
 * NFlowsFlow(build_nsf at x_numel == 1)) of sbi: one continuous column followed by V categorical columns.
 *
 * Discrete part (residual MADE over F = V + 1 features, the first a zero dummy whose outputs are dropped), context
 * cz = (c - mean_c) / std_c, input xin = [0, idx_0 .. idx_{V-1}] (category indices as floats):
 *     h = initial(xin) + relu(context_layer(cz))
 *     per block: t = L1(relu(L0(relu(h)))); h = h + t * sigmoid(block_context(cz))
 *     logits = final(h)[Kmax:], Kmax = max(num_categories); log p_d = sum_v log_softmax(logits[v, :nc_v])[idx_v]
 * degrees: inputs 1..F, hidden i % V + 1, outputs o / Kmax + 1; hidden masks deg_out >= deg_in, final deg_out > deg_in.
 * Continuous part: u = [val_0 .. val_{V-1}, cz] (raw category VALUES), e = relu(Wb relu(Wa u + ba) + bb); per
 * transform h = relu(W0 e + b0), L times h = relu(W1 h + b1) (one shared layer), p = Wf h + bf (3K - 1 spline
 * parameters, width / height logits divided by sqrt(hidden)); z = x' * scale + shift, x' = log x when log_transform,
 * then T rational-quadratic splines with linear tails, standard normal base;
 *     log p_c = -z_T^2 / 2 - log sqrt(2 pi) + sum log|det| + log|scale| - (log x when log_transform).
 *
 * Flat parameter layout (`params`, each weight then bias, torch (out, in) row-major); linear index `which`:
 *     0 initial (Hd, F) | 1 context (Hd, C) | per block b: 2+3b L0 (Hd, Hd), 3+3b L1 (Hd, Hd), 4+3b context (Hd, C)
 *     | 2+3NB final (F*Kmax, Hd) | 3+3NB Wa (E, V+C) | 4+3NB Wb (E, E)
 *     | per transform t, base 5+3NB + t*(L > 0 ? 3 : 2): W0 (Hc, E), [W1 (Hc, Hc) when L > 0], Wf (3K-1, Hc)
 * zstats: [shift, scale, mean_c (C), std_c (C), values_lookup (V x 16, sorted raw values of every variable)].
 */
#ifndef SBI_AMD_MNLE_H
#define SBI_AMD_MNLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_mnle_config {
  int32_t V;                   /* discrete variables (1..4) */
  int32_t num_categories[4];   /* per variable (1..16); entries >= V are ignored */
  int32_t C;                   /* (embedded) theta features (1..64) */
  int32_t discrete_hidden;     /* width of the MADE (1..64) */
  int32_t discrete_blocks;     /* residual blocks (0..4) */
  int32_t embedding;           /* combined_embedding_features (1..64) */
  int32_t hidden;              /* width of the spline-context MLPs (1..64) */
  int32_t num_bins;            /* K in {4, 5, 8, 10, 16} */
  int32_t num_transforms;      /* T (1..16) */
  int32_t context_layers;      /* hidden_layers_spline_context (0..4) */
  int32_t log_transform;       /* the flow sees log(x_cont) */
  float tail_bound;
  float min_bin_width, min_bin_height, min_derivative;
} sbi_amd_mnle_config;

/* Floats in the flat parameter buffer / the packed image; < 0 = SBI_AMD_E_*.  Every entry point answers a
 * configuration outside the envelope above with SBI_AMD_E_UNSUPPORTED before anything is launched; a NULL cfg, a
 * missing pointer, n < 0 or c_rows < 1 are SBI_AMD_E_BADARG.  n == 0 is a no-op (the training pass zeroes grad_out). */
int64_t sbi_amd_mnle_param_count(const sbi_amd_mnle_config* cfg);
int64_t sbi_amd_mnle_packed_floats(const sbi_amd_mnle_config* cfg);
int64_t sbi_amd_mnle_param_offset(const sbi_amd_mnle_config* cfg, int32_t which, int32_t bias);

/* flat params -> the image the kernels read: one stage of three zero-padded 64 x 66 matrices (+ 64 biases each) per
 * residual block / embedding / transform, MADE masks multiplied in, followed by the 0/1 mask of the flat buffer that
 * the weight-gradient kernel applies. */
int sbi_amd_mnle_pack(const sbi_amd_mnle_config* cfg, const float* params, float* packed, void* stream);

/* logp_out[i] = [parts & 1] log p_d(d_i | c_i) + [parts & 2] log p_c(x_i | d_i, c_i); one launch.  d_idx (n, V) int32
 * category indices, d_val (n, V) raw values; logits_out optional (n, V, Kmax), -inf beyond num_categories[v]. */
int sbi_amd_mnle_log_prob(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                          const float* x_cont, const int32_t* d_idx, const float* d_val, const float* c, int64_t n,
                          int64_t c_rows, int32_t parts, float* logp_out, float* logits_out, void* stream);

/* out[j] = sum_t log p(x_t | c_j), t = 0 .. num_trials - 1 summed in that order in fp32: bit-identical to the paired
 * entry point's outputs accumulated in trial order.  Trials (num_trials rows of x_cont / d_idx / d_val) and conditions
 * (num_cond rows) are read in place; workspace: num_trials * num_cond floats. */
int sbi_amd_mnle_log_prob_trials(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                                 const float* x_cont, const int32_t* d_idx, const float* d_val, const float* c,
                                 int64_t num_trials, int64_t num_cond, float* out, float* workspace, void* stream);

/* One launch: V autoregressive passes (category v = first k whose cumulative softmax >= u[i, v], clamped to
 * num_categories[v] - 1), the raw-value lookup, then the inverse spline chain for noise[i].  d_idx_out (n, V) int32,
 * x_cont_out (n). */
int sbi_amd_mnle_sample(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats, const float* u,
                        const float* noise, const float* c, int64_t n, int64_t c_rows, int32_t* d_idx_out,
                        float* x_cont_out, void* stream);

/* Training pass: loss_out[i] = -log p_i (optional), grad_out (param_count) = d(sum_i w_i loss_i) / d params, w_i =
 * row_weight[i] or uniform_weight; grad_cond_out (n, C) optional (needs c_rows == n): d / d c.  A row-parallel kernel
 * leaves layer inputs and per-row layer gradients in the workspace; the weight gradients are the split-K MFMA GEMMs
 * of the MAF path with their fixed-order reduction (deterministic, no atomics), MADE masks applied. */
int64_t sbi_amd_mnle_train_workspace_floats(const sbi_amd_mnle_config* cfg, int64_t n);
int sbi_amd_mnle_loss_fwd_bwd(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                              const float* x_cont, const int32_t* d_idx, const float* d_val, const float* c, int64_t n,
                              int64_t c_rows, const float* row_weight, float uniform_weight, float* loss_out,
                              float* grad_out, float* grad_cond_out, float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
