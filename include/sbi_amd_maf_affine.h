/*
 * sbi_amd_maf_affine.h -- C ABI of the MI355X (gfx950) affine masked autoregressive flow, sbi's default density
 * estimator "maf" (sbi build_maf, sbi/neural_nets/net_builders/flow.py:115-209).  Same library (libsbi_amd_nsf.so)
 * and the conventions of sbi_amd_maf.h: device pointers, fp32 row-major, asynchronous on `stream`, return
 * 0 / SBI_AMD_E_* / hipError_t, condition row = x[n % x_rows].
 *
 * Per transform the flow applies nflows' MaskedAffineAutoregressiveTransform(features=D, hidden_features=H,
 * context_features=C, num_blocks=NB, use_residual_blocks=False, random_mask=False, activation=tanh) and then
 * RandomPermutation(D).  With (u_d, s_d) = rows (2d, 2d+1) of the MADE's final layer:
 *     scale_d = softplus(u_d) + epsilon,   y_d = scale_d z_d + s_d,   logabsdet = sum_d log scale_d.
 * nflows 0.14 is not importable where this was written: the parity is unpinned at the nflows boundary (same caveat
 * as oracle/maf_oracle.py); `epsilon` travels in the config so that another reading is a one-line change.
 *
 * Flat parameter layout (`params`, nflows' natural order), per transform t = 0..T-1:
 *     autoregressive_net.initial_layer.weight (H, D), .bias (H)        MaskedLinear, hidden degrees
 *     autoregressive_net.context_layer.weight (H, C), .bias (H)        nn.Linear
 *     per block b: autoregressive_net.blocks.b.linear.weight (H, H), .bias (H)   MaskedLinear
 *     autoregressive_net.final_layer.weight (2D, H), .bias (2D)        MaskedLinear, output degrees repeat(1..D, 2)
 * The degree masks are static: sbi_amd_maf_affine_pack folds them into the packed image, the training pass applies
 * them to the weight gradients (masked entries of grad_out are exactly zero).  The packed image holds the final
 * layer de-interleaved as two dense 16-row tiles [scale logits of dims 0..15 | shifts of dims 0..15].
 * `perms`: T x D int32, RandomPermutation._permutation of every transform (forward: out[d] = in[perm[d]]).
 */
#ifndef SBI_AMD_MAF_AFFINE_H
#define SBI_AMD_MAF_AFFINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_maf_affine_config {
  int32_t D;       /* input features (1..16)                  */
  int32_t C;       /* embedded condition features (1..32)     */
  int32_t H;       /* hidden_features (<= 64)                 */
  int32_t T;       /* num_transforms (<= 16)                  */
  int32_t NB;      /* num_blocks: feed-forward blocks (<= 4)  */
  float epsilon;   /* added to softplus(u): 1e-3 in nflows    */
} sbi_amd_maf_affine_config;
/* Outside the envelope every function returns SBI_AMD_E_UNSUPPORTED. */

/* Floats in the flat parameter buffer / in the packed weight image; <0 = SBI_AMD_E_*. */
int64_t sbi_amd_maf_affine_param_count(const sbi_amd_maf_affine_config* cfg);
int64_t sbi_amd_maf_affine_packed_floats(const sbi_amd_maf_affine_config* cfg);
/* Float offset of linear `which` (0 initial, 1 context, 2+b block b, 2+NB final) of transform t; `bias` != 0
 * selects its bias vector. */
int64_t sbi_amd_maf_affine_param_offset(const sbi_amd_maf_affine_config* cfg, int32_t t, int32_t which, int32_t bias);

/* Waves per workgroup (16 rows each) an n-row launch gets, or SBI_AMD_E_*: 8, halved while the rows make fewer than
 * 256 workgroups, then one fewer at a time until the weight image plus the waves' scratch fit 160 KiB of LDS.
 * trials == 0: log_prob, sample and the training pass; != 0: log_prob_trials with n thetas (its scratch also holds
 * the flow states of a block of trials).  Host-side answer, no device call. */
int32_t sbi_amd_maf_affine_plan_waves(const sbi_amd_maf_affine_config* cfg, int64_t n, int32_t trials);

/* flat params (+ the permutations) -> packed image (masked weights in the MFMA operand layout). */
int sbi_amd_maf_affine_pack(const sbi_amd_maf_affine_config* cfg, const float* params, const int32_t* perms,
                            float* packed, void* stream);

/* Flow.log_prob: logp_out[n] = log p(theta_n | x_{n % x_rows}); noise_out (n, D) optional (transform output).
 * One launch: z-scoring, T x [MADE on MFMA -> affine transform in registers -> permutation], base density. */
int sbi_amd_maf_affine_log_prob(const sbi_amd_maf_affine_config* cfg, const float* packed, const float* zstats,
                                const float* theta, const float* x, int64_t n, int64_t x_rows, float* logp_out,
                                float* noise_out, void* stream);

/* Inverse for GIVEN noise: theta_out (n, D) = transform^{-1}(noise | x); logabsdet_out (n) optional.  D conditioner
 * passes per transform (pass i fixes dimension i); the context gate is computed once per transform. */
int sbi_amd_maf_affine_sample(const sbi_amd_maf_affine_config* cfg, const float* packed, const float* zstats,
                              const float* noise, const float* x, int64_t n, int64_t x_rows, float* theta_out,
                              float* logabsdet_out, void* stream);

/* Training pass: loss_out[n] = -log p_n (optional), grad_out (param_count, nflows' order) =
 * d( sum_n w_n loss_n ) / d params with w_n = row_weight[n] (or uniform_weight when row_weight is NULL),
 * grad_theta_out (n, D) optional; grad_x_out (n, C) optional, d loss / d x per row (it needs x_rows == n, else
 * SBI_AMD_E_BADARG; it is accumulated across the per-transform backward launches, which this call enqueues one
 * after the other on `stream`, so the buffer must not be touched by other streams until the call's work is done).
 * Deterministic, no atomics: forward with the per-transform input stash, per
 * transform (last -> first) a row-parallel backward and split-K weight-gradient GEMMs, one fixed-order reduction. */
int64_t sbi_amd_maf_affine_train_workspace_floats(const sbi_amd_maf_affine_config* cfg, int64_t n);
int sbi_amd_maf_affine_loss_fwd_bwd(const sbi_amd_maf_affine_config* cfg, const float* packed, const float* zstats,
                                    const float* theta, const float* x, int64_t n, int64_t x_rows,
                                    const float* row_weight, float uniform_weight, float* loss_out, float* grad_out,
                                    float* grad_theta_out, float* grad_x_out, float* workspace, void* stream);

/* NLE's potential over iid trials: loglik_out[c] = sum_i log q(x_i | theta_c) for the estimator q(x | theta) (cfg is
 * the estimator's own: D is the x dimension, C the theta dimension).  x_trials (num_trials, D) and theta
 * (num_theta, C) are read in place; every term is bit-identical to sbi_amd_maf_affine_log_prob on the pair and the
 * terms are added in trial order in fp32.  The context gate of a transform is computed once per tile of 16 thetas
 * and block of up to 8 trials. */
int sbi_amd_maf_affine_log_prob_trials(const sbi_amd_maf_affine_config* cfg, const float* packed, const float* zstats,
                                       const float* x_trials, int64_t num_trials, const float* theta,
                                       int64_t num_theta, float* loglik_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
