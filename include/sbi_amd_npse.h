/* sbi_amd_npse.h -- C ABI of the MI355X-native NPSE (neural posterior score estimation) path.
 *
 * The score network of sbi's NPSE is the vector-field MLP of the FMPE path (include/sbi_amd_fmpe.h): parameter count,
 * flat parameter order, packed operand images and the pack call are THOSE (sbi_amd_fmpe_param_count / _param_offset /
 * _packed_floats / _pack on `cfg->net`).  New here is what surrounds the trunk: the SDE-dependent input scaling and
 * output pre-conditioning, the denoising-score-matching loss with its control variate, and the Euler-Maruyama sampler.
 * Plain pointers and sizes only; every pointer is a DEVICE pointer (fp32) unless noted; `stream` is a hipStream_t.
 *
 * What each entry point replaces in the reference (file:line under sbi/):
 *   sbi_amd_npse_score           ConditionalScoreEstimator.forward   neural_nets/estimators/score_estimator.py:149-215
 *                                and, with `ode` != 0, ConditionalScoreEstimator.ode_fn  :511-528
 *   sbi_amd_npse_loss            ConditionalScoreEstimator.loss (validation: no gradient)  :230-316
 *   sbi_amd_npse_loss_fwd_bwd    the same loss + loss.backward() of the training loop
 *                                inference/trainers/vfpe/base_vf_inference.py:443-470, trainers/base.py:1160-1190
 *   sbi_amd_npse_sample_sde      Diffuser.run with the euler_maruyama predictor and no corrector
 *                                samplers/score/diffuser.py:124-172, samplers/score/predictors.py:112-120
 *
 * N iid observations (the fnpe / gauss / auto_gauss score composition and its sampler) have a header of their own:
 * include/sbi_amd_npse_iid.h.
 *
 * SDE families (mean_t_fn m(t), std_fn s(t), drift f(theta, t), diffusion g(t); score_estimator.py:582-641, 695-769,
 * 905-975), with B = beta_max - beta_min, beta(t) = beta_min + B t, sigma(t) = sigma_min (sigma_max / sigma_min)^t:
 *   0 ve     m = 1                                   s = sigma(t)           f = 0                 g = sigma(t) sqrt(2 ln(sigma_max / sigma_min))
 *   1 vp     m = exp(-B t^2 / 4 - beta_min t / 2)    s = sqrt(1 - m^2)      f = -beta(t) theta/2  g = sqrt(beta(t))
 *   2 subvp  m as vp                                 s = 1 - m^2            f = -beta(t) theta/2  g = sqrt(beta(t) (1 - m^4))
 * With mu = m mean_0 and var = m^2 std_0^2 + s^2 the network sees ((theta_t - mu) / sqrt(var), standardised x, time
 * feature s(t)) and  score = -(m / s) net - (theta_t - mu) / var.
 * zstats keeps the FMPE layout: mean_0 [D], std_0 [D], x mean [C], x std [C].
 */
#ifndef SBI_AMD_NPSE_H
#define SBI_AMD_NPSE_H
#include <stdint.h>
#include "sbi_amd_fmpe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_npse_config {
  sbi_amd_fmpe_config net; /* the score network; noise_scale is unused */
  int32_t sde;             /* 0 ve, 1 vp, 2 subvp */
  int32_t weight;          /* loss weight over time: 0 identity, 1 max_likelihood (g^2), 2 variance (s^2) */
  float beta_min, beta_max;   /* vp / subvp */
  float sigma_min, sigma_max; /* ve */
  float cv_threshold;      /* the control variate applies to rows with s(t) < cv_threshold; <= 0: no control variate */
  float t_min, t_max;      /* time range of the diffusion (informational: times arrive as arrays) */
} sbi_amd_npse_config;

/* out[n][D] = score at (theta_t[n][D], x, times), or with ode != 0 the probability-flow right-hand side
 * f - g^2 score / 2.  x has x_rows rows (1 = one observation for every row, else n); times has t_rows entries (1 or n). */
int sbi_amd_npse_score(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats, const float* theta_t,
                       const float* x, int64_t x_rows, const float* times, int64_t t_rows, int64_t n, int32_t ode,
                       float* out, void* stream);

/* loss_out[n] = weight(t_i) * ( sum_f (score(m theta + s eps) + eps / s)^2  +  [s < cv_threshold] * control variate )
 * for theta[n][D], x, times[n], eps[n][D] ~ N(0, I) (the draw ConditionalScoreEstimator.loss makes internally). */
int sbi_amd_npse_loss(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats, const float* theta,
                      const float* x, int64_t x_rows, const float* times, const float* eps, int64_t n,
                      float* loss_out, void* stream);

/* Workspace (floats) for one training pass over n rows (activation stash of both forward passes, gradient partials). */
int64_t sbi_amd_npse_train_workspace_floats(const sbi_amd_npse_config* cfg, int64_t n);

/* Per-row losses and grad_out[param_count] = d/dparams sum_i w_i loss_i, with w_i = row_weight[i] if
 * row_weight != NULL else uniform_weight (1/n for the mean loss).  Deterministic (fixed-order reductions). */
int sbi_amd_npse_loss_fwd_bwd(const sbi_amd_npse_config* cfg, const float* params, const float* packed,
                              const float* zstats, const float* theta, const float* x, int64_t x_rows,
                              const float* times, const float* eps, int64_t n, const float* row_weight,
                              float uniform_weight, float* loss_out, float* grad_out, float* workspace, void* stream);

/* theta_out[n][D] = end point of `steps` Euler-Maruyama steps of the reverse SDE over the time grid ts[0..steps]
 * (decreasing; steps >= 0), in ONE launch:
 *   theta <- mean_base + std_base * z_0;   for k = 1..steps, at t = ts[k-1], dt = ts[k-1] - ts[k]:
 *   theta <- theta - (f - (1 + eta^2) / 2 g^2 score) dt + eta g sqrt(dt) z_k.
 * base[2 D] = mean_base, std_base.  noise: NULL, or (steps + 1, n, D) standard-normal draws z_k (then the result is a
 * pure function of the arguments).  With NULL, z comes from Philox4x32-10 keyed by `seed`, counter = (row, row >> 32,
 * k, 4-dim block), Box-Muller: the draws of a row depend on (seed, row + row_offset, k, dim) only.
 * Returns SBI_AMD_E_UNSUPPORTED for steps > 65535 (the caller falls back to a loop over sbi_amd_npse_score). */
int sbi_amd_npse_sample_sde(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats,
                            const float* base, const float* x, int64_t x_rows, const float* ts, int32_t steps,
                            float eta, const float* noise, uint64_t seed, int64_t row_offset, int64_t n,
                            float* theta_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
