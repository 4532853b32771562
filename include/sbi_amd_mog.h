/*
 * sbi_amd_mog.h -- C ABI of the MI355X (gfx950) mixture-of-Gaussians algebra behind NPE-A: the analytic proposal
 * correction, and log_prob / sample of an arbitrary mixture that does not come out of the MDN image.
 * Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_mdn.h (device pointers, fp32 row-major, asynchronous
 * on `stream`, return 0 / SBI_AMD_E_* / hipError_t, n == 0 is a no-op).
 *
 * Reference path replaced (pure Python): sbi's `_correct_for_proposal` / `_compute_posterior_logits`
 * (inference/trainers/npe/npe_a.py), `MoG.log_prob` / `MoG.sample` (neural_nets/estimators/mog.py) and the z-score
 * handling of `NPE_A_Posterior._corrected_log_prob` / `_corrected_sample`.
 *
 * A mixture row: logits (M) unnormalised, means (M, D), precisions (M, D, D) symmetric, factors (M, D, D) upper
 * triangular with precision = factor^T factor.
 * Envelope: 1 <= D <= 16, 1 <= M <= 65 536 components per mixture row (M = L K for the correction); anything else is
 * SBI_AMD_E_UNSUPPORTED before a launch.  A missing pointer, a negative count, prop_rows not in {1, B} or
 * mog_rows < 1 is SBI_AMD_E_BADARG.
 * No float atomics anywhere: every output row depends only on its own inputs, so slicing the batch gives
 * bit-identical rows.  (The only atomic is the integer minimum that finds a row's first failed component.)
 */
#ifndef SBI_AMD_MOG_H
#define SBI_AMD_MOG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace sbi_amd_mog_correct needs: the fp64 per-component tables (P m, m^T P m, logdet P) of the B K
 * density and prop_rows L proposal components.  <0 = SBI_AMD_E_*. */
int64_t sbi_amd_mog_correct_workspace_bytes(int64_t B, int32_t K, int32_t L, int32_t D, int64_t prop_rows);

/* p(theta | x) ~ q(theta | x) prior(theta) / proposal(theta), all factors mixtures of Gaussians (Papamakarios &
 * Murray 2016, Eqs. 23-26).  Density rows d_* (B, K, ...), proposal rows p_* (prop_rows in {1, B}, L, ...), optional
 * Gaussian prior (prior_mean (D), prior_prec (D, D); both NULL = uniform prior, its terms omitted).  Component
 * j = l K + k pairs proposal component l with density component k:
 *     S      = P_d - P_p (+ P_0)
 *     m      = (S + eps I)^-1 (P_d m_d - P_p m_p (+ P_0 m_0))
 *     logit  = logit_d - logit_p + (-logdet(S + eps I) - logdet P_p + logdet P_d) / 2
 *              - (m_d^T P_d m_d - m_p^T P_p m_p - m^T S m) / 2                (the last form on the unstabilised S)
 * The subtraction, the Cholesky factorisation, the solves and the quadratic forms run in fp64 (fp32 in and out).
 * Outputs: logits_out (B, M) raw, means_out (B, M, D), prec_out (B, M, D, D) = S + eps I, factor_out (B, M, D, D) its
 * upper Cholesky factor, status (B) int32: 0, or 1 + the first j whose S + eps I is not positive definite (or whose
 * input precisions are not).  A failed component gets zero logit, mean and factor (never a NaN), and touches no
 * other row. */
int sbi_amd_mog_correct(const float* d_logits, const float* d_means, const float* d_prec, int64_t B, int32_t K,
                        const float* p_logits, const float* p_means, const float* p_prec, int64_t prop_rows,
                        int32_t L, int32_t D, const float* prior_mean, const float* prior_prec, float eps,
                        float* logits_out, float* means_out, float* prec_out, float* factor_out, int32_t* status,
                        void* workspace, void* stream);

/* out[i] = logsumexp_j( log_softmax(logits)_j - D/2 log 2pi + sum_c log U_j[c, c] - d^T P_j d / 2 ) - sum log scale,
 * d = (theta_i - shift) / scale - m_j, with the mixture row i % mog_rows.  shift / scale (D) optional: both NULL =
 * identity.  The quadratic form is taken on the difference d.
 * mog_rows == 1 (one observation, many theta): 16-row theta tiles, per component four v_mfma_f32_16x16x4_f32 against
 * the zero-padded P_j streamed through LDS in groups, online log-sum-exp in component order (M is not bounded by
 * LDS).  mog_rows > 1: one wave per row, lanes over the components. */
int sbi_amd_mog_log_prob(const float* logits, const float* means, const float* prec, const float* factors,
                         int64_t mog_rows, int32_t M, int32_t D, const float* theta, int64_t n, const float* shift,
                         const float* scale, float* out, void* stream);

/* theta_out (n, D) = (m_k + U_k^-1 zeta_i) * scale + shift (back-substitution) from the mixture row i % mog_rows.
 * k = comp[i] (int32) when `comp` is non-NULL; otherwise the number of cumulative normalised weights <= u[i], clamped
 * to M - 1 (a zero-weight component is never selected).  The cumulative table of every mixture row is built once per
 * call in fp64 into `cdf_workspace` (mog_rows * M doubles; may be NULL when `comp` is given) and binary-searched per
 * draw. */
int sbi_amd_mog_sample(const float* logits, const float* means, const float* factors, int64_t mog_rows, int32_t M,
                       int32_t D, const float* u, const int32_t* comp, const float* zeta, int64_t n,
                       const float* shift, const float* scale, float* theta_out, void* cdf_workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
