/*
 * sbi_amd_vi.h -- C ABI of the MI355X (gfx950) Gaussian variational family of VIPosterior.
 * Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_nsf.h (device pointers, fp32 row-major,
 * asynchronous on `stream` (a hipStream_t), return 0 / SBI_AMD_E_* / hipError_t).
 *
 * Reference path replaced (sbi/samplers/vi/vi_divergence_optimizers.py `DivergenceOptimizer.step` around the
 * potential, with `LearnableGaussian` of vi_utils.py as q): rsample, MultivariateNormal.log_prob, the link transform
 * and its log-det, logsumexp / softmax, the autograd tape back through them, clip_grad_norm_, Adam -- as one `draw`
 * launch before the potential and one `step` launch after it.
 *
 * The family.  phi is ONE flat fp32 vector: [loc (D) | scale_tril (D x D row-major)] for the full-covariance family
 * (only the lower triangle is read, as `.tril()`), [loc (D) | log_scale (D)] for the diagonal one.  L = tril(scale_tril)
 * or diag(exp(log_scale)).  With eps ~ N(0, I):  z = loc + L eps,  theta = T(z),
 *     log q(theta) = -1/2 |eps|^2 - D/2 log(2 pi) - sum_d log L_dd - sum_d log |T'(z_d)|.
 * (A non-positive L_dd makes log q NaN, as MultivariateNormal's does.)
 *
 * The link T acts per dimension.  `link` is a (4, D) fp32 table [kind | a | b | c] or NULL (the identity):
 *     kind 0  affine       theta = a + b z                 log|T'| = log|b|
 *     kind 1  interval     theta = a + b sigma_c(z)        log|T'| = -softplus(-z) - softplus(z) + log b   (b = c - a > 0)
 *     kind 2  lower bound  theta = a + exp(z)              log|T'| = z
 *     kind 3  upper bound  theta = a - exp(z)              log|T'| = z
 * sigma_c is torch's clipped sigmoid (clamped to [FLT_MIN, 1 - FLT_EPSILON]); c is the interval's upper end and the
 * result is kept inside [nextafter(a, +inf), nextafter(c, -inf)], so theta never lands on a boundary.
 *
 * The draws.  eps of (row, dimension block j = d / 4) is Box-Muller on
 *     philox4x32_10(counter = (row lo, row hi, step, 0x56494731 + j), key = (seed lo, seed hi)):
 *     u1 = ((o0 >> 8) + 1) 2^-24, u2 = (o1 >> 8) 2^-24: eps[4j] = sqrt(-2 log u1) cos(2 pi u2), eps[4j+1] = ... sin;
 *     eps[4j+2], eps[4j+3] the same from o2, o3.
 * It depends on (seed, step, row, dimension) alone: not on n, on the row's place in the grid or on the launch.
 */
#ifndef SBI_AMD_VI_H
#define SBI_AMD_VI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBI_AMD_VI_MAX_D 16
#define SBI_AMD_VI_MAX_PARTICLES 65536

#define SBI_AMD_VI_RKL 0
#define SBI_AMD_VI_IW 1
#define SBI_AMD_VI_ALPHA 2
#define SBI_AMD_VI_FKL 3

typedef struct sbi_amd_vi_config {
  int32_t D;                 /* 1..16 */
  int32_t full_cov;          /* 1: scale_tril, 0: log_scale */
  int32_t method;            /* SBI_AMD_VI_* */
  int32_t K;                 /* IW: rows form groups of K consecutive rows (n % K == 0); otherwise ignored */
  int32_t stick_the_landing; /* rKL / IW / alpha */
  int32_t dreg;              /* IW / alpha: squared weights; the caller also sets stick_the_landing (the biased alpha
                                bound and IW); the unbiased alpha bound has no weights to square */
  int32_t unbiased;          /* alpha */
  float alpha;               /* alpha: the Renyi order (!= 1) */
} sbi_amd_vi_config;

/* SBI_AMD_E_UNSUPPORTED outside the envelope (D > 16, more than 65 536 rows per step); SBI_AMD_E_BADARG for D < 1 or
 * n_rows < 1; otherwise 0 and *workspace_bytes = what `step` needs for n_rows rows. */
int sbi_amd_vi_gauss_plan(int32_t D, int64_t n_rows, int64_t* workspace_bytes);

/* Rows r = 0 .. n-1 draw eps of row (r + row_offset): theta (n, D), log_q (n), eps_out (n, D) or NULL.  Any n >= 0. */
int sbi_amd_vi_gauss_draw(int32_t D, int32_t full_cov, const float* phi, const float* link, int64_t n, uint64_t seed,
                          uint32_t step, uint64_t row_offset, float* theta, float* log_q, float* eps_out, void* stream);

/* log q of given theta (n, D): z = T^-1(theta) (the interval kind clamps (theta - a) / b as torch does), eps by forward
 * substitution, the same sum. */
int sbi_amd_vi_gauss_log_prob(int32_t D, int32_t full_cov, const float* phi, const float* link, const float* theta,
                              int64_t n, float* log_q, void* stream);

/*
 * One optimiser iteration on the rows that `draw` produced with the same (phi, link, seed, step) and row_offset 0.
 * One workgroup; eps, z and log q are regenerated from Philox.
 *   p (n): the potential at theta_i.  r (n, D): its gradient with respect to theta; NULL (only) for fKL.
 *   e_i = p_i - log q_i;  J_i = T'(z_i);  h_i = d/dz sum_d log|T'(z_d)|;  b_i = L^-T eps_i;
 *   a_i = J_i * r_i + h_i (+ b_i under stick_the_landing);  with per-row coefficients c_i
 *     grad loc = -sum c_i a_i
 *     grad scale_tril = -tril(sum c_i a_i eps_i^T) - (sum c_i) diag(1 / L_dd)     (strict upper triangle: exactly 0)
 *     grad log_scale_d = -sum c_i a_id eps_id exp(s_d) - sum c_i
 *   (the terms with sum c_i are dropped under stick_the_landing).
 *   rKL: c_i = 1/n; loss = -mean e.
 *   IW: G = n / K groups; c_i = softmax of e over the row's group / G (squared under dreg);
 *       loss = -mean_g (logsumexp_g e - log K).
 *   alpha: beta = 1 - alpha, m = logsumexp(beta e) - log n; c_i = exp(beta e_i - m) / n (squared under dreg);
 *       unbiased: beta = (1 - alpha)^2 (the reference scales the particles by 1 - alpha twice), c_i = beta exp(beta e_i) / n;
 *       loss = -m / (1 - alpha).
 *   fKL: w_i = exp(e_i - max e) / sum; grad loc = -sum w_i b_i; grad scale_tril = -tril(sum w_i b_i eps_i^T) +
 *       diag(1 / L_dd); grad log_scale_d = -sum w_i (eps_id^2 - 1); loss = sum w_i e_i.
 * All sums over rows run in a fixed order (no float atomics): two launches on the same inputs give the same bits.
 * Then clip_grad_norm_(clip_value) (clip_value <= 0: no clipping) and Adam (csrc/adam_math.h, bias corrections from
 * `t` >= 1 as sbi_amd_adam_clip_step computes them) with learning rate lr_t on phi, exp_avg, exp_avg_sq (P = D + D*D or
 * 2 D floats each); ring[t % ring_size] = loss; grad_out (P) or NULL receives the unclipped gradient.
 * Non-finite guard: if the loss or any gradient entry is not finite, phi <- snapshot, both moments <- 0, status[0] += 1
 * and NOTHING else is written.  Otherwise, when t % 50 == 0 and the updated phi is finite: snapshot <- phi,
 * status[1] += 1.  status: 4 int32 -- [0] steps the guard skipped, [1] snapshot refreshes, [2] the `t` of the last step
 * that was applied, [3] unused.  workspace: sbi_amd_vi_gauss_plan bytes.
 */
int sbi_amd_vi_gauss_step(const sbi_amd_vi_config* cfg, const float* p, const float* r, int64_t n, float* phi,
                          float* exp_avg, float* exp_avg_sq, float* snapshot, const float* link, float clip_value,
                          float lr_t, float beta1, float beta2, float eps, int64_t t, uint64_t seed, uint32_t step,
                          float* workspace, float* ring, int32_t ring_size, int32_t* status, float* grad_out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
