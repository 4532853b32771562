/*
 * sbi_amd_abc.h -- C ABI of the two MI355X (gfx950) kernels behind ABC (MCABC / SMCABC), its KDE and its
 * Wasserstein distance.  Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_nsf.h (device pointers, fp32
 * row-major, asynchronous on `stream` (a hipStream_t), return 0 / SBI_AMD_E_* / hipError_t).
 *
 * ---- sbi_amd_mixture_lse: pairwise mixture log-sum-exp ----------------------------------------------------------
 * Reference paths replaced: the per-particle Python loop of SMCABC._calculate_new_log_weights (one batched
 * MultivariateNormal / BoxUniform and a logsumexp per new particle), KernelDensity.score_samples, and the up to
 * 5 x 10 x 20 fits and scores of the "cv" bandwidth search -- each as ONE launch.
 *
 * Gaussian mode (half_width == NULL):
 *   out[h M + i] = log sum_j exp(log_w_j - 1/2 scale_h |A (q_i - c_j)|^2)
 * over the centres j with c_group[j] != q_group[i] (all centres when either group pointer is NULL).  A = whiten
 * (D x D row-major, NULL = identity).  Every point is whitened ONCE when it is staged, z = A (x - c_0), after the
 * common offset c_0 (the first centre) is subtracted; d^2 = sum_e (z_q,e - z_c,e)^2 from DIFFERENCES, accumulated in
 * feature order with fused multiply-adds (never |a|^2 + |b|^2 - 2 a.b), once per pair for all H scales.
 *
 * Box mode (half_width = v != NULL; H must be 1, scale / whiten ignored):
 *   out[i] = log sum_j exp(log_w_j) over the centres with c_j - v <= q_i < c_j + v in every dimension; the two bounds
 *   are formed in fp32 and then compared (what BoxUniform(c - v, c + v).log_prob does).  Groups apply as above.
 *
 * Both: the log-sum-exp is max-shifted (a running maximum per scale; exponents of -10^4 and below stay finite), the
 * shifted terms are accumulated in fp64.  An empty sum, or log_w_j = -inf for every remaining centre, gives -inf,
 * never NaN.  log_w_j = -inf removes centre j.  A NaN in query i (or a NaN exponent met by query i) makes out[., i]
 * NaN and touches no other query.  The constants -- -sum log diag L - (D/2) log 2 pi, -sum log 2 v, the KDE
 * normalisation -- are the host's.
 *
 * Mapping: a workgroup of 256 threads owns SBI_AMD_MLSE_QUERIES = 64 queries; lane l of each of its 4 waves holds
 * query l in registers together with the H running maxima and sums.  The centres pass through LDS in tiles of
 * SBI_AMD_MLSE_TILE = 256 (whitened while staged); wave w takes centres [64 w, 64 w + 64) of every tile, in order, and
 * the 4 partial (maximum, sum) pairs of a query are combined in wave order.  out[., i] therefore depends only on query
 * i, the centres and N: not on M, not on the query's place in the grid.  No float atomics.
 *
 * Envelope: D <= SBI_AMD_MLSE_MAX_D = 32, H <= SBI_AMD_MLSE_MAX_H = 16; beyond: SBI_AMD_E_UNSUPPORTED.
 *
 * ---- sbi_amd_sinkhorn: persistent batched Sinkhorn ---------------------------------------------------------------
 * Reference path replaced (sbi/utils/metrics.py regularized_ot_dual behind wasserstein_2_squared): up to max_iter
 * iterations of ~15 launches over (B, m, n) temporaries with two host synchronisations each, after an x_o.repeat.
 * Here: one workgroup per problem, the whole iteration on the device, nothing read back, no problem waits for another.
 *
 * Problem p: C_ij = cost[p, i, j], or sum_d (x_id - y_jd)^2 by differences in feature order (fused multiply-adds) with
 * x = x + p * x_batch_stride (0: one x for every problem) and y = y + p n D.  f = g = 0, then per iteration
 *   f_i <- f_i + eps (log a_i - LSE_j((f_i + g_j - C_ij) / eps))         (old g)
 *   g_j <- g_j + eps (log b_j - LSE_i((f_i + g_j - C_ij) / eps))         (new f)
 *   err = max(sum_i |df_i|, sum_j |dg_j|), summed in a fixed order.
 * The problem stops after the first iteration with err < tol (that iteration's update is kept), else after max_iter.
 * iters[p] = the number of iterations executed (tol = 0: exactly max_iter).
 * w[p] = sum_ij exp(-(C_ij - f_i - g_j) / eps) C_ij, accumulated in fp64 in a fixed order.
 * (f_i + g_j - C_ij) / eps is evaluated as ((f_i - C_ij) + g_j) * (1 / eps).
 *
 * Mapping: C sits in LDS with the odd row stride n | 1, so that a half-wave reading one column of 32 consecutive rows
 * (the row pass: one lane group per row) and one reading 32 consecutive columns of a row (the column pass) both hit 32
 * different banks.  A line (row or column) is reduced by a group of G lanes, G the largest power of two with
 * G max(m, n) <= 256: fixed by (m, n) alone, so a problem's result does not depend on B or on its place in the grid.
 *
 * Envelope: the cost matrix, the potentials and the reduction scratch must fit one workgroup's LDS,
 *     m * (n | 1) + 5 * (m + n) + 16 <= SBI_AMD_SINKHORN_LDS_FLOATS = 40 000 floats (156.25 KiB of the CU's 160 KiB).
 * That is more than the 64 KiB a launch gets without opting in: the launcher raises the kernel's dynamic-LDS limit
 * (hipFuncAttributeMaxDynamicSharedMemorySize) on the device that is current.  (m, n) = (100, 100) uses 11 116,
 * (195, 195) 39 991.  Outside it: SBI_AMD_E_UNSUPPORTED, nothing launched.
 */
#ifndef SBI_AMD_ABC_H
#define SBI_AMD_ABC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBI_AMD_MLSE_MAX_D 32
#define SBI_AMD_MLSE_MAX_H 16
#define SBI_AMD_MLSE_TILE 256
#define SBI_AMD_MLSE_QUERIES 64
#define SBI_AMD_SINKHORN_LDS_FLOATS 40000

/* q (M, D) queries; c (N, D) centres; log_w (N) or NULL (= 0); whiten (D, D) or NULL (= I); half_width (D): box mode,
 * NULL: Gaussian mode; scale (H) (Gaussian mode); q_group (M), c_group (N) int32 or NULL; out (H, M).
 * M == 0 is a no-op.  SBI_AMD_E_BADARG (host-side, nothing launched): q, c or out missing, scale missing in Gaussian
 * mode, M < 0, N < 1, D < 1, H < 1, H != 1 in box mode, M or N >= 2^31.
 * SBI_AMD_E_UNSUPPORTED: D > 32 or H > 16. */
int sbi_amd_mixture_lse(const float* q, int64_t M, const float* c, int64_t N, int32_t D, const float* log_w,
                        const float* whiten, const float* half_width, const float* scale, int32_t H,
                        const int32_t* q_group, const int32_t* c_group, float* out, void* stream);

/* x (m, D) per problem, `x_batch_stride` floats apart (0: shared); y (B, n, D); cost (B, m, n) or NULL (then x and y
 * are needed); a (B, m), b (B, n) probability vectors or NULL (uniform); outputs f (B, m), g (B, n), w (B), iters (B),
 * each nullable.  B == 0 is a no-op.  SBI_AMD_E_BADARG: cost == NULL with x or y missing or D < 1, m < 1, n < 1,
 * B < 0 or >= 2^31, x_batch_stride < 0, eps <= 0 or NaN, max_iter < 0, tol negative or NaN.
 * SBI_AMD_E_UNSUPPORTED: m * (n | 1) + 5 * (m + n) + 16 > SBI_AMD_SINKHORN_LDS_FLOATS. */
int sbi_amd_sinkhorn(const float* x, int64_t x_batch_stride, int32_t m, const float* y, int32_t n, int32_t D,
                     const float* cost, const float* a, const float* b, int64_t B, float eps, int32_t max_iter,
                     float tol, float* f, float* g, float* w, int32_t* iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif
