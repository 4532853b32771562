/* sbi_amd_npse_iid.h -- C ABI of NPSE with N iid observations: the compositional score and its SDE sampler.
 *
 * Companion of include/sbi_amd_npse.h (configuration struct, packed images, zstats layout, SDE families, Philox
 * keying and the `noise` replay contract are THOSE).  What the entry points replace in the reference (file:line under
 * sbi/): IIDScoreFunction.__call__ of FactorizedNPEScoreFunction, GaussCorrectedScoreFn and AutoGaussCorrectedScoreFn
 * (inference/potentials/vector_field_adaptor.py:725-1270) inside Diffuser.run (samplers/score/diffuser.py:124-172).
 *
 * Under a Gaussian prior everything in the composed score except the per-observation scores
 * s_i = score(theta, t | x_i) is independent of theta, so the caller tabulates it (in fp64, once per call) and the
 * kernels evaluate, for the step k that sits at t = ts[k-1],
 *     score_k(theta) = Linv_k ( C_k sum_i s_i + sum_i Lam_i s_i ) + A_k theta + b_k
 * with row-major fp32 tables: lam [N][D][D] (NULL = all zero), step_mats [steps][3][D][D] = (Linv_k, C_k, A_k) and
 * step_vecs [steps][D] = b_k.  The sums over observations run in the order i = 0..N-1 without atomics; a row's result
 * depends on neither n nor the tile it falls into.
 *
 * Envelope of the fused kernels: D <= 16 (every table is one 16x16 MFMA tile) and 1 <= N <= 1024.  Outside of it the
 * entry points return SBI_AMD_E_UNSUPPORTED and the caller composes per-step launches of sbi_amd_npse_score.
 * workspace: sbi_amd_npse_iid_workspace_floats(cfg, N) floats (the condition half of the merge layer per observation,
 * written by a small prologue kernel of the same call).
 */
#ifndef SBI_AMD_NPSE_IID_H
#define SBI_AMD_NPSE_IID_H
#include <stdint.h>
#include "sbi_amd_npse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of workspace for N observations, or a negative error (SBI_AMD_E_UNSUPPORTED outside the envelope). */
int64_t sbi_amd_npse_iid_workspace_floats(const sbi_amd_npse_config* cfg, int64_t N);

/* out[n][D] = composed score at (theta_t[n][D], time[0]) given x[N][C]; mats [3][D][D] and vec [D] are the tables of
 * that one time.  `time` is a device pointer to one float. */
int sbi_amd_npse_score_iid(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats,
                           const float* theta_t, const float* x, int64_t N, const float* time, const float* lam,
                           const float* mats, const float* vec, int64_t n, float* workspace, float* out, void* stream);

/* theta_out[n][D] = end point of `steps` Euler-Maruyama steps over ts[0..steps], all steps in one launch: the update of
 * sbi_amd_npse_sample_sde with score replaced by score_k.  base[2 D] = mean_base, std_base (the caller applies fnpe's
 * 1/sqrt(N)).  noise: NULL or (steps + 1, n, D); with NULL the draws of a row depend on (seed, row + row_offset, k, dim)
 * only.  Returns SBI_AMD_E_UNSUPPORTED for steps > 65535. */
int sbi_amd_npse_sample_sde_iid(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats,
                                const float* base, const float* x, int64_t N, const float* ts, int32_t steps, float eta,
                                const float* lam, const float* step_mats, const float* step_vecs, const float* noise,
                                uint64_t seed, int64_t row_offset, int64_t n, float* workspace, float* theta_out,
                                void* stream);

/* out[n][D] = Linv (C sum_i s_i + sum_i Lam_i s_i) + A theta + b from per-observation scores s[n][N][D] (the host-loop
 * leg: any D <= 128, any N).  mats [3][D][D], vec [D], lam [N][D][D] or NULL.  Every sum runs sequentially in index order
 * inside one row's block, so a row's result is bit-identical whatever n is and wherever the row sits. */
int sbi_amd_npse_compose_iid(const float* s, const float* theta, const float* lam, const float* mats, const float* vec,
                             int64_t n, int64_t N, int32_t D, float* out, void* stream);

/* out[n][D] = the standard-normal draws z_k (k = 0: the start, k >= 1: step k) that both samplers make for rows
 * row_offset .. row_offset + n - 1 under `seed`: lets a host loop over score launches follow the same noise as the
 * fused kernels, and keeps its samples independent of how the rows are split into calls.  Any k >= 0. */
int sbi_amd_npse_sde_normals(uint64_t seed, int64_t row_offset, int32_t k, int64_t n, int32_t D, float* out,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
