/*
 * sbi_amd_cond.h -- C ABI of the MI355X (gfx950) conditional-density grid kernels behind sbi_amd.analysis.
 * Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_nsf.h (device pointers, fp32 row-major,
 * asynchronous on `stream` (a hipStream_t), return 0 / SBI_AMD_E_* / hipError_t).
 *
 * Reference path replaced (pure Python, sbi/analysis/conditional_density.py `conditional_corrcoeff` and
 * sbi/utils/conditional_density_utils.py `compute_corrcoeff`): for every condition row and every pair of dimensions a
 * `linspace` / `repeat` / `repeat_interleave` grid, one `log_prob` call, about a dozen fp32 reductions and several host
 * reads.  Here a chunk of whole grids is filled by one launch, evaluated by ONE `log_prob` call, and reduced to its
 * correlation coefficients by one launch.
 *
 * Grid numbering: g = c P + p -- condition row c, pair p with the dimensions (d1, d2) = pairs[p].
 *
 * Moments of one grid (R x R cells, cell i R + j at x = axes[d1][j], y = axes[d2][i]):
 *   m = max logp, w = exp(logp - m) in fp32 (-inf gives exactly 0);
 *   xc = x - (axes[d1][0] + axes[d1][R-1]) / 2, yc likewise, in fp64;
 *   S, Sx, Sy, Sxx, Syy, Sxy = sum of w (1, xc, yc, xc^2, yc^2, xc yc) in fp64, in an order fixed by R alone;
 *   vx = Sxx/S - (Sx/S)^2, vy likewise, rho = (Sxy/S - Sx Sy/S^2) / sqrt(vx vy).
 * A grid is DEGENERATE -- rho = NaN -- when it holds a NaN, when m = +-inf, or when vx vy <= 0 (all mass in one cell:
 * both variances are then exactly 0, the products are not contracted into fma).  Its probs are NaN when a NaN or +inf
 * is present, 0 when every cell is -inf, and w otherwise.
 * No other grid is affected.  (The reference returns +-inf or an arbitrary number there.)
 *
 * A grid's outputs depend only on R and its own inputs: not on G, on g0 or on its place in the launch (no atomics).
 *
 * Mapping: R^2 <= 64 packs grids into lane groups of width next_pow2(R^2) (cross-lane butterflies only, no LDS); larger
 * grids take one 256-thread workgroup each: every thread walks its cells 256 apart, the 64 lanes of a wave are folded
 * by a butterfly and the four waves are added in wave order through LDS.  logp is read twice (maximum, then weights);
 * the second pass comes from L2.
 *
 * The host cannot read `pairs` (device memory) without a synchronisation, so the CONTENT of `pairs` is the caller's to
 * validate (sbi_amd.utils.conditional_density_utils does, on its host copy, and raises SBI_AMD_E_BADARG's message).
 * The kernels never index with an unchecked pair: a pair outside [0, D), or one that breaks the mode's rule, turns its
 * grid's rows (fill) or its rho and probs (moments) into NaN.
 */
#ifndef SBI_AMD_COND_H
#define SBI_AMD_COND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cond (C, D) condition rows; axes (D, R) the grid points of every dimension (the host's `linspace`: gathered, never
 * re-derived, so the rows are bit-equal to the eager construction); pairs (P, 2) int32; out: the theta rows of grids
 * g0 ... g1-1, ((g1 - g0) * cells, D) with cells = R^2 (mode 2) or R (mode 1).
 *   mode 2 (d1 != d2): row i R + j of a grid is the condition row with [d1] = axes[d1][j] and [d2] = axes[d2][i];
 *   mode 1 (d1 == d2): row j is the condition row with [d1] = axes[d1][j].
 * g0 == g1 is a no-op.  A missing pointer, D < 1, R < 1, P < 1, a mode other than 1 / 2 or g0 > g1 or g0 < 0:
 * SBI_AMD_E_BADARG; R > 1024 or D > 64: SBI_AMD_E_UNSUPPORTED.  `cond` must hold row (g1 - 1) / P. */
int sbi_amd_cond_grid_fill(const float* cond, const float* axes, const int32_t* pairs, int32_t D, int32_t R, int32_t P,
                           int32_t mode, int64_t g0, int64_t g1, float* out, void* stream);

/* logp (G, R^2) the log-density on grids g0 ... g0+G-1 (only the pair p = g % P of a grid depends on g0); rho (G);
 * probs (G, R^2) or NULL; moments (G, 6) DOUBLE or NULL: S, Sx, Sy, Sxx, Syy, Sxy (NaN for a grid with a NaN or
 * m = +-inf).  G == 0 is a no-op.  A missing pointer, D < 1, R < 1, P < 1, g0 < 0 or G < 0: SBI_AMD_E_BADARG;
 * R > 1024 or D > 64: SBI_AMD_E_UNSUPPORTED. */
int sbi_amd_cond_grid_moments(const float* logp, const float* axes, const int32_t* pairs, int32_t D, int32_t R,
                              int32_t P, int64_t g0, int64_t G, float* rho, float* probs, double* moments,
                              void* stream);

/* out (N, D): out[n] = cond (one row of D floats) with out[n][dims[q]] = theta[n][q], q < k (dims (k) int32, distinct;
 * an entry outside [0, D) is skipped).  N == 0 is a no-op.  A missing pointer, N < 0, D < 1, k < 1 or k > D:
 * SBI_AMD_E_BADARG; D > 1024: SBI_AMD_E_UNSUPPORTED. */
int sbi_amd_cond_expand(const float* cond, const int32_t* dims, const float* theta, int64_t N, int32_t D, int32_t k,
                        float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
