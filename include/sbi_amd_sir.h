/*
 * sbi_amd_sir.h -- C ABI of the MI355X (gfx950) sampling-importance-resampling selection step.
 * Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_nsf.h (device pointers, fp32 row-major,
 * asynchronous on `stream` (a hipStream_t), return 0 / SBI_AMD_E_* / hipError_t).
 *
 * Reference path replaced (pure Python, sbi/samplers/importance/sir.py:49-71): per batch of B rows with K candidates
 * each -- subtract, softmax over the candidates, cumsum, rand, compare, a second cumsum to find the first hit and a
 * boolean-mask gather (which synchronises with the host) -- as ONE launch.
 *
 * Row r:
 *   lw_k = log_p[r K + k] - log_q[r K + k],  m = max_k lw_k.
 *   The row is DEAD if any lw_k is NaN, or m = +inf, or m = -inf (the rows whose softmax is all-NaN in the reference,
 *   where its mask selects nothing): idx[r] = -1, out row r is left untouched, *n_dead is incremented.
 *   Otherwise e_k = exp(lw_k - m) (-inf gives exactly 0), P_k the inclusive prefix of the e_k from a fixed-order scan
 *   (64-candidate chunks: a Hillis-Steele scan inside the chunk, chunk totals carried serially; a lane group narrower
 *   than 64 for K < 64), S = P_{K-1}.  With t = u_r S the winner is the smallest k with P_k > t and e_k > 0; if rounding
 *   leaves none, the largest k with e_k > 0.  (In exact arithmetic "and e_k > 0" is implied by P_k > t >= P_{k-1}; in
 *   fp32 two prefixes of a tree scan can differ in the last bit around a zero weight, and the condition keeps a
 *   candidate of weight zero from ever being selected.)  row_lse[r] = m + log S.
 *
 * Two deliberate departures from the reference's `cumsum(softmax) >= u`: a candidate of weight zero is never selected,
 * and a live row always selects.  Both differ from the reference only for u exactly on a boundary.
 *
 * A row's result depends only on K, D, its inputs and its u: not on B, on the row's place in the grid or on the lanes
 * that process it (no atomics on floats; the only atomic is the integer dead-row counter).
 *
 * Mapping: K <= 64 packs rows into lane groups of width min(64, next_pow2(K)) -- max, sum and scan through cross-lane
 * operations, no LDS, the log-weights read once.  K > 64: one wave per row; the row is staged in LDS while its maximum
 * is taken, so it is read from memory once.  A row must fit one workgroup's LDS: K > 40 960 is SBI_AMD_E_UNSUPPORTED.
 * The winner's D floats are copied by the row's lane group.
 */
#ifndef SBI_AMD_SIR_H
#define SBI_AMD_SIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* log_p (B*K) potential at the candidates; log_q (B*K) proposal log-prob or NULL (= 0); cand (B*K, D) row-major;
 * u (B) uniforms in [0, 1) or NULL: drawn in the kernel as u01(philox4x32_10(counter = (row lo, row hi, 0,
 * 0x53495231), key = (seed lo, seed hi))[0]) with row = r + row_offset (u01(w) = (w >> 8) * 2^-24) -- the stream
 * depends only on the row number; out (B, D) the winners; idx (B) the winner's k in [0, K), -1 for a dead row;
 * row_lse (B) log sum_k w_k or NULL (a dead row gets NaN when it holds a NaN, otherwise its maximum: -inf or +inf);
 * n_dead: one int32 counter that is INCREMENTED (zero it first) or NULL.
 * B == 0 is a no-op; a missing pointer, B < 0, K < 1 or D < 1: SBI_AMD_E_BADARG; K > 40 960: SBI_AMD_E_UNSUPPORTED. */
int sbi_amd_sir_resample(const float* log_p, const float* log_q, const float* cand, int64_t B, int32_t K, int32_t D,
                         const float* u, uint64_t seed, uint64_t row_offset, float* out, int32_t* idx, float* row_lse,
                         int32_t* n_dead, void* stream);

#ifdef __cplusplus
}
#endif
#endif
