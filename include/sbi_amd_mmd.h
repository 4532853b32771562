/*
 * sbi_amd_mmd.h -- C ABI of the MI355X (gfx950) RBF-kernel two-sample sums behind the misspecification test and the
 * MMD metrics.  Same library (libsbi_amd_nsf.so), same conventions as sbi_amd_nsf.h (device pointers, fp32 row-major,
 * asynchronous on `stream` (a hipStream_t), return 0 / SBI_AMD_E_* / hipError_t).
 *
 * Reference path replaced (pure Python, sbi/diagnostics/misspecification.py:56-86): a loop over n_shuffle shuffles,
 * each a randperm, three cdist calls, an exact median over up to 10^6 distances (read back with .item()) and three
 * exp + mean passes -- as ONE launch for all shuffles, one workgroup per shuffle ("split").
 *
 * Split s:
 *   rows   r_j = pool[src_j], j in [0, M), with src_j = idx[s M + j] if idx != NULL, else
 *          shf_prp(j, N, shf_half_bits(N), key(seed, s + split_offset))  (csrc/shuffle_prp.h; restated in
 *          tests/shuffle_restatement.py), where key is the splitmix64 output function on seed + (t + 1) G:
 *            z = seed + 0x9E3779B97F4A7C15 (t + 1);  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
 *            z = (z ^ z >> 27) 0x94D049BB133111EB;   key = z ^ z >> 31          (all mod 2^64)
 *          Set A = rows [0, n_a), set B = rows [n_a, M).
 *   d^2    = sum_f (a_f - b_f)^2 from DIFFERENCES, accumulated in feature order with fused multiply-adds: translation
 *          invariant, no cancellation (never |a|^2 + |b|^2 - 2 a.b).
 *   bw     = bandwidth[s] if bandwidth != NULL, else max(bw_floor, the LOWER median of a population of P Euclidean
 *          distances: the element of 0-based ascending rank (P - 1) / 2, what torch.median returns).  Population:
 *          median_set 0 = the n_a (M - n_a) cross pairs; 1 = the cross pairs plus the within-A and within-B pairs of
 *          `pair_set`.  The rank is radix-selected (four 8-bit digits, most significant first) on the bit pattern of
 *          d^2 -- non-negative floats order as unsigned integers and sqrt is monotone, so ONE correctly rounded sqrt is
 *          taken at the end.  Exact: ties, duplicate rows and zero distances give the element a sort would give.  The
 *          population is never materialised; every pass recomputes the distances from the rows in LDS.
 *   S_xy   = sum over the pairs of exp(-d^2 / (2 bw^2)), evaluated as exp(-d^2 * (1 / (2 bw^2))).  pair_set 0 = all
 *          ordered within-set pairs, diagonal included (m^2 terms); 1 = the strict lower triangle (m (m - 1) / 2
 *          terms).  S_ab always has all n_a (M - n_a) terms.  bw == 0 gives what the formula gives in fp32: a zero
 *          distance contributes 0 * inf = NaN, every other pair exp(-inf) = 0.
 *   out[4 s .. 4 s + 3] = { bw, S_aa, S_bb, S_ab }.
 *
 * A split that holds a non-finite value (a NaN or an infinity in any of its M rows), or an idx entry outside [0, N),
 * gets NaN in all four outputs; other splits are untouched.
 *
 * out[s] depends only on the split's rows, D, M, n_a and the two flags: not on S, on the split's place in the grid or
 * on where its indices came from.  No float atomics (the histogram uses integer LDS atomics); every thread sums its
 * pairs in a fixed order in fp64, and the 256 partial sums are combined in a fixed tree.
 *
 * Envelope: the split's rows are staged once in LDS with the row stride padded to the odd number D | 1 (lanes that read
 * the same feature of different rows then hit different banks).  The staging budget is
 *     M * (D | 1) <= SBI_AMD_MMD_STAGE_FLOATS = 15 360 floats (60 KiB),
 * which leaves room for the histogram and the reduction scratch below the 64 KiB a launch gets without opting in, and
 * for two workgroups per CU of 160 KiB.  (M, D) = (1000, 10) uses 11 000.  Outside it: SBI_AMD_E_UNSUPPORTED.
 */
#ifndef SBI_AMD_MMD_H
#define SBI_AMD_MMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBI_AMD_MMD_STAGE_FLOATS 15360

/* pool (N, D); idx (S, M) int32 or NULL; bandwidth (S) or NULL; out (S, 4).
 * S == 0 is a no-op.  SBI_AMD_E_BADARG (host-side, nothing launched): pool or out missing, S < 0, S or N >= 2^31,
 * N < 1, D < 1, M < 2, n_a < 1, n_a >= M, a flag outside {0, 1}, bw_floor negative or NaN, idx == NULL with M > N.
 * SBI_AMD_E_UNSUPPORTED: M * (D | 1) > SBI_AMD_MMD_STAGE_FLOATS. */
int sbi_amd_mmd_rbf_splits(const float* pool, int64_t N, int32_t D, const int32_t* idx, uint64_t seed,
                           uint64_t split_offset, int64_t S, int32_t M, int32_t n_a, int32_t pair_set,
                           int32_t median_set, const float* bandwidth, float bw_floor, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
