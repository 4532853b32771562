// mixture_lse.hip -- pairwise mixture log-sum-exp: out[h, i] = log sum_j exp(log_w_j - 1/2 scale_h |A (q_i - c_j)|^2)
// (Gaussian mode) or log sum_{j: q_i in box(c_j, v)} exp(log_w_j) (box mode), with optional leave-group-out.  One launch
// replaces the per-particle loop of the SMC-ABC weight update, KernelDensity.score_samples and one zoom repetition of
// the KDE bandwidth cross-validation.  Semantics and envelope: include/sbi_amd_abc.h.
//   * 256 threads = 4 waves own 64 queries: lane l of every wave keeps query l (whitened, D registers) and the H running
//     (maximum, sum) pairs in registers.
//   * Centres go through LDS in tiles of 256, one centre per thread, whitened ONCE while staged: z = A (x - c_0).  Wave w
//     walks centres [64 w, 64 w + 64) of the tile; every lane reads the same centre (an LDS broadcast: no conflicts),
//     d^2 is formed once per pair from differences and serves all H scales.
//   * Online max-shifted log-sum-exp; the shifted terms are summed in fp64.  The 4 partial pairs of a query are combined
//     in wave order by wave 0.  Nothing depends on M or on the block index; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_abc.h"

#define MLSE_THREADS 256
#define MLSE_TILE SBI_AMD_MLSE_TILE
#define MLSE_Q SBI_AMD_MLSE_QUERIES
static_assert(MLSE_TILE == MLSE_THREADS && MLSE_Q == 64, "one centre per thread, one query per lane");

template <int DMAX, int HMAX>
struct MlseSmem {
  static constexpr int kTileBytes = MLSE_TILE * DMAX * 4;
  static constexpr int kPartBytes = 3 * HMAX * 64 * 12 + 3 * 64 * 4;   // waves 1..3: fp64 sums, fp32 maxima, bad flags
  static constexpr int kBytes = kTileBytes > kPartBytes ? kTileBytes : kPartBytes;
};

// Rows [r0, r0 + cnt) of src (row-major, D wide) into tile rows [0, cnt), DMAX wide, zero padded.  Gaussian mode:
// z = A (x - off) (A == identity when !has_A), every product chain in feature order.  Box mode: the raw row.
template <int DMAX, bool BOX>
__device__ __forceinline__ void mlse_stage(const float* __restrict__ src, long long r0, int cnt, int D, bool has_A,
                                           const float* __restrict__ s_A, const float* __restrict__ s_off,
                                           float* __restrict__ s_tile, int tid) {
  if (tid >= cnt) return;
  float x[DMAX];
  const float* __restrict__ row = src + (r0 + tid) * D;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) x[d] = d < D ? row[d] : 0.f;
  float* __restrict__ dst = s_tile + tid * DMAX;
  if (BOX) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) dst[d] = x[d];
    return;
  }
#pragma unroll
  for (int d = 0; d < DMAX; ++d) x[d] = d < D ? x[d] - s_off[d] : 0.f;
  if (!has_A) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d) dst[d] = x[d];
    return;
  }
  for (int e = 0; e < DMAX; ++e) {                 // (rows e >= D of s_A are zero)
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) acc = fmaf(s_A[e * DMAX + d], x[d], acc);
    dst[e] = acc;
  }
}

template <int DMAX, int HMAX, bool BOX>
__global__ void __launch_bounds__(MLSE_THREADS)
mlse_kernel(const float* __restrict__ q, long long M, const float* __restrict__ c, long long N, int D,
            const float* __restrict__ log_w, const float* __restrict__ whiten, const float* __restrict__ half_width,
            const float* __restrict__ scale, int H, const int* __restrict__ q_group, const int* __restrict__ c_group,
            float* __restrict__ out) {
  using SM = MlseSmem<DMAX, HMAX>;
  __shared__ __align__(16) unsigned char s_raw[SM::kBytes];
  __shared__ float s_lw[MLSE_TILE];
  __shared__ int s_grp[MLSE_TILE];
  __shared__ float s_A[BOX ? 1 : DMAX * DMAX];
  __shared__ float s_off[DMAX];                    // Gaussian mode: the offset c_0; box mode: the half widths
  float* s_tile = reinterpret_cast<float*>(s_raw);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long qi = (long long)blockIdx.x * MLSE_Q + lane;
  const bool valid = qi < M;
  const bool has_A = !BOX && whiten != nullptr;
  const bool grouped = q_group != nullptr && c_group != nullptr;

  if (tid < DMAX) s_off[tid] = tid < D ? (BOX ? half_width[tid] : c[tid]) : 0.f;
  if (has_A)
    for (int k = tid; k < DMAX * DMAX; k += MLSE_THREADS) {
      const int e = k / DMAX, d = k % DMAX;
      s_A[k] = (e < D && d < D) ? whiten[e * D + d] : 0.f;
    }
  __syncthreads();
  // ---- the block's queries: staged like a centre tile (whitened once), then one row per lane into registers
  {
    const long long left = M - (long long)blockIdx.x * MLSE_Q;
    mlse_stage<DMAX, BOX>(q, (long long)blockIdx.x * MLSE_Q, (int)(left < MLSE_Q ? left : MLSE_Q), D, has_A, s_A, s_off,
                          s_tile, tid);
  }
  __syncthreads();
  float zq[DMAX];
  bool bad = false;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    zq[d] = valid ? s_tile[lane * DMAX + d] : 0.f;
    bad |= (zq[d] != zq[d]);
  }
  const int myg = (grouped && valid) ? q_group[qi] : 0;
  float nh[HMAX], mx[HMAX];
  double sm[HMAX];
#pragma unroll
  for (int h = 0; h < HMAX; ++h) {
    nh[h] = (!BOX && h < H) ? -0.5f * scale[h] : 0.f;
    mx[h] = -INFINITY;
    sm[h] = 0.0;
  }

  for (long long j0 = 0; j0 < N; j0 += MLSE_TILE) {
    const long long left = N - j0;
    const int cnt = (int)(left < MLSE_TILE ? left : MLSE_TILE);
    __syncthreads();                               // (the tile, or the staged queries, have been consumed)
    mlse_stage<DMAX, BOX>(c, j0, cnt, D, has_A, s_A, s_off, s_tile, tid);
    if (tid < cnt) {
      s_lw[tid] = log_w ? log_w[j0 + tid] : 0.f;
      s_grp[tid] = grouped ? c_group[j0 + tid] : 0;
    }
    __syncthreads();
    const int jb = wave * 64, je = jb + 64 < cnt ? jb + 64 : cnt;
    for (int jj = jb; jj < je; ++jj) {
      const float4* __restrict__ zc4 = reinterpret_cast<const float4*>(s_tile + jj * DMAX);
      float lw = s_lw[jj];
      if (grouped && s_grp[jj] == myg) lw = -INFINITY;
      if (BOX) {
        bool in = true;
#pragma unroll
        for (int d4 = 0; d4 < DMAX / 4; ++d4) {
          const float4 v = zc4[d4];
          const float cc[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int d = 4 * d4 + k;
            if (d < D) {
              const float lo = cc[k] - s_off[d], hi = cc[k] + s_off[d];
              in = in && (lo <= zq[d]) && (zq[d] < hi);
            }
          }
        }
        const float t = in ? lw : -INFINITY;
        if (t > mx[0]) {
          sm[0] = sm[0] * (double)expf(mx[0] - t) + 1.0;
          mx[0] = t;
        } else if (t > -INFINITY) {
          sm[0] += (double)expf(t - mx[0]);
        }
        bad |= (lw != lw);
      } else {
        float d2 = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < DMAX / 4; ++d4) {
          const float4 v = zc4[d4];
          const float e0 = zq[4 * d4] - v.x, e1 = zq[4 * d4 + 1] - v.y, e2 = zq[4 * d4 + 2] - v.z,
                      e3 = zq[4 * d4 + 3] - v.w;
          d2 = fmaf(e0, e0, d2);
          d2 = fmaf(e1, e1, d2);
          d2 = fmaf(e2, e2, d2);
          d2 = fmaf(e3, e3, d2);
        }
#pragma unroll
        for (int h = 0; h < HMAX; ++h) {
          if (h < H) {
            const float t = fmaf(nh[h], d2, lw);
            bad |= (t != t);
            if (t > mx[h]) {
              sm[h] = sm[h] * (double)expf(mx[h] - t) + 1.0;
              mx[h] = t;
            } else if (t > -INFINITY) {
              sm[h] += (double)expf(t - mx[h]);
            }
          }
        }
      }
    }
  }

  // ---- combine the 4 waves' partials in wave order (the tile storage is reused)
  __syncthreads();
  double* p_s = reinterpret_cast<double*>(s_raw);                      // [3][HMAX][64]
  float* p_m = reinterpret_cast<float*>(s_raw + 3 * HMAX * 64 * 8);    // [3][HMAX][64]
  int* p_bad = reinterpret_cast<int*>(s_raw + 3 * HMAX * 64 * 12);     // [3][64]
  if (wave > 0) {
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
      p_s[((wave - 1) * HMAX + h) * 64 + lane] = sm[h];
      p_m[((wave - 1) * HMAX + h) * 64 + lane] = mx[h];
    }
    p_bad[(wave - 1) * 64 + lane] = bad ? 1 : 0;
  }
  __syncthreads();
  if (wave == 0 && valid) {
    for (int w = 0; w < 3; ++w) bad |= p_bad[w * 64 + lane] != 0;
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
      if (h < H) {
        float pm[4];
        double ps[4];
        pm[0] = mx[h];
        ps[0] = sm[h];
        for (int w = 0; w < 3; ++w) {
          pm[w + 1] = p_m[(w * HMAX + h) * 64 + lane];
          ps[w + 1] = p_s[(w * HMAX + h) * 64 + lane];
        }
        const float top = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
        float res;
        if (bad) {
          res = __builtin_nanf("");
        } else if (top == -INFINITY) {
          res = -INFINITY;
        } else {
          double S = 0.0;
          for (int w = 0; w < 4; ++w)
            if (pm[w] > -INFINITY) S += ps[w] * (double)expf(pm[w] - top);
          res = (float)((double)top + log(S));
        }
        out[(long long)h * M + qi] = res;
      }
    }
  }
}

template <int DMAX, int HMAX, bool BOX>
static void mlse_launch(unsigned blocks, hipStream_t s, const float* q, long long M, const float* c, long long N, int D,
                        const float* log_w, const float* whiten, const float* half_width, const float* scale, int H,
                        const int* q_group, const int* c_group, float* out) {
  hipLaunchKernelGGL((mlse_kernel<DMAX, HMAX, BOX>), dim3(blocks), dim3(MLSE_THREADS), 0, s, q, M, c, N, D, log_w, whiten,
                     half_width, scale, H, q_group, c_group, out);
}

template <int DMAX>
static void mlse_dispatch_h(bool box, unsigned blocks, hipStream_t s, const float* q, long long M, const float* c,
                            long long N, int D, const float* log_w, const float* whiten, const float* half_width,
                            const float* scale, int H, const int* q_group, const int* c_group, float* out) {
#define MLSE_GO(HM, BX) \
  mlse_launch<DMAX, HM, BX>(blocks, s, q, M, c, N, D, log_w, whiten, half_width, scale, H, q_group, c_group, out)
  if (box) MLSE_GO(1, true);
  else if (H <= 1) MLSE_GO(1, false);
  else if (H <= 4) MLSE_GO(4, false);
  else if (H <= 10) MLSE_GO(10, false);
  else MLSE_GO(16, false);
#undef MLSE_GO
}

extern "C" int sbi_amd_mixture_lse(const float* q, int64_t M, const float* c, int64_t N, int32_t D, const float* log_w,
                                   const float* whiten, const float* half_width, const float* scale, int32_t H,
                                   const int32_t* q_group, const int32_t* c_group, float* out, void* stream) {
  const bool box = half_width != nullptr;
  if (!q || !c || !out || M < 0 || N < 1 || D < 1 || H < 1 || M > 0x7fffffffll || N > 0x7fffffffll)
    return SBI_AMD_E_BADARG;
  if (box ? H != 1 : scale == nullptr) return SBI_AMD_E_BADARG;
  if (D > SBI_AMD_MLSE_MAX_D || H > SBI_AMD_MLSE_MAX_H) return SBI_AMD_E_UNSUPPORTED;
  if (M == 0) return 0;
  const unsigned blocks = (unsigned)((M + MLSE_Q - 1) / MLSE_Q);
  hipStream_t s = (hipStream_t)stream;
#define MLSE_D(DM) \
  mlse_dispatch_h<DM>(box, blocks, s, q, (long long)M, c, (long long)N, D, log_w, whiten, half_width, scale, H, \
                      q_group, c_group, out)
  if (D <= 4) MLSE_D(4);
  else if (D <= 8) MLSE_D(8);
  else if (D <= 16) MLSE_D(16);
  else MLSE_D(32);
#undef MLSE_D
  return (int)hipGetLastError();
}
