// mmd.hip -- the RBF-kernel sums of S independent two-sample problems ("splits") over one pool of rows: the permutation
// baseline of the misspecification test (sbi/diagnostics/misspecification.py:56-86: per shuffle a randperm, three
// cdist, an exact median read back by the host, three exp + mean) as ONE launch.  Semantics: include/sbi_amd_mmd.h.
//   * One workgroup of 256 threads per split.  The split's M rows are gathered once into LDS (row stride D | 1: odd, so
//     the lanes of a wave, which read the same feature of different rows, hit different banks); every later pass
//     recomputes d^2 = sum_f (a_f - b_f)^2 from there.  The population of distances is never materialised.
//   * A thread owns the columns j = tid, tid + 256, ... of a region and walks the rows i of that column: row i is the
//     same address in every lane (an LDS broadcast), row j is conflict-free.
//   * Bandwidth: the rank (P - 1) / 2 is radix-selected on the bit pattern of d^2, four 8-bit digits, most significant
//     first.  A pass counts the digit of the elements that match the prefix found so far into a 256-bin LDS histogram
//     (integer atomics; a thread merges runs of equal digits first, because in the first passes nearly every element
//     has the same digit), then wave 0 scans the bins and fixes the digit.  One sqrt at the end.
//   * Sums: every thread adds its pairs in a fixed order in fp64; partial sums go through a fixed shuffle tree and a
//     fixed serial sum over the four waves.  No float atomics: out[s] does not depend on S or on the grid position.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_mmd.h"
#include "shuffle_prp.h"

#define MMD_THREADS 256

__host__ __device__ __forceinline__ unsigned long long mmd_key(unsigned long long seed, unsigned long long t) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (t + 1ull);       // splitmix64's output function
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the ONE place a distance is computed: every pass gets the same bits
__device__ __forceinline__ float mmd_dist2(const float* __restrict__ ri, const float* __restrict__ rj, int D) {
  float acc = 0.f;
  for (int f = 0; f < D; ++f) {
    const float d = ri[f] - rj[f];
    acc = fmaf(d, d, acc);
  }
  return acc;
}

// Calls fn(d^2) for this thread's pairs of the region rows [ib, ib + ni) x columns [jb, jb + nj); `tri`: only i < j
// (ib == jb, ni == nj: the strict lower triangle).
template <typename F>
__device__ __forceinline__ void mmd_region(const float* __restrict__ rows, int stride, int D, int ib, int ni, int jb,
                                           int nj, bool tri, int tid, F fn) {
  for (int j = tid; j < nj; j += MMD_THREADS) {
    const float* __restrict__ rj = rows + (size_t)(jb + j) * stride;
    const int iend = tri ? j : ni;
    for (int i = 0; i < iend; ++i) fn(mmd_dist2(rows + (size_t)(ib + i) * stride, rj, D));
  }
}

// the population of the median: fn(d^2) over this thread's share
template <typename F>
__device__ __forceinline__ void mmd_population(const float* __restrict__ rows, int stride, int D, int M, int n_a,
                                               int pair_set, int median_set, int tid, F fn) {
  mmd_region(rows, stride, D, 0, n_a, n_a, M - n_a, false, tid, fn);
  if (median_set) {
    mmd_region(rows, stride, D, 0, n_a, 0, n_a, pair_set != 0, tid, fn);
    mmd_region(rows, stride, D, n_a, M - n_a, n_a, M - n_a, pair_set != 0, tid, fn);
  }
}

__device__ __forceinline__ double mmd_block_sum(double v, double* __restrict__ red, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(MMD_THREADS)
mmd_rbf_splits_kernel(const float* __restrict__ pool, long long N, int D, const int* __restrict__ idx,
                      unsigned long long seed, unsigned long long split_offset, int M, int n_a, int pair_set,
                      int median_set, const float* __restrict__ bandwidth, float bw_floor, float* __restrict__ out,
                      int stride, int hb) {
  extern __shared__ float mmd_rows[];
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[2];                       // { prefix found so far, rank inside it }
  __shared__ int bad;
  __shared__ double red[MMD_THREADS / 64];
  const int tid = threadIdx.x;
  const long long s = blockIdx.x;
  float* __restrict__ o = out + s * 4;
  if (tid == 0) bad = 0;
  __syncthreads();
  // ---- gather the split's rows (independent loads: element e = (row j, feature f))
  {
    const unsigned long long key = mmd_key(seed, (unsigned long long)s + split_offset);
    const int* __restrict__ sidx = idx ? idx + s * M : nullptr;
    const int total = M * D;
    int flag = 0;
    for (int e = tid; e < total; e += MMD_THREADS) {
      const int j = e / D, f = e - j * D;
      const long long src = sidx ? (long long)sidx[j] : (long long)shf_prp((unsigned)j, (unsigned)N, hb, key);
      float v = 0.f;
      if (src < 0 || src >= N) flag = 1;
      else v = pool[src * D + f];
      if (!(fabsf(v) <= 3.402823466e38f)) flag = 1;   // NaN or infinity
      mmd_rows[(size_t)j * stride + f] = v;
    }
    if (flag) atomicOr(&bad, 1);
  }
  __syncthreads();
  if (bad) {                                         // (the same in every thread)
    if (tid < 4) o[tid] = __builtin_nanf("");
    return;
  }
  const int n_b = M - n_a;
  float bw;
  if (bandwidth) {
    bw = bandwidth[s];
  } else {
    // ---- the element of rank (P - 1) / 2 of the population, by its bit pattern
    const unsigned within_a = pair_set ? (unsigned)n_a * (unsigned)(n_a - 1) / 2u : (unsigned)n_a * (unsigned)n_a;
    const unsigned within_b = pair_set ? (unsigned)n_b * (unsigned)(n_b - 1) / 2u : (unsigned)n_b * (unsigned)n_b;
    const unsigned P = (unsigned)n_a * (unsigned)n_b + (median_set ? within_a + within_b : 0u);
    if (tid == 0) {
      sel[0] = 0u;
      sel[1] = (P - 1u) / 2u;
    }
    unsigned mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[tid] = 0u;                                // (MMD_THREADS == 256 bins)
      __syncthreads();
      const unsigned prefix = sel[0];
      int cur = -1;
      unsigned cnt = 0u;
      mmd_population(mmd_rows, stride, D, M, n_a, pair_set, median_set, tid, [&](float d2) {
        const unsigned bits = __float_as_uint(d2);
        if ((bits & mask) == prefix) {
          const int dg = (int)((bits >> shift) & 255u);
          if (dg == cur) {
            ++cnt;
          } else {
            if (cnt) atomicAdd(&hist[cur], cnt);
            cur = dg;
            cnt = 1u;
          }
        }
      });
      if (cnt) atomicAdd(&hist[cur], cnt);
      __syncthreads();
      if (tid < 64) {                                // wave 0: lane l owns bins 4 l .. 4 l + 3
        const unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
        const unsigned mine = h0 + h1 + h2 + h3;
        unsigned incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned v = __shfl_up(incl, off);
          if (tid >= off) incl += v;
        }
        const unsigned rank = sel[1];
        const unsigned long long hit = __ballot(incl > rank);    // never empty: the prefix holds more than `rank`
        const int owner = (int)__builtin_ctzll(hit);
        if (tid == owner) {
          unsigned r = rank - (incl - mine);
          int dg = 4 * tid;
          if (r >= h0) { r -= h0; ++dg;
            if (r >= h1) { r -= h1; ++dg;
              if (r >= h2) { r -= h2; ++dg; } } }
          sel[0] = prefix | ((unsigned)dg << shift);
          sel[1] = r;
        }
      }
      mask |= 255u << shift;
      __syncthreads();
    }
    bw = fmaxf(bw_floor, __fsqrt_rn(__uint_as_float(sel[0])));
  }
  // ---- the three sums at that bandwidth
  const float inv = 1.f / (2.f * bw * bw);
  double acc;
  auto add = [&](float d2) { acc += (double)expf(-d2 * inv); };
  acc = 0.0;
  mmd_region(mmd_rows, stride, D, 0, n_a, 0, n_a, pair_set != 0, tid, add);
  const double s_aa = mmd_block_sum(acc, red, tid);
  acc = 0.0;
  mmd_region(mmd_rows, stride, D, n_a, n_b, n_a, n_b, pair_set != 0, tid, add);
  const double s_bb = mmd_block_sum(acc, red, tid);
  acc = 0.0;
  mmd_region(mmd_rows, stride, D, 0, n_a, n_a, n_b, false, tid, add);
  const double s_ab = mmd_block_sum(acc, red, tid);
  if (tid == 0) {
    o[0] = bw;
    o[1] = (float)s_aa;
    o[2] = (float)s_bb;
    o[3] = (float)s_ab;
  }
}

extern "C" int sbi_amd_mmd_rbf_splits(const float* pool, int64_t N, int32_t D, const int32_t* idx, uint64_t seed,
                                      uint64_t split_offset, int64_t S, int32_t M, int32_t n_a, int32_t pair_set,
                                      int32_t median_set, const float* bandwidth, float bw_floor, float* out,
                                      void* stream) {
  if (!pool || !out || S < 0 || S > 0x7fffffffll || N < 1 || N > 0x7fffffffll || D < 1 || M < 2 || n_a < 1 ||
      n_a >= M || (pair_set != 0 && pair_set != 1) || (median_set != 0 && median_set != 1) || !(bw_floor >= 0.f) ||
      (!idx && (int64_t)M > N))
    return SBI_AMD_E_BADARG;
  const int64_t stride = (int64_t)D | 1;
  if ((int64_t)M * stride > SBI_AMD_MMD_STAGE_FLOATS) return SBI_AMD_E_UNSUPPORTED;
  if (S == 0) return 0;
  hipLaunchKernelGGL(mmd_rbf_splits_kernel, dim3((unsigned)S), dim3(MMD_THREADS),
                     (size_t)M * (size_t)stride * sizeof(float), (hipStream_t)stream, pool, (long long)N, (int)D, idx,
                     (unsigned long long)seed, (unsigned long long)split_offset, (int)M, (int)n_a, (int)pair_set,
                     (int)median_set, bandwidth, bw_floor, out, (int)stride, shf_half_bits((long long)N));
  return (int)hipGetLastError();
}
