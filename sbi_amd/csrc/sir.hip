// sir.hip -- the selection step of sampling-importance-resampling (sbi/samplers/importance/sir.py:49-71: per row of
// K candidates `softmax(log_p - log_q)`, `cumsum`, `rand`, first index whose cumulative weight reaches u, mask gather)
// as ONE launch without a host synchronisation.  Semantics, the dead-row rule and the two departures from the
// reference: include/sbi_amd_sir.h.
//   * K <= 64: rows packed into lane groups of width W = min(64, next_pow2(K)); max, scan and search through
//     cross-lane operations only (no LDS); the log-weights are read once.
//   * K > 64: one wave per row, 64-candidate chunks with a serial carry.  The row is staged in LDS while its maximum
//     is taken and is overwritten there by its prefix sums, so memory is read once; a row that does not fit one
//     workgroup's LDS (K > SIR_LDS_MAX_K = 40 960) has no kernel: SBI_AMD_E_UNSUPPORTED.
//   * A row's arithmetic is fixed by K alone (group width, chunking, scan order): the result does not depend on B, on
//     the row's position in the grid or on the lanes that process it.  No float atomics; 64-bit indexing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_sir.h"
#include "philox.h"

#define SIR_THREADS 256
#define SIR_STREAM_TAG 0x53495231u               // "SIR1": keeps this stream apart from the samplers' (philox.h)
#define SIR_LDS_MAX_K (160 * 1024 / 4)           // a row of this many candidates still fits one workgroup's LDS

__device__ __forceinline__ float sir_uniform(const float* __restrict__ u, long long r, unsigned long long seed,
                                             unsigned long long row_offset) {
  if (u) return u[r];
  const unsigned long long row = (unsigned long long)r + row_offset;
  unsigned o[4];
  philox4x32_10((unsigned)row, (unsigned)(row >> 32), 0u, SIR_STREAM_TAG, (unsigned)seed, (unsigned)(seed >> 32), o);
  return u01(o[0]);
}

// Inclusive Hillis-Steele scan inside an aligned group of W lanes (gl = lane inside the group): a fixed order.
template <int W>
__device__ __forceinline__ float sir_scan(float e, int gl) {
  float p = e;
#pragma unroll
  for (int off = 1; off < W; off <<= 1) {
    const float v = __shfl_up(p, off, W);
    if (gl >= off) p += v;
  }
  return p;
}

// idx, row_lse, the dead-row counter and the copy of the winner's D floats by the row's W lanes
template <int W>
__device__ __forceinline__ void sir_finish(const float* __restrict__ cand, long long r, int K, int D, int gl, int w,
                                           bool dead, bool bad, float m, float S, float* __restrict__ out,
                                           int* __restrict__ idx, float* __restrict__ row_lse,
                                           int* __restrict__ n_dead) {
  if (gl == 0) {
    idx[r] = w;
    if (row_lse) row_lse[r] = dead ? (bad ? __builtin_nanf("") : m) : m + logf(S);
    if (dead && n_dead) atomicAdd(n_dead, 1);
  }
  if (w >= 0) {
    const float* __restrict__ src = cand + (r * K + w) * D;
    float* __restrict__ dst = out + r * D;
    for (int d = gl; d < D; d += W) dst[d] = src[d];
  }
}

template <int W>
__global__ void __launch_bounds__(SIR_THREADS)
sir_group_kernel(const float* __restrict__ lp, const float* __restrict__ lq, const float* __restrict__ cand,
                 long long B, int K, int D, const float* __restrict__ u, unsigned long long seed,
                 unsigned long long row_offset, float* __restrict__ out, int* __restrict__ idx,
                 float* __restrict__ row_lse, int* __restrict__ n_dead) {
  constexpr int RPB = SIR_THREADS / W;             // rows per workgroup
  const int tid = threadIdx.x, lane = tid & 63, gl = tid & (W - 1);
  const long long r = (long long)blockIdx.x * RPB + tid / W;
  const bool valid = r < B;                        // (no early exit: every lane takes part in the ballots below)
  const bool has = valid && gl < K;
  float lw = -INFINITY;
  if (has) {
    const long long i = r * K + gl;
    lw = lp[i];
    if (lq) lw -= lq[i];
  }
  int bad = has && (lw != lw);
  float m = bad ? -INFINITY : lw;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    m = fmaxf(m, __shfl_xor(m, off, W));
    bad |= __shfl_xor(bad, off, W);
  }
  const bool dead = bad || m == INFINITY || m == -INFINITY;
  const float e = (has && !dead) ? expf(lw - m) : 0.f;
  const float P = sir_scan<W>(e, gl);
  const float S = __shfl(P, K - 1, W);
  const float t = (valid ? sir_uniform(u, r, seed, row_offset) : 0.f) * S;
  const bool pos = e > 0.f;
  const int gbase = lane & ~(W - 1);
  const unsigned long long gmask = W == 64 ? ~0ull : ((1ull << (W & 63)) - 1ull);
  const unsigned long long hb = (__ballot(pos && P > t) >> gbase) & gmask;
  const unsigned long long pb = (__ballot(pos) >> gbase) & gmask;
  const int w = hb ? (int)__builtin_ctzll(hb) : (pb ? 63 - (int)__builtin_clzll(pb) : -1);
  if (valid) sir_finish<W>(cand, r, K, D, gl, w, dead, bad != 0, m, S, out, idx, row_lse, n_dead);
}

// e_k and P_k of chunk c for this lane (k = 64 c + lane); `carry` = P of the last candidate of the chunk before
__device__ __forceinline__ void sir_chunk(float lw, bool in, float m, float carry, int lane, float& e, float& P) {
  e = in ? expf(lw - m) : 0.f;
  P = carry + sir_scan<64>(e, lane);
}

__global__ void __launch_bounds__(64)
sir_wave_kernel(const float* __restrict__ lp, const float* __restrict__ lq, const float* __restrict__ cand, int K, int D,
                const float* __restrict__ u, unsigned long long seed, unsigned long long row_offset,
                float* __restrict__ out, int* __restrict__ idx, float* __restrict__ row_lse, int* __restrict__ n_dead) {
  extern __shared__ float sir_row[];               // lw_k, then +-P_k (the sign says e_k == 0); lane-private slots
  const int lane = threadIdx.x;
  const long long r = blockIdx.x;
  const float* __restrict__ gp = lp + r * K;
  const float* __restrict__ gq = lq ? lq + r * K : nullptr;
  const int nch = (K + 63) >> 6;
  // ---- pass 1: maximum, NaN flag (and the row into LDS); four independent loads in flight per lane
  float m = -INFINITY;
  int bad = 0;
  for (int k0 = lane; k0 < K; k0 += 256) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 64 * j;
      v[j] = k < K ? gp[k] : -INFINITY;
    }
    if (gq) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + 64 * j;
        if (k < K) v[j] -= gq[k];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 64 * j;
      if (k < K) {
        sir_row[k] = v[j];
        bad |= (v[j] != v[j]);
        m = fmaxf(m, v[j]);                          // (a NaN operand is ignored: `bad` carries it)
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m = fmaxf(m, __shfl_xor(m, off));
    bad |= __shfl_xor(bad, off);
  }
  const bool dead = bad || m == INFINITY || m == -INFINITY;      // (the same in every lane)
  float S = 0.f;
  int w = -1;
  if (!dead) {
    // ---- pass 2: the prefix sums in chunk order; S = P_{K-1}
    float carry = 0.f;
    for (int c = 0; c < nch; ++c) {
      const int k = c * 64 + lane;
      const bool in = k < K;
      float lw = 0.f, e, P;
      if (in) lw = sir_row[k];
      sir_chunk(lw, in, m, carry, lane, e, P);
      if (in) sir_row[k] = e > 0.f ? P : -P;
      carry = __shfl(P, 63);
      if (c == nch - 1) S = __shfl(P, (K - 1) & 63);
    }
    // ---- pass 3: the smallest k with P_k > t and e_k > 0, else the largest k with e_k > 0
    const float t = sir_uniform(u, r, seed, row_offset) * S;
    int last_pos = -1;
    for (int c = 0; c < nch; ++c) {
      const int k = c * 64 + lane;
      const bool in = k < K;
      const float v = in ? sir_row[k] : -0.f;
      const bool pos = in && !signbit(v);
      const float P = fabsf(v);
      const unsigned long long hb = __ballot(pos && P > t), pb = __ballot(pos);
      if (pb) last_pos = c * 64 + 63 - (int)__builtin_clzll(pb);
      if (hb) {
        w = c * 64 + (int)__builtin_ctzll(hb);
        break;                                      // (wave-uniform: a ballot)
      }
    }
    if (w < 0) w = last_pos;
  }
  sir_finish<64>(cand, r, K, D, lane, w, dead, bad != 0, m, S, out, idx, row_lse, n_dead);
}

extern "C" int sbi_amd_sir_resample(const float* log_p, const float* log_q, const float* cand, int64_t B, int32_t K,
                                    int32_t D, const float* u, uint64_t seed, uint64_t row_offset, float* out,
                                    int32_t* idx, float* row_lse, int32_t* n_dead, void* stream) {
  if (!log_p || !cand || !out || !idx || B < 0 || K < 1 || D < 1) return SBI_AMD_E_BADARG;
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned long long sd = seed, ro = row_offset;
  if (K <= 64) {
    int W = 1;
    while (W < K) W <<= 1;
    const int64_t blocks = (B + SIR_THREADS / W - 1) / (SIR_THREADS / W);
    if (blocks > 0x7fffffffll) return SBI_AMD_E_BADARG;
#define SIR_LAUNCH(WW)                                                                                              \
  hipLaunchKernelGGL(sir_group_kernel<WW>, dim3((unsigned)blocks), dim3(SIR_THREADS), 0, s, log_p, log_q, cand,    \
                     (long long)B, K, D, u, sd, ro, out, idx, row_lse, n_dead)
    switch (W) {
      case 1: SIR_LAUNCH(1); break;
      case 2: SIR_LAUNCH(2); break;
      case 4: SIR_LAUNCH(4); break;
      case 8: SIR_LAUNCH(8); break;
      case 16: SIR_LAUNCH(16); break;
      case 32: SIR_LAUNCH(32); break;
      default: SIR_LAUNCH(64); break;
    }
#undef SIR_LAUNCH
    return (int)hipGetLastError();
  }
  if (K > SIR_LDS_MAX_K) return SBI_AMD_E_UNSUPPORTED;          // (the row no longer fits one workgroup's LDS)
  if (B > 0x7fffffffll) return SBI_AMD_E_BADARG;
  // (more than 64 KiB of dynamic LDS has to be asked for, on the device that is current, as the other launchers do)
  if (hipFuncSetAttribute((const void*)sir_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          SIR_LDS_MAX_K * 4) != hipSuccess)
    return SBI_AMD_E_UNSUPPORTED;
  hipLaunchKernelGGL(sir_wave_kernel, dim3((unsigned)B), dim3(64), (size_t)K * sizeof(float), s, log_p, log_q, cand, K,
                     D, u, sd, ro, out, idx, row_lse, n_dead);
  return (int)hipGetLastError();
}
