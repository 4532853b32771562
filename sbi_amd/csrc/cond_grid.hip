// cond_grid.hip -- conditional-density grids (sbi/analysis/conditional_density.py `eval_conditional_density` /
// `conditional_corrcoeff`, sbi/utils/conditional_density_utils.py `compute_corrcoeff` / `ConditionedPotential`):
//   * sbi_amd_cond_grid_fill: the theta rows of a chunk of whole grids in one launch (a gather from the host's
//     `linspace` values: bit-equal to the eager repeat / repeat_interleave construction);
//   * sbi_amd_cond_grid_moments: per grid the maximum, w = exp(logp - m) in fp32, six fp64 moments on coordinates
//     centred at the axis midpoint and the correlation coefficient, one launch per chunk;
//   * sbi_amd_cond_expand: a conditioned potential's `repeat` plus scatter as one launch.
// Semantics, the degenerate-grid rule and the mapping: include/sbi_amd_cond.h.  A grid's arithmetic is fixed by R alone
// (lane-group width or the 256-thread stride, butterfly order, wave order): no atomics, 64-bit indexing of the chunk.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_cond.h"

#pragma clang fp contract(off)   // vx = Sxx/S - mx*mx must be exactly 0 for a one-cell grid, and match the host formula

#define COND_THREADS 256
#define COND_MAX_R 1024
#define COND_MAX_D 64
#define COND_EXPAND_MAX_D 1024

// ---------------------------------------------------------------------------------------------------------------- fill
__global__ void __launch_bounds__(COND_THREADS)
cond_fill_kernel(const float* __restrict__ cond, const float* __restrict__ axes, const int* __restrict__ pairs, int D,
                 int R, int P, int mode, long long g0, int E, long long total, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * COND_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long gl = e / E;                      // grid inside the chunk
  const int r = (int)(e - gl * E);                 // element inside the grid: cell * D + d
  const int cell = r / D, d = r - cell * D;
  const long long g = g0 + gl;
  const long long c = g / P;
  const int p = (int)(g - c * P);
  const int d1 = pairs[2 * p], d2 = pairs[2 * p + 1];
  const bool ok = (unsigned)d1 < (unsigned)D && (unsigned)d2 < (unsigned)D && (mode == 2 ? d1 != d2 : d1 == d2);
  float v;
  if (!ok) {
    v = __builtin_nanf("");
  } else if (mode == 2) {
    const int i = cell / R, j = cell - i * R;
    v = d == d1 ? axes[d1 * R + j] : (d == d2 ? axes[d2 * R + i] : cond[c * D + d]);
  } else {
    v = d == d1 ? axes[d1 * R + cell] : cond[c * D + d];
  }
  out[e] = v;
}

extern "C" int sbi_amd_cond_grid_fill(const float* cond, const float* axes, const int32_t* pairs, int32_t D, int32_t R,
                                      int32_t P, int32_t mode, int64_t g0, int64_t g1, float* out, void* stream) {
  if (!cond || !axes || !pairs || !out || D < 1 || R < 1 || P < 1 || (mode != 1 && mode != 2) || g0 < 0 || g1 < g0)
    return SBI_AMD_E_BADARG;
  if (R > COND_MAX_R || D > COND_MAX_D) return SBI_AMD_E_UNSUPPORTED;
  if (g1 == g0) return 0;
  const int64_t cells = mode == 2 ? (int64_t)R * R : R;
  const int64_t E = cells * D;                                    // <= 2^26
  const int64_t G = g1 - g0;
  const int64_t total = G * E;
  const int64_t blocks = (total + COND_THREADS - 1) / COND_THREADS;
  if (G > ((int64_t)1 << 62) / E || blocks > 0x7fffffffll) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(cond_fill_kernel, dim3((unsigned)blocks), dim3(COND_THREADS), 0, (hipStream_t)stream, cond, axes,
                     pairs, D, R, P, mode, (long long)g0, (int)E, (long long)total, out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------- moments
struct CondAxes {
  const float* ax;   // axes[d1] (x, varies with j)
  const float* ay;   // axes[d2] (y, varies with i)
  double cx, cy;     // the axis midpoints
  bool ok;
};

__device__ __forceinline__ CondAxes cond_axes(const float* __restrict__ axes, const int* __restrict__ pairs, int D, int R,
                                              int P, long long g) {
  CondAxes a;
  const int p = (int)(g % P);
  const int d1 = pairs[2 * p], d2 = pairs[2 * p + 1];
  a.ok = (unsigned)d1 < (unsigned)D && (unsigned)d2 < (unsigned)D && d1 != d2;
  a.ax = axes + (a.ok ? d1 : 0) * R;
  a.ay = axes + (a.ok ? d2 : 0) * R;
  a.cx = ((double)a.ax[0] + (double)a.ax[R - 1]) * 0.5;
  a.cy = ((double)a.ay[0] + (double)a.ay[R - 1]) * 0.5;
  return a;
}

// The weight of one cell added to the six running sums (s[0..5] = S, Sx, Sy, Sxx, Syy, Sxy).
__device__ __forceinline__ void cond_accumulate(double* s, float w, double xc, double yc) {
  const double wd = (double)w, wx = wd * xc, wy = wd * yc;
  s[0] += wd;
  s[1] += wx;
  s[2] += wy;
  s[3] += wx * xc;
  s[4] += wy * yc;
  s[5] += wx * yc;
}

// rho and the moments row of one grid, written by one thread.  `bad`: a NaN (or an invalid pair); m: the maximum.
__device__ __forceinline__ void cond_finish(const double* s, bool bad, float m, long long g, float* __restrict__ rho,
                                            double* __restrict__ moments) {
  const bool dead = bad || m == INFINITY || m == -INFINITY;
  float r = __builtin_nanf("");
  if (!dead) {
    const double S = s[0], mx = s[1] / S, my = s[2] / S;
    const double vx = s[3] / S - mx * mx, vy = s[4] / S - my * my;
    const double cov = s[5] / S - mx * my, vv = vx * vy;
    if (vv > 0.0) r = (float)(cov / sqrt(vv));
  }
  rho[g] = r;
  if (moments) {
#pragma unroll
    for (int q = 0; q < 6; ++q) moments[g * 6 + q] = dead ? (double)__builtin_nanf("") : s[q];
  }
}

// the weight of a cell once the grid's verdict is known: NaN / 0 for a degenerate grid, exp(lp - m) otherwise
__device__ __forceinline__ float cond_weight(float lp, float m, bool bad) {
  if (bad || m == INFINITY) return __builtin_nanf("");
  if (m == -INFINITY) return 0.f;
  return expf(lp - m);
}

template <int W>
__global__ void __launch_bounds__(COND_THREADS)
cond_moments_group_kernel(const float* __restrict__ logp, const float* __restrict__ axes, const int* __restrict__ pairs,
                          int D, int R, int P, long long g0, long long G, float* __restrict__ rho,
                          float* __restrict__ probs, double* __restrict__ moments) {
  constexpr int GPB = COND_THREADS / W;            // grids per workgroup
  const int tid = threadIdx.x, gl = tid & (W - 1), N = R * R;
  const long long g = (long long)blockIdx.x * GPB + tid / W;
  const bool valid = g < G;                        // (no early exit: every lane takes part in the butterflies)
  const bool has = valid && gl < N;
  const CondAxes a = cond_axes(axes, pairs, D, R, P, g0 + (valid ? g : 0));
  float lp = -INFINITY;
  if (has) lp = logp[g * N + gl];
  int bad = (has && lp != lp) || !a.ok;
  float m = (lp != lp) ? -INFINITY : lp;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    m = fmaxf(m, __shfl_xor(m, off, W));
    bad |= __shfl_xor(bad, off, W);
  }
  const float w = cond_weight(lp, m, bad != 0);
  if (has && probs) probs[g * N + gl] = w;
  double s[6] = {0., 0., 0., 0., 0., 0.};
  if (has && !bad && m != INFINITY && m != -INFINITY) {
    const int i = gl / R, j = gl - i * R;
    cond_accumulate(s, w, (double)a.ax[j] - a.cx, (double)a.ay[i] - a.cy);
  }
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] += __shfl_xor(s[q], off, W);
  }
  if (valid && gl == 0) cond_finish(s, bad != 0, m, g, rho, moments);
}

__global__ void __launch_bounds__(COND_THREADS)
cond_moments_block_kernel(const float* __restrict__ logp, const float* __restrict__ axes, const int* __restrict__ pairs,
                          int D, int R, int P, long long g0, float* __restrict__ rho, float* __restrict__ probs,
                          double* __restrict__ moments) {
  __shared__ float sh_m[COND_THREADS / 64];
  __shared__ int sh_bad[COND_THREADS / 64];
  __shared__ double sh_s[COND_THREADS / 64][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = R * R;
  const long long g = blockIdx.x;
  const CondAxes a = cond_axes(axes, pairs, D, R, P, g0 + g);
  const float* __restrict__ lpg = logp + g * N;
  // ---- pass 1: the maximum and the NaN flag
  float m = -INFINITY;
  int bad = !a.ok;
  for (int n = tid; n < N; n += COND_THREADS) {
    const float v = lpg[n];
    bad |= (v != v);
    m = fmaxf(m, v);                               // (a NaN operand is ignored: `bad` carries it)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    m = fmaxf(m, __shfl_xor(m, off));
    bad |= __shfl_xor(bad, off);
  }
  if (lane == 0) {
    sh_m[wave] = m;
    sh_bad[wave] = bad;
  }
  __syncthreads();
  m = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
  bad = sh_bad[0] | sh_bad[1] | sh_bad[2] | sh_bad[3];
  const bool live = !bad && m != INFINITY && m != -INFINITY;
  // ---- pass 2: the weights (from L2) and the six sums: per thread in cell order, lanes by butterfly, waves in order
  double s[6] = {0., 0., 0., 0., 0., 0.};
  float* __restrict__ pg = probs ? probs + g * N : nullptr;
  for (int n = tid; n < N; n += COND_THREADS) {
    const float w = cond_weight(lpg[n], m, bad != 0);
    if (pg) pg[n] = w;
    if (live) {
      const int i = n / R, j = n - i * R;
      cond_accumulate(s, w, (double)a.ax[j] - a.cx, (double)a.ay[i] - a.cy);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] += __shfl_xor(s[q], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) sh_s[wave][q] = s[q];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] = ((sh_s[0][q] + sh_s[1][q]) + sh_s[2][q]) + sh_s[3][q];
    cond_finish(s, bad != 0, m, g, rho, moments);
  }
}

extern "C" int sbi_amd_cond_grid_moments(const float* logp, const float* axes, const int32_t* pairs, int32_t D,
                                         int32_t R, int32_t P, int64_t g0, int64_t G, float* rho, float* probs,
                                         double* moments, void* stream) {
  if (!logp || !axes || !pairs || !rho || D < 1 || R < 1 || P < 1 || g0 < 0 || G < 0) return SBI_AMD_E_BADARG;
  if (R > COND_MAX_R || D > COND_MAX_D) return SBI_AMD_E_UNSUPPORTED;
  if (G == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int N = R * R;
  if (N <= 64) {
    int W = 1;
    while (W < N) W <<= 1;
    const int64_t blocks = (G + COND_THREADS / W - 1) / (COND_THREADS / W);
    if (blocks > 0x7fffffffll) return SBI_AMD_E_BADARG;
#define COND_LAUNCH(WW)                                                                                              \
  hipLaunchKernelGGL(cond_moments_group_kernel<WW>, dim3((unsigned)blocks), dim3(COND_THREADS), 0, s, logp, axes,   \
                     pairs, D, R, P, (long long)g0, (long long)G, rho, probs, moments)
    switch (W) {
      case 1: COND_LAUNCH(1); break;
      case 2: COND_LAUNCH(2); break;
      case 4: COND_LAUNCH(4); break;
      case 8: COND_LAUNCH(8); break;
      case 16: COND_LAUNCH(16); break;
      case 32: COND_LAUNCH(32); break;
      default: COND_LAUNCH(64); break;
    }
#undef COND_LAUNCH
    return (int)hipGetLastError();
  }
  if (G > 0x7fffffffll) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(cond_moments_block_kernel, dim3((unsigned)G), dim3(COND_THREADS), 0, s, logp, axes, pairs, D, R, P,
                     (long long)g0, rho, probs, moments);
  return (int)hipGetLastError();
}

// -------------------------------------------------------------------------------------------------------------- expand
__global__ void __launch_bounds__(COND_THREADS)
cond_expand_kernel(const float* __restrict__ cond, const int* __restrict__ dims, const float* __restrict__ theta,
                   long long total, int D, int k, float* __restrict__ out) {
  __shared__ int inv[COND_EXPAND_MAX_D];           // column of theta that lands in dimension d, or -1
  for (int d = threadIdx.x; d < D; d += COND_THREADS) inv[d] = -1;
  __syncthreads();
  for (int q = threadIdx.x; q < k; q += COND_THREADS) {
    const int d = dims[q];
    if ((unsigned)d < (unsigned)D) inv[d] = q;
  }
  __syncthreads();
  const long long e = (long long)blockIdx.x * COND_THREADS + threadIdx.x;
  if (e >= total) return;
  const long long n = e / D;
  const int d = (int)(e - n * D);
  const int q = inv[d];
  out[e] = q >= 0 ? theta[n * k + q] : cond[d];
}

extern "C" int sbi_amd_cond_expand(const float* cond, const int32_t* dims, const float* theta, int64_t N, int32_t D,
                                   int32_t k, float* out, void* stream) {
  if (!cond || !dims || !theta || !out || N < 0 || D < 1 || k < 1 || k > D) return SBI_AMD_E_BADARG;
  if (D > COND_EXPAND_MAX_D) return SBI_AMD_E_UNSUPPORTED;
  if (N == 0) return 0;
  const int64_t total = N * D;
  const int64_t blocks = (total + COND_THREADS - 1) / COND_THREADS;
  if (N > ((int64_t)1 << 62) / D || blocks > 0x7fffffffll) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(cond_expand_kernel, dim3((unsigned)blocks), dim3(COND_THREADS), 0, (hipStream_t)stream, cond, dims,
                     theta, (long long)total, D, k, out);
  return (int)hipGetLastError();
}
