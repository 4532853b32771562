// sinkhorn.hip -- persistent batched Sinkhorn (log-domain dual updates of entropic optimal transport), one workgroup per
// problem: the cost matrix and both potentials stay in LDS for all iterations, convergence is decided on the device and
// nothing is read back.  Replaces the loop of sbi/utils/metrics.py regularized_ot_dual (about 15 launches and two host
// synchronisations per iteration, up to 1000 iterations).  Semantics, envelope and the LDS budget: include/sbi_amd_abc.h.
//   * C in LDS with the odd row stride n | 1: 32 consecutive rows of one column and 32 consecutive columns of one row
//     both fall on 32 different banks.
//   * A line (row in the f pass, column in the g pass) is reduced by G lanes, G = the largest power of two with
//     G max(m, n) <= 256; the lanes of a line sit 64 / G apart in one wave, so a half-wave covers neighbouring lines
//     at one element offset.  Maximum, then sum of exponentials, each through a fixed xor butterfly.
//   * err = max(sum |df|, sum |dg|): wave 0 sums |df|, wave 1 sums |dg|, each lane in index order, then a butterfly.
//   * Everything is a function of the problem's own data, m, n and D: not of B or the block index.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_abc.h"

#define SK_THREADS 256

__device__ __forceinline__ float sk_wave_sum(float v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
  return v;
}

// One dual update of every line.  ROW: line = row i, own = f, other = g, element (i, e).  !ROW: line = column j,
// own = g, other = f, element (e, j).  value(e) = ((f - C) + g) * inv_eps with f, g the row's and the column's potential.
template <bool ROW>
__device__ __forceinline__ void sk_pass(const float* __restrict__ C, int stride, int nl, int ne, float* __restrict__ own,
                                        const float* __restrict__ other, const float* __restrict__ logm,
                                        float* __restrict__ delta, float eps, float inv_eps, int G, int lane, int wave) {
  const int Lw = 64 / G, il = lane & (Lw - 1), k = lane / Lw;
  for (int base = 0; base < nl; base += 4 * Lw) {
    const int line = base + wave * Lw + il;
    const bool act = line < nl;
    const float p = act ? own[line] : 0.f;
    const float* __restrict__ cl = C + (ROW ? line * stride : line);
    const int step = ROW ? 1 : stride;
    float mx = -INFINITY;
    if (act)
      for (int e = k; e < ne; e += G) {
        const float cij = cl[e * step];
        const float v = ROW ? ((p - cij) + other[e]) * inv_eps : ((other[e] - cij) + p) * inv_eps;
        mx = fmaxf(mx, v);
      }
    for (int off = Lw; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float shift = mx == -INFINITY ? 0.f : mx;
    float s = 0.f;
    if (act)
      for (int e = k; e < ne; e += G) {
        const float cij = cl[e * step];
        const float v = ROW ? ((p - cij) + other[e]) * inv_eps : ((other[e] - cij) + p) * inv_eps;
        s += expf(v - shift);
      }
    for (int off = Lw; off < 64; off <<= 1) s += __shfl_xor(s, off);
    if (act && k == 0) {
      const float lse = shift + logf(s);
      const float np = p + eps * (logm[line] - lse);
      delta[line] = fabsf(p - np);
      own[line] = np;
    }
  }
}

__global__ void __launch_bounds__(SK_THREADS)
sinkhorn_kernel(const float* __restrict__ x, long long x_batch_stride, int m, const float* __restrict__ y, int n, int D,
                const float* __restrict__ cost, const float* __restrict__ a, const float* __restrict__ b, float eps,
                int max_iter, float tol, float* __restrict__ f_out, float* __restrict__ g_out, float* __restrict__ w_out,
                int* __restrict__ iters_out) {
  extern __shared__ double sk_dyn[];
  const int stride = n | 1;
  double* s_wrow = sk_dyn;                                   // m doubles
  float* s_C = reinterpret_cast<float*>(sk_dyn + m);          // m * stride
  float* s_f = s_C + m * stride;                              // m
  float* s_g = s_f + m;                                       // n
  float* s_la = s_g + n;                                      // m
  float* s_lb = s_la + m;                                     // n
  float* s_df = s_lb + n;                                     // m
  float* s_dg = s_df + m;                                     // n
  float* s_red = s_dg + n;                                    // 2 (of 16)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p = blockIdx.x;
  const float inv_eps = 1.f / eps;
  int G = 1;
  {
    const int big = m > n ? m : n;
    while (G < 64 && 2 * G * big <= SK_THREADS) G <<= 1;
  }

  // ---- the problem's cost matrix and log-marginals
  if (cost) {
    const float* __restrict__ cp = cost + p * m * n;
    for (int e = tid; e < m * n; e += SK_THREADS) s_C[(e / n) * stride + e % n] = cp[e];
  } else {
    const float* __restrict__ xp = x + p * x_batch_stride;
    const float* __restrict__ yp = y + p * n * D;
    for (int e = tid; e < m * n; e += SK_THREADS) {
      const int i = e / n, j = e % n;
      float d2 = 0.f;
      for (int d = 0; d < D; ++d) {
        const float df = xp[i * D + d] - yp[j * D + d];
        d2 = fmaf(df, df, d2);
      }
      s_C[i * stride + j] = d2;
    }
  }
  for (int i = tid; i < m; i += SK_THREADS) {
    s_f[i] = 0.f;
    s_la[i] = a ? logf(a[p * m + i]) : -logf((float)m);
  }
  for (int j = tid; j < n; j += SK_THREADS) {
    s_g[j] = 0.f;
    s_lb[j] = b ? logf(b[p * n + j]) : -logf((float)n);
  }
  __syncthreads();

  int it = 0;
  while (it < max_iter) {
    sk_pass<true>(s_C, stride, m, n, s_f, s_g, s_la, s_df, eps, inv_eps, G, lane, wave);
    __syncthreads();
    sk_pass<false>(s_C, stride, n, m, s_g, s_f, s_lb, s_dg, eps, inv_eps, G, lane, wave);
    __syncthreads();
    if (wave < 2) {
      const float* __restrict__ dl = wave == 0 ? s_df : s_dg;
      const int cnt = wave == 0 ? m : n;
      float acc = 0.f;
      for (int i = lane; i < cnt; i += 64) acc += dl[i];
      acc = sk_wave_sum(acc);
      if (lane == 0) s_red[wave] = acc;
    }
    __syncthreads();
    const float err = fmaxf(s_red[0], s_red[1]);
    ++it;
    if (err < tol) break;                                     // (block-uniform: every thread reads the same two floats)
  }

  // ---- w = sum_ij exp(((f_i - C_ij) + g_j) / eps) C_ij, rows by lane groups as in the f pass, in fp64
  if (w_out) {
    const int Lw = 64 / G, il = lane & (Lw - 1), k = lane / Lw;
    for (int base = 0; base < m; base += 4 * Lw) {
      const int i = base + wave * Lw + il;
      const bool act = i < m;
      double acc = 0.0;
      if (act) {
        const float fi = s_f[i];
        for (int j = k; j < n; j += G) {
          const float cij = s_C[i * stride + j];
          acc += (double)expf(((fi - cij) + s_g[j]) * inv_eps) * (double)cij;
        }
      }
      for (int off = Lw; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
      if (act && k == 0) s_wrow[i] = acc;
    }
    __syncthreads();
    if (wave == 0) {
      double acc = 0.0;
      for (int i = lane; i < m; i += 64) acc += s_wrow[i];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
      if (lane == 0) w_out[p] = (float)acc;
    }
  }
  if (f_out)
    for (int i = tid; i < m; i += SK_THREADS) f_out[p * m + i] = s_f[i];
  if (g_out)
    for (int j = tid; j < n; j += SK_THREADS) g_out[p * n + j] = s_g[j];
  if (iters_out && tid == 0) iters_out[p] = it;
}

extern "C" int sbi_amd_sinkhorn(const float* x, int64_t x_batch_stride, int32_t m, const float* y, int32_t n, int32_t D,
                                const float* cost, const float* a, const float* b, int64_t B, float eps,
                                int32_t max_iter, float tol, float* f, float* g, float* w, int32_t* iters,
                                void* stream) {
  if (m < 1 || n < 1 || B < 0 || B > 0x7fffffffll || x_batch_stride < 0 || !(eps > 0.f) || max_iter < 0 ||
      !(tol >= 0.f))
    return SBI_AMD_E_BADARG;
  if (!cost && (!x || !y || D < 1)) return SBI_AMD_E_BADARG;
  const long long floats = (long long)m * (n | 1) + 5ll * ((long long)m + n) + 16;
  if (floats > SBI_AMD_SINKHORN_LDS_FLOATS) return SBI_AMD_E_UNSUPPORTED;
  if (B == 0) return 0;
  // (more than 64 KiB of dynamic LDS has to be asked for, on the device that is current, as the other launchers do)
  if (hipFuncSetAttribute((const void*)sinkhorn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          SBI_AMD_SINKHORN_LDS_FLOATS * 4) != hipSuccess)
    return SBI_AMD_E_UNSUPPORTED;
  // the fp64 row sums come first, then m * (n | 1) + 3 (m + n) + 16 floats
  const size_t bytes = (size_t)m * 8 + ((size_t)m * (n | 1) + 3 * ((size_t)m + n) + 16) * 4;
  hipLaunchKernelGGL(sinkhorn_kernel, dim3((unsigned)B), dim3(SK_THREADS), bytes, (hipStream_t)stream, x,
                     (long long)x_batch_stride, m, y, n, D, cost, a, b, eps, max_iter, tol, f, g, w, iters);
  return (int)hipGetLastError();
}
