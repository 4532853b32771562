// mog.hip -- mixture-of-Gaussians algebra of NPE-A on gfx950 (C ABI: include/sbi_amd_mog.h): the analytic proposal
// correction in fp64, log_prob of an arbitrary mixture (MFMA for one mixture against many theta, a VALU wave per row
// for one mixture per row) and sampling by a binary search of an fp64 cumulative table.  DESIGN.md section 7o.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_mog.h"

namespace {

typedef float mog_f4 __attribute__((ext_vector_type(4)));
#define MOG_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

constexpr int MOG_DMAX = 16;
constexpr int MOG_MMAX = 65536;
constexpr int MOG_TAB = 18;               // doubles per component table entry: P m (16) | m^T P m | logdet P
constexpr int MOG_STATUS_NONE = 0x7f7f7f7f;
constexpr int MOG_PAIRS = 16;             // pairs (16 lanes each) per 256-thread workgroup
constexpr int MOG_TLD = 17;               // row stride (doubles) of the LDS transpose tile

__device__ __forceinline__ double bc16(double v, int src) { return __shfl(v, src, 16); }
__device__ __forceinline__ double sum16(double v) {
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}
// a[r] of the lane's own column index c (r == c), without a dynamic register index
__device__ __forceinline__ double own16(const double (&a)[MOG_DMAX], int c) {
  double v = 0.0;
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r) v = (r == c) ? a[r] : v;
  return v;
}

// In-place upper Cholesky factor of a symmetric D x D matrix held one column per lane (lane c of a 16-lane group:
// a[r] = S[r][c]); afterwards a[r] = U[r][c] for r <= c (entries below the diagonal are scratch).  Right-looking: row
// k is scaled by the broadcast pivot, then every lane takes U[k][r] from lane r for the trailing update.  Returns
// true when a pivot is not positive (the factorisation then carries on with pivot 1: no NaN is produced by it).
__device__ __forceinline__ bool chol16(double (&a)[MOG_DMAX], int D, int c) {
  bool fail = false;
#pragma unroll
  for (int k = 0; k < MOG_DMAX; ++k) {
    if (k < D) {
      double piv = bc16(a[k], k);
      if (!(piv > 0.0) || !(piv < 1.0e300)) {
        fail = true;
        piv = 1.0;
      }
      const double dk = sqrt(piv);
      const double ukc = (c == k) ? dk : a[k] / dk;
      a[k] = ukc;
#pragma unroll
      for (int r = k + 1; r < MOG_DMAX; ++r) {
        if (r < D) {
          const double ukr = bc16(a[k], r);
          if (r <= c) a[r] -= ukr * ukc;
        }
      }
    }
  }
  return fail;
}

// ---- pass 1 of the correction: per component P m, m^T P m, logdet P (fp64) -------------------------------------------
__global__ void __launch_bounds__(256)
mog_table_kernel(const float* __restrict__ d_means, const float* __restrict__ d_prec, long long n_d,
                 const float* __restrict__ p_means, const float* __restrict__ p_prec, long long n_p, int D,
                 double* __restrict__ tab) {
  const int c = threadIdx.x & 15;
  const long long total = n_d + n_p;
  long long q = (long long)blockIdx.x * MOG_PAIRS + (threadIdx.x >> 4);
  const bool live = q < total;
  if (!live) q = total - 1;                     // (clamped: the cross-lane operations below stay uniform)
  const bool dens = q < n_d;
  const float* P = dens ? d_prec + q * D * D : p_prec + (q - n_d) * D * D;
  const float* m = dens ? d_means + q * D : p_means + (q - n_d) * D;
  double a[MOG_DMAX];
  double pm = 0.0;
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r) {
    a[r] = (r < D && c < D) ? (double)P[r * D + c] : 0.0;
    if (r < D) pm += a[r] * (double)m[r];
  }
  const double mc = c < D ? (double)m[c] : 0.0;
  const double mpm = sum16(mc * pm);
  const bool fail = chol16(a, D, c);
  const double dg = own16(a, c);
  double ld = 2.0 * sum16(c < D ? log(dg) : 0.0);
  if (fail) ld = __longlong_as_double(0x7ff8000000000000LL);        // NaN marks a precision that is not positive definite
  if (live) {
    double* t = tab + q * MOG_TAB;
    t[c] = pm;
    if (c == 0) {
      t[16] = mpm;
      t[17] = ld;
    }
  }
}

// ---- pass 2: one corrected component per 16-lane group ----------------------------------------------------------------
struct MogCorrectArgs {
  const float *d_logits, *d_prec, *p_logits, *p_prec, *prior_mean, *prior_prec;
  const double* tab;
  long long B, prop_rows;
  int K, L, D, M;
  double eps;
  float *logits_out, *means_out, *prec_out, *factor_out;
  int* status;
};

__global__ void __launch_bounds__(256) mog_pair_kernel(const MogCorrectArgs A) {
  __shared__ double tile[MOG_PAIRS][MOG_DMAX * MOG_TLD];
  const int c = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const int D = A.D, K = A.K, M = A.M;
  const long long total = A.B * (long long)M;
  long long g = (long long)blockIdx.x * MOG_PAIRS + slot;
  const bool live = g < total;
  if (!live) g = total - 1;
  const long long b = g / M;
  const int j = (int)(g - b * M), l = j / K, k = j - l * K;
  const long long pb = A.prop_rows == 1 ? 0 : b;
  const long long dq = b * K + k, pq = pb * A.L + l;
  const float* Pd = A.d_prec + dq * D * D;
  const float* Pp = A.p_prec + pq * D * D;
  const double* td = A.tab + dq * MOG_TAB;
  const double* tp = A.tab + (A.B * (long long)K + pq) * MOG_TAB;
  const bool has_prior = A.prior_prec != nullptr;
  const bool act = c < D;

  double s[MOG_DMAX], a[MOG_DMAX];
  double rhs = act ? td[c] - tp[c] : 0.0;
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r) {
    double v = 0.0;
    if (r < D && act) {
      v = (double)Pd[r * D + c] - (double)Pp[r * D + c];
      if (has_prior) {
        const double p0 = (double)A.prior_prec[r * D + c];
        v += p0;
        rhs += p0 * (double)A.prior_mean[r];
      }
    }
    s[r] = v;
    a[r] = v + ((r == c && act) ? A.eps : 0.0);
  }
  float* prec_o = A.prec_out + g * D * D;
  float* fac_o = A.factor_out + g * D * D;
  if (live && act) {
#pragma unroll
    for (int r = 0; r < MOG_DMAX; ++r)
      if (r < D) prec_o[r * D + c] = (float)a[r];
  }
  bool fail = chol16(a, D, c);
  const double dg = act ? own16(a, c) : 1.0;

  // U^T y = rhs: lane r finalises y[r], the lanes to its right subtract U[r][c] y[r]
  double acc = rhs, y = 0.0;
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r) {
    if (r < D) {
      const double yr = bc16(acc / dg, r);
      if (c == r) y = yr;
      if (c > r) acc -= a[r] * yr;
    }
  }
  // rows of U for the back-substitution: transpose through LDS
  double* T = tile[slot];
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r) T[r * MOG_TLD + c] = (r <= c && act && r < D) ? a[r] : 0.0;
  __syncthreads();
  double row[MOG_DMAX], mm[MOG_DMAX];
#pragma unroll
  for (int cc = 0; cc < MOG_DMAX; ++cc) row[cc] = T[c * MOG_TLD + cc];
  // U m = y: lane cc finalises m[cc], the lanes above it subtract U[r][cc] m[cc]; every lane keeps the whole m
  acc = y;
#pragma unroll
  for (int cc = MOG_DMAX - 1; cc >= 0; --cc) {
    mm[cc] = 0.0;
    if (cc < D) {
      const double mc = bc16(acc / dg, cc);
      mm[cc] = mc;
      if (c < cc) acc -= row[cc] * mc;
    }
  }
  // m^T S m on the unstabilised S: lane c holds column c = row c of the symmetric S
  double sm = 0.0;
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r) sm += s[r] * mm[r];
  const double m_own = own16(mm, c);
  const double q_post = sum16(act ? m_own * sm : 0.0);
  const double ld_post = 2.0 * sum16(act ? log(dg) : 0.0);
  const double ld_d = td[17], ld_p = tp[17];
  fail = fail || ld_d != ld_d || ld_p != ld_p;
  const double logit = (double)A.d_logits[dq] - (double)A.p_logits[pq] + 0.5 * (-ld_post - ld_p + ld_d) -
                       0.5 * (td[16] - tp[16] - q_post);
  fail = fail || !(fabs(logit) < 1.0e300);
  if (live) {
    if (act) {
      A.means_out[g * D + c] = fail ? 0.f : (float)m_own;
#pragma unroll
      for (int r = 0; r < MOG_DMAX; ++r)
        if (r < D) fac_o[r * D + c] = (fail || r > c) ? 0.f : (float)a[r];
    }
    if (c == 0) {
      A.logits_out[g] = fail ? 0.f : (float)logit;
      if (fail) atomicMin(A.status + b, 1 + j);
    }
  }
}

__global__ void mog_status_kernel(int* __restrict__ status, long long B) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B && status[i] >= MOG_STATUS_NONE) status[i] = 0;
}

// ---- log_prob, one mixture for every theta row (MFMA) ------------------------------------------------------------------
constexpr int LP_G = 32;                  // components staged per group
constexpr int LP_LD = 20;                 // row stride of a staged P tile (conflict-free A-operand reads)
constexpr int LP_CF = 16 * LP_LD + 16 + 4;   // floats per staged component: P tile | mean | constant, padded
constexpr int LP_T = 4;                   // 16-row tiles per wave
constexpr int LP_ROWS = 4 * LP_T * 16;    // rows per workgroup (4 waves)

__device__ __forceinline__ double block_reduce_256(double v, double* red, bool take_max) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] = take_max ? fmax(red[t], red[t + w]) : red[t] + red[t + w];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(256)
mog_logp_bcast_kernel(const float* __restrict__ logits, const float* __restrict__ means,
                      const float* __restrict__ prec, const float* __restrict__ factors, int M, int D,
                      const float* __restrict__ theta, long long n, const float* __restrict__ shift,
                      const float* __restrict__ scale, float* __restrict__ out) {
  __shared__ float grp[LP_G * LP_CF];
  __shared__ double red[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  // log-sum-exp of the logits: every workgroup takes it in the same fixed order
  double mx = -INFINITY;
  for (int j = tid; j < M; j += 256) mx = fmax(mx, (double)logits[j]);
  mx = block_reduce_256(mx, red, true);
  double se = 0.0;
  for (int j = tid; j < M; j += 256) se += exp((double)logits[j] - mx);
  se = block_reduce_256(se, red, false);
  const float lse = (float)(mx + log(se));
  const float log_z = (float)(0.5 * D * log(2.0 * M_PI));

  // this wave's theta rows in the two fragment layouts: B operand (feature 4 s + g) and D layout (feature 4 g + r)
  float zB[LP_T][4], zD[LP_T][4], run_m[LP_T], run_s[LP_T];
  float sum_log_scale = 0.f;
  for (int e = 0; e < D; ++e) sum_log_scale += scale ? logf(scale[e]) : 0.f;
#pragma unroll
  for (int t = 0; t < LP_T; ++t) {
    const long long row = (long long)blockIdx.x * LP_ROWS + (wave * LP_T + t) * 16 + i16;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int eb = 4 * s + g, ed = 4 * g + s;
      float vb = 0.f, vd = 0.f;
      if (row < n) {
        if (eb < D) vb = shift ? (theta[row * D + eb] - shift[eb]) / scale[eb] : theta[row * D + eb];
        if (ed < D) vd = shift ? (theta[row * D + ed] - shift[ed]) / scale[ed] : theta[row * D + ed];
      }
      zB[t][s] = vb;
      zD[t][s] = vd;
    }
    run_m[t] = -INFINITY;
    run_s[t] = 0.f;
  }

  for (int g0 = 0; g0 < M; g0 += LP_G) {
    const int cnt = min(LP_G, M - g0);
    __syncthreads();
    for (int e = tid; e < cnt * LP_CF; e += 256) {
      const int jj = e / LP_CF, rem = e - jj * LP_CF;
      const long long j = g0 + jj;
      float v = 0.f;
      if (rem < 16 * LP_LD) {
        const int r = rem / LP_LD, cc = rem - r * LP_LD;
        if (r < D && cc < D) v = prec[(j * D + r) * D + cc];
      } else if (rem < 16 * LP_LD + 16) {
        const int cc = rem - 16 * LP_LD;
        if (cc < D) v = means[j * D + cc];
      } else if (rem == 16 * LP_LD + 16) {
        float sld = 0.f;
        for (int cc = 0; cc < D; ++cc) sld += logf(factors[(j * D + cc) * D + cc]);
        v = logits[j] - lse - log_z + sld;
      }
      grp[e] = v;
    }
    __syncthreads();
    for (int jj = 0; jj < cnt; ++jj) {
      const float* C = grp + jj * LP_CF;
      float pa[4], mB[4], mD[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        pa[s] = C[i16 * LP_LD + 4 * s + g];                 // A[c = i16][e = 4 s + g] = P[c][e]
        mB[s] = C[16 * LP_LD + 4 * s + g];
        mD[s] = C[16 * LP_LD + 4 * g + s];
      }
      const float cst = C[16 * LP_LD + 16];
#pragma unroll
      for (int t = 0; t < LP_T; ++t) {
        mog_f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = MOG_MFMA(pa[s], zB[t][s] - mB[s], acc);   // (P d^T)[c = 4 g + r][row i16]
        float q = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) q += acc[r] * (zD[t][r] - mD[r]);
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        const float term = cst - 0.5f * q;
        if (term > run_m[t]) {
          run_s[t] = run_s[t] * expf(run_m[t] - term) + 1.f;
          run_m[t] = term;
        } else if (term > -INFINITY) {
          run_s[t] += expf(term - run_m[t]);
        }
      }
    }
  }
  if (g == 0) {
#pragma unroll
    for (int t = 0; t < LP_T; ++t) {
      const long long row = (long long)blockIdx.x * LP_ROWS + (wave * LP_T + t) * 16 + i16;
      if (row < n) out[row] = run_m[t] + logf(run_s[t]) - sum_log_scale;
    }
  }
}

// ---- log_prob, one mixture per row: a wave per row, lanes over the components -------------------------------------------
__global__ void __launch_bounds__(256)
mog_logp_rows_kernel(const float* __restrict__ logits, const float* __restrict__ means,
                     const float* __restrict__ prec, const float* __restrict__ factors, long long mog_rows, int M,
                     int D, const float* __restrict__ theta, long long n, const float* __restrict__ shift,
                     const float* __restrict__ scale, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                       // (whole waves leave: the cross-lane operations below stay uniform)
  const long long b = row % mog_rows;
  const float* lg = logits + b * M;
  float z[MOG_DMAX];
  float sum_log_scale = 0.f;
#pragma unroll
  for (int e = 0; e < MOG_DMAX; ++e) {
    z[e] = 0.f;
    if (e < D) {
      z[e] = shift ? (theta[row * D + e] - shift[e]) / scale[e] : theta[row * D + e];
      sum_log_scale += scale ? logf(scale[e]) : 0.f;
    }
  }
  float mx = -INFINITY;
  for (int j = lane; j < M; j += 64) mx = fmaxf(mx, lg[j]);
  for (int w = 32; w > 0; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
  float se = 0.f;
  for (int j = lane; j < M; j += 64) se += expf(lg[j] - mx);
  for (int w = 32; w > 0; w >>= 1) se += __shfl_xor(se, w);
  const float lse = mx + logf(se);
  const float log_z = (float)(0.5 * D * log(2.0 * M_PI));
  float run_m = -INFINITY, run_s = 0.f;
  for (int j = lane; j < M; j += 64) {
    const long long cj = b * M + j;
    const float* P = prec + cj * D * D;
    const float* U = factors + cj * D * D;
    const float* mu = means + cj * D;
    float d[MOG_DMAX];
#pragma unroll
    for (int e = 0; e < MOG_DMAX; ++e) d[e] = e < D ? z[e] - mu[e] : 0.f;
    float q = 0.f, sld = 0.f;
#pragma unroll
    for (int r = 0; r < MOG_DMAX; ++r) {
      if (r < D) {
        float pr = 0.f;
#pragma unroll
        for (int cc = 0; cc < MOG_DMAX; ++cc)
          if (cc < D) pr += P[r * D + cc] * d[cc];
        q += d[r] * pr;
        sld += logf(U[r * D + r]);
      }
    }
    const float term = lg[j] - lse - log_z + sld - 0.5f * q;
    if (term > run_m) {
      run_s = run_s * expf(run_m - term) + 1.f;
      run_m = term;
    } else if (term > -INFINITY) {
      run_s += expf(term - run_m);
    }
  }
  float all_m = run_m;
  for (int w = 32; w > 0; w >>= 1) all_m = fmaxf(all_m, __shfl_xor(all_m, w));
  float tot = run_m > -INFINITY ? run_s * expf(run_m - all_m) : 0.f;
  for (int w = 32; w > 0; w >>= 1) tot += __shfl_xor(tot, w);
  if (lane == 0) out[row] = all_m + logf(tot) - sum_log_scale;
}

// ---- sampling ----------------------------------------------------------------------------------------------------------
// cdf[b][j] = (sum of the first j + 1 weights) / (sum of all), fp64, in component order: thread t of the row's
// workgroup owns the t-th contiguous chunk, sums it serially, the chunk offsets are a serial prefix over the 256 chunks
__global__ void __launch_bounds__(256)
mog_cdf_kernel(const float* __restrict__ logits, int M, double* __restrict__ cdf) {
  __shared__ double red[256];
  __shared__ double offs[257];
  const int tid = threadIdx.x;
  const float* lg = logits + (long long)blockIdx.x * M;
  double* out = cdf + (long long)blockIdx.x * M;
  double mx = -INFINITY;
  for (int j = tid; j < M; j += 256) mx = fmax(mx, (double)lg[j]);
  mx = block_reduce_256(mx, red, true);
  const int chunk = (M + 255) / 256;
  const int lo = min(tid * chunk, M), hi = min(lo + chunk, M);
  double local = 0.0;
  for (int j = lo; j < hi; ++j) local += exp((double)lg[j] - mx);
  __syncthreads();
  red[tid] = local;
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int t = 0; t < 256; ++t) {
      offs[t] = run;
      run += red[t];
    }
    offs[256] = run;
  }
  __syncthreads();
  const double total = offs[256], base = offs[tid];
  local = 0.0;
  for (int j = lo; j < hi; ++j) {
    local += exp((double)lg[j] - mx);
    out[j] = (base + local) / total;
  }
}

__global__ void __launch_bounds__(256)
mog_sample_kernel(const float* __restrict__ means, const float* __restrict__ factors, long long mog_rows, int M, int D,
                  const float* __restrict__ u, const int* __restrict__ comp, const float* __restrict__ zeta,
                  long long n, const float* __restrict__ shift, const float* __restrict__ scale,
                  float* __restrict__ theta_out, const double* __restrict__ cdf) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long b = i % mog_rows;
  int k;
  if (comp) {
    k = min(max(comp[i], 0), M - 1);
  } else {
    // number of table entries <= u[i]
    const double* T = cdf + b * M;
    const double ui = (double)u[i];
    int lo = 0, hi = M;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (T[mid] <= ui) lo = mid + 1; else hi = mid;
    }
    k = min(lo, M - 1);
  }
  const long long cj = b * M + k;
  const float* U = factors + cj * D * D;
  const float* mu = means + cj * D;
  float x[MOG_DMAX];
#pragma unroll
  for (int r = MOG_DMAX - 1; r >= 0; --r) {
    x[r] = 0.f;
    if (r < D) {
      float acc = zeta[i * D + r];
#pragma unroll
      for (int cc = r + 1; cc < MOG_DMAX; ++cc)
        if (cc < D) acc -= U[r * D + cc] * x[cc];
      x[r] = acc / U[r * D + r];
    }
  }
#pragma unroll
  for (int r = 0; r < MOG_DMAX; ++r)
    if (r < D) {
      const float v = mu[r] + x[r];
      theta_out[i * D + r] = shift ? v * scale[r] + shift[r] : v;
    }
}

int mog_envelope(int64_t M, int D) {
  if (D < 1 || M < 1) return SBI_AMD_E_BADARG;
  if (D > MOG_DMAX || M > MOG_MMAX) return SBI_AMD_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" int64_t sbi_amd_mog_correct_workspace_bytes(int64_t B, int32_t K, int32_t L, int32_t D, int64_t prop_rows) {
  if (B < 0 || K < 1 || L < 1 || (B > 0 && prop_rows != 1 && prop_rows != B)) return SBI_AMD_E_BADARG;
  const int rc = mog_envelope((int64_t)K * L, D);
  if (rc) return rc;
  return (int64_t)sizeof(double) * MOG_TAB * (B * K + prop_rows * L);
}

extern "C" int sbi_amd_mog_correct(const float* d_logits, const float* d_means, const float* d_prec, int64_t B,
                                   int32_t K, const float* p_logits, const float* p_means, const float* p_prec,
                                   int64_t prop_rows, int32_t L, int32_t D, const float* prior_mean,
                                   const float* prior_prec, float eps, float* logits_out, float* means_out,
                                   float* prec_out, float* factor_out, int32_t* status, void* workspace,
                                   void* stream) {
  if (B < 0 || K < 1 || L < 1) return SBI_AMD_E_BADARG;
  const int rc = mog_envelope((int64_t)K * L, D);
  if (rc) return rc;
  if (B == 0) return 0;
  if (!d_logits || !d_means || !d_prec || !p_logits || !p_means || !p_prec || !logits_out || !means_out ||
      !prec_out || !factor_out || !status || !workspace || (prop_rows != 1 && prop_rows != B) ||
      ((prior_mean == nullptr) != (prior_prec == nullptr)) || !(eps >= 0.f))
    return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const long long n_d = B * K, n_p = prop_rows * L;
  double* tab = (double*)workspace;
  hipLaunchKernelGGL(mog_table_kernel, dim3((unsigned)((n_d + n_p + MOG_PAIRS - 1) / MOG_PAIRS)), dim3(256), 0, st,
                     d_means, d_prec, n_d, p_means, p_prec, n_p, (int)D, tab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(status, 0x7f, sizeof(int32_t) * (size_t)B, st);
  if (e != hipSuccess) return (int)e;
  MogCorrectArgs A;
  A.d_logits = d_logits; A.d_prec = d_prec; A.p_logits = p_logits; A.p_prec = p_prec;
  A.prior_mean = prior_mean; A.prior_prec = prior_prec; A.tab = tab;
  A.B = B; A.prop_rows = prop_rows; A.K = K; A.L = L; A.D = D; A.M = K * L;
  A.eps = (double)eps;
  A.logits_out = logits_out; A.means_out = means_out; A.prec_out = prec_out; A.factor_out = factor_out;
  A.status = status;
  const long long pairs = B * (long long)A.M;
  hipLaunchKernelGGL(mog_pair_kernel, dim3((unsigned)((pairs + MOG_PAIRS - 1) / MOG_PAIRS)), dim3(256), 0, st, A);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mog_status_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, status, (long long)B);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_mog_log_prob(const float* logits, const float* means, const float* prec, const float* factors,
                                    int64_t mog_rows, int32_t M, int32_t D, const float* theta, int64_t n,
                                    const float* shift, const float* scale, float* out, void* stream) {
  if (n < 0 || mog_rows < 1) return SBI_AMD_E_BADARG;
  const int rc = mog_envelope(M, D);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!logits || !means || !prec || !factors || !theta || !out || ((shift == nullptr) != (scale == nullptr)))
    return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (mog_rows == 1)
    hipLaunchKernelGGL(mog_logp_bcast_kernel, dim3((unsigned)((n + LP_ROWS - 1) / LP_ROWS)), dim3(256), 0, st, logits,
                       means, prec, factors, (int)M, (int)D, theta, (long long)n, shift, scale, out);
  else
    hipLaunchKernelGGL(mog_logp_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, logits, means, prec,
                       factors, (long long)mog_rows, (int)M, (int)D, theta, (long long)n, shift, scale, out);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_mog_sample(const float* logits, const float* means, const float* factors, int64_t mog_rows,
                                  int32_t M, int32_t D, const float* u, const int32_t* comp, const float* zeta,
                                  int64_t n, const float* shift, const float* scale, float* theta_out,
                                  void* cdf_workspace, void* stream) {
  if (n < 0 || mog_rows < 1) return SBI_AMD_E_BADARG;
  const int rc = mog_envelope(M, D);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!means || !factors || !zeta || !theta_out || (!u && !comp) || ((shift == nullptr) != (scale == nullptr)) ||
      (!comp && (!logits || !cdf_workspace)))
    return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (!comp) {
    hipLaunchKernelGGL(mog_cdf_kernel, dim3((unsigned)mog_rows), dim3(256), 0, st, logits, (int)M,
                       (double*)cdf_workspace);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(mog_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, means, factors,
                     (long long)mog_rows, (int)M, (int)D, u, comp, zeta, (long long)n, shift, scale, theta_out,
                     (const double*)cdf_workspace);
  return (int)hipGetLastError();
}
