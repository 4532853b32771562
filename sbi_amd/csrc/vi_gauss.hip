// vi_gauss.hip -- the Gaussian variational family of VIPosterior (sbi/samplers/vi/vi_utils.py `LearnableGaussian`) and
// one iteration of its divergence optimisers (vi_divergence_optimizers.py: rKL, IW, alpha, fKL) around the potential.
// Semantics, the link table, the Philox stream and the gradient formulas: include/sbi_amd_vi.h.
//   * draw / log_prob: one thread per row; phi and the link table are staged in LDS once per workgroup (broadcast reads).
//   * step: ONE workgroup of 512 threads.  Pass 1 regenerates eps, z, log q per row and leaves e_i = p_i - log q_i in
//     the workspace; pass 2 takes the normalisers (block reductions in a fixed order; IW: one thread per group of K);
//     pass 3 walks tiles of 512 rows: every thread writes c_i a_i and eps_i of its row into an LDS tile (augmented by
//     c_i and by a column of ones, so that sum c a eps^T, sum c a and sum c are ONE (D+1) x (D+1) product), then the
//     threads own output entries and run down the tile serially -- plain FMAs, a fixed order, no atomics.  The tail
//     (clip, Adam through adam_math.h, the non-finite guard, the snapshot) runs in the same launch.
//   * eps and z come from the same two inline functions in all kernels, with every multiply-add an explicit fmaf: a
//     row's eps / z bits do not depend on the kernel, on n or on the row's place in the grid.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <atomic>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_vi.h"
#include "adam_math.h"
#include "philox.h"

#define VI_D 16                                   // SBI_AMD_VI_MAX_D: the unrolled register arrays
#define VI_STREAM_TAG 0x56494731u                 // "VIG1": keeps this stream apart from the samplers' (philox.h)
#define VI_DRAW_THREADS 256
#define VI_STEP_THREADS 512
#define VI_TILE 512                               // rows per tile of the step kernel (= its workgroup size)
#define VI_TS (VI_TILE + 1)                       // LDS row stride: rows k, k + 1 of the tile land in different banks
#define VI_MAX_DEVICES 64
#define VI_LOG_2PI_HALF 0.9189385332046727f

struct ViShared {
  float mu[VI_D];
  float L[VI_D * VI_D];      // lower triangle (diag family: exp(s) on the diagonal), zero elsewhere and for d >= D
  float logLd[VI_D];         // log L_dd (diag family: s_d itself)
  float kind[VI_D], a[VI_D], b[VI_D], lo_in[VI_D], hi_in[VI_D], logb[VI_D];
};

// every thread of the workgroup calls this; ends with a barrier
__device__ __forceinline__ void vi_load(ViShared& S, const float* __restrict__ phi, const float* __restrict__ link, int D,
                                        int full) {
  for (int i = threadIdx.x; i < VI_D * VI_D; i += blockDim.x) {
    const int d = i >> 4, k = i & 15;
    float v = 0.f;
    if (d < D && k <= d) {
      if (full) v = phi[D + d * D + k];
      else if (k == d) v = expf(phi[D + d]);
    }
    S.L[i] = v;
  }
  for (int d = threadIdx.x; d < VI_D; d += blockDim.x) {
    const bool in = d < D;
    S.mu[d] = in ? phi[d] : 0.f;
    S.logLd[d] = in ? (full ? logf(phi[D + d * D + d]) : phi[D + d]) : 0.f;
    float kind = 0.f, a = 0.f, b = 1.f, c = 0.f;
    if (in && link) {
      kind = link[d];
      a = link[D + d];
      b = link[2 * D + d];
      c = link[3 * D + d];
    }
    S.kind[d] = kind;
    S.a[d] = a;
    S.b[d] = b;
    S.lo_in[d] = nextafterf(a, INFINITY);
    S.hi_in[d] = nextafterf(c, -INFINITY);
    S.logb[d] = logf(fabsf(b));
  }
  __syncthreads();
}

__device__ __forceinline__ void vi_eps(unsigned long long seed, unsigned step, unsigned long long row, int D,
                                       float (&eps)[VI_D]) {
#pragma unroll
  for (int j = 0; j < VI_D / 4; ++j) {
    if (4 * j < D) {
      unsigned o[4];
      philox4x32_10((unsigned)row, (unsigned)(row >> 32), step, VI_STREAM_TAG + (unsigned)j, (unsigned)seed,
                    (unsigned)(seed >> 32), o);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((o[2 * h] >> 8) + 1u) * (1.0f / 16777216.0f);      // (0, 1]
        const float rad = sqrtf(-2.f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u01(o[2 * h + 1]), &sn, &cs);
        eps[4 * j + 2 * h] = 4 * j + 2 * h < D ? rad * cs : 0.f;
        eps[4 * j + 2 * h + 1] = 4 * j + 2 * h + 1 < D ? rad * sn : 0.f;
      }
    } else {
#pragma unroll
      for (int h = 0; h < 4; ++h) eps[4 * j + h] = 0.f;
    }
  }
}

__device__ __forceinline__ void vi_z(const ViShared& S, const float (&eps)[VI_D], float (&z)[VI_D]) {
#pragma unroll
  for (int d = 0; d < VI_D; ++d) {
    float acc = S.mu[d];
#pragma unroll
    for (int k = 0; k <= d; ++k) acc = __builtin_fmaf(S.L[d * VI_D + k], eps[k], acc);
    z[d] = acc;
  }
}

// theta_d, log|T'(z_d)|, J = T'(z_d), h = d/dz log|T'(z_d)|
__device__ __forceinline__ void vi_link(const ViShared& S, int d, float z, float& th, float& ld, float& J, float& h) {
  const float kind = S.kind[d], a = S.a[d], b = S.b[d];
  if (kind == 0.f) {
    th = __builtin_fmaf(b, z, a);
    ld = S.logb[d];
    J = b;
    h = 0.f;
  } else if (kind == 1.f) {
    const float s = 1.f / (1.f + expf(-z));
    const float sc = fminf(fmaxf(s, FLT_MIN), 1.f - FLT_EPSILON);
    th = fminf(fmaxf(__builtin_fmaf(b, sc, a), S.lo_in[d]), S.hi_in[d]);
    ld = -fabsf(z) - 2.f * log1pf(expf(-fabsf(z))) + S.logb[d];     // -softplus(-z) - softplus(z) + log b
    J = b * s * (1.f - s);
    h = 1.f - 2.f * s;
  } else {
    const float e = expf(z);
    th = kind == 2.f ? a + e : a - e;
    ld = z;
    J = kind == 2.f ? e : -e;
    h = 1.f;
  }
}

__device__ __forceinline__ float vi_log_q(const ViShared& S, int D, float sq, float sum_ld) {
  float sl = 0.f;
#pragma unroll
  for (int d = 0; d < VI_D; ++d) sl += S.logLd[d];                 // (zero for d >= D)
  return -0.5f * sq - (float)D * VI_LOG_2PI_HALF - sl - sum_ld;
}

__global__ void __launch_bounds__(VI_DRAW_THREADS)
vi_draw_kernel(int D, int full, const float* __restrict__ phi, const float* __restrict__ link, long long n,
               unsigned long long seed, unsigned step, unsigned long long row_offset, float* __restrict__ theta,
               float* __restrict__ log_q, float* __restrict__ eps_out) {
  __shared__ ViShared S;
  vi_load(S, phi, link, D, full);
  const long long r = (long long)blockIdx.x * VI_DRAW_THREADS + threadIdx.x;
  if (r >= n) return;
  float eps[VI_D], z[VI_D];
  vi_eps(seed, step, (unsigned long long)r + row_offset, D, eps);
  vi_z(S, eps, z);
  float sq = 0.f, sum_ld = 0.f;
#pragma unroll
  for (int d = 0; d < VI_D; ++d) {
    if (d < D) {
      float th, ld, J, h;
      vi_link(S, d, z[d], th, ld, J, h);
      theta[r * D + d] = th;
      if (eps_out) eps_out[r * D + d] = eps[d];
      sq = __builtin_fmaf(eps[d], eps[d], sq);
      sum_ld += ld;
    }
  }
  log_q[r] = vi_log_q(S, D, sq, sum_ld);
}

__global__ void __launch_bounds__(VI_DRAW_THREADS)
vi_log_prob_kernel(int D, int full, const float* __restrict__ phi, const float* __restrict__ link,
                   const float* __restrict__ theta, long long n, float* __restrict__ log_q) {
  __shared__ ViShared S;
  vi_load(S, phi, link, D, full);
  const long long r = (long long)blockIdx.x * VI_DRAW_THREADS + threadIdx.x;
  if (r >= n) return;
  float eps[VI_D];
  float sq = 0.f, sum_ld = 0.f;
#pragma unroll
  for (int d = 0; d < VI_D; ++d) {
    eps[d] = 0.f;
    if (d < D) {
      const float th = theta[r * D + d], kind = S.kind[d], a = S.a[d], b = S.b[d];
      float z, ld;
      if (kind == 0.f) {
        z = (th - a) / b;
        ld = S.logb[d];
      } else if (kind == 1.f) {
        const float y = fminf(fmaxf((th - a) / b, FLT_MIN), 1.f - FLT_EPSILON);
        z = logf(y) - log1pf(-y);
        ld = -fabsf(z) - 2.f * log1pf(expf(-fabsf(z))) + S.logb[d];
      } else {
        z = logf(kind == 2.f ? th - a : a - th);
        ld = z;
      }
      float acc = z - S.mu[d];
#pragma unroll
      for (int k = 0; k < d; ++k) acc = __builtin_fmaf(-S.L[d * VI_D + k], eps[k], acc);
      eps[d] = acc / S.L[d * VI_D + d];
      sq = __builtin_fmaf(eps[d], eps[d], sq);
      sum_ld += ld;
    }
  }
  log_q[r] = vi_log_q(S, D, sq, sum_ld);
}

// ---- the step kernel ------------------------------------------------------------------------------------------------
// Block reductions over VI_STEP_THREADS values in a fixed tree; `red` has VI_STEP_THREADS floats; ends with a barrier, so
// `red` can be reused at once.
__device__ __forceinline__ float vi_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = VI_STEP_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const float out = red[0];
  __syncthreads();
  return out;
}
__device__ __forceinline__ float vi_block_max(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = VI_STEP_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const float out = red[0];
  __syncthreads();
  return out;
}

struct ViStepArgs {
  int D, full, method, K, stl, dreg, unbiased;
  float beta, loss_scale;              // alpha: beta = (1 - alpha) or (1 - alpha)^2; loss_scale = 1 / (1 - alpha)
  int n, P;
  float clip, lr, beta1, beta2, eps, bc1, bc2_sqrt;
  long long t;
  unsigned long long seed;
  unsigned step;
  int ring_size;
};

__global__ void __launch_bounds__(VI_STEP_THREADS)
vi_step_kernel(ViStepArgs A, const float* __restrict__ p, const float* __restrict__ r, float* __restrict__ phi,
               float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, float* __restrict__ snapshot,
               const float* __restrict__ link, float* __restrict__ ws, float* __restrict__ ring,
               int* __restrict__ status, float* __restrict__ grad_out) {
  extern __shared__ float vi_tile[];               // ca: (D + 1) rows of VI_TS, then ep: (D + 1) rows of VI_TS
  __shared__ ViShared S;
  __shared__ float red[VI_STEP_THREADS];
  __shared__ float part[VI_STEP_THREADS];          // the accumulate phase's partial sums, q-major
  __shared__ float G[(VI_D + 1) * (VI_D + 1)];
  const int tid = threadIdx.x, D = A.D, n = A.n, D1 = D + 1, NE = D1 * D1;
  const bool fkl = A.method == SBI_AMD_VI_FKL;
  vi_load(S, phi, link, D, A.full);
  float* __restrict__ ws_e = ws;                   // e_i (n)
  float* __restrict__ ws_g = ws + n;               // IW: logsumexp of every group (n / K)

  // ---- pass 1: e_i = p_i - log q_i; this thread's partial sum / maximum over its rows (tid, tid + 512, ...)
  float s_e = 0.f, mx = -INFINITY;
  for (int i = tid; i < n; i += VI_STEP_THREADS) {
    float eps[VI_D], z[VI_D];
    vi_eps(A.seed, A.step, (unsigned long long)i, D, eps);
    vi_z(S, eps, z);
    float sq = 0.f, sum_ld = 0.f;
#pragma unroll
    for (int d = 0; d < VI_D; ++d) {
      if (d < D) {
        float th, ld, J, h;
        vi_link(S, d, z[d], th, ld, J, h);
        sq = __builtin_fmaf(eps[d], eps[d], sq);
        sum_ld += ld;
      }
    }
    const float e = p[i] - vi_log_q(S, D, sq, sum_ld);
    ws_e[i] = e;
    s_e += e;
    mx = fmaxf(mx, A.method == SBI_AMD_VI_ALPHA ? A.beta * e : e);
  }
  __syncthreads();                                 // (ws_e is read by other threads of this workgroup below)

  // ---- pass 2: the normalisers and the displayed loss
  float loss = 0.f, M = 0.f, lnorm = 0.f;          // c_i = exp(x_i - lnorm) * scale (see pass 3)
  const float logn = logf((float)n);
  if (A.method == SBI_AMD_VI_RKL) {
    loss = -vi_block_sum(s_e, red) / (float)n;
  } else if (A.method == SBI_AMD_VI_IW) {
    const int K = A.K, ng = n / K;
    float acc = 0.f;
    for (int g = tid; g < ng; g += VI_STEP_THREADS) {
      const float* __restrict__ eg = ws_e + (long long)g * K;
      float m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmaxf(m, eg[k]);
      float zs = 0.f;
      for (int k = 0; k < K; ++k) zs += expf(eg[k] - m);
      const float lse = m + logf(zs);
      ws_g[g] = lse;
      acc += lse - logf((float)K);
    }
    loss = -vi_block_sum(acc, red) / (float)ng;     // (the barriers inside also publish ws_g)
  } else {
    M = vi_block_max(mx, red);
    float zs = 0.f;
    for (int i = tid; i < n; i += VI_STEP_THREADS)
      zs += expf((A.method == SBI_AMD_VI_ALPHA ? A.beta * ws_e[i] : ws_e[i]) - M);
    const float Z = vi_block_sum(zs, red);
    lnorm = M + logf(Z);
    if (fkl) {
      float acc = 0.f;
      for (int i = tid; i < n; i += VI_STEP_THREADS) acc += expf(ws_e[i] - lnorm) * ws_e[i];
      loss = vi_block_sum(acc, red);
    } else {
      loss = -(lnorm - logn) * A.loss_scale;
    }
  }

  // ---- pass 3: G = sum_i [c a | c]_i [eps | 1]_i^T over tiles of VI_TILE rows
  float* __restrict__ ca = vi_tile;
  float* __restrict__ ep = vi_tile + D1 * VI_TS;
  int Q = VI_STEP_THREADS / NE;
  if (Q > 16) Q = 16;
  const int chunk = (VI_TILE + Q - 1) / Q;
  const bool owner = tid < Q * NE;
  const int oq = tid / NE, oe = tid % NE, od = oe / D1, ok = oe % D1;
  const int i0 = oq * chunk, i1 = min(VI_TILE, i0 + chunk);
  const bool need_b = fkl || A.stl;
  float acc = 0.f;
  for (int tb = 0; tb < n; tb += VI_TILE) {
    const int i = tb + tid;
    float cav[VI_D], eps[VI_D], c = 0.f;
#pragma unroll
    for (int d = 0; d < VI_D; ++d) { cav[d] = 0.f; eps[d] = 0.f; }
    if (i < n) {
      float z[VI_D], b[VI_D];
      vi_eps(A.seed, A.step, (unsigned long long)i, D, eps);
      vi_z(S, eps, z);
      if (need_b) {                                  // b = L^-T eps: back substitution
#pragma unroll
        for (int d = VI_D - 1; d >= 0; --d) {
          b[d] = 0.f;
          if (d < D) {
            float v = eps[d];
#pragma unroll
            for (int k = d + 1; k < VI_D; ++k) v = __builtin_fmaf(-S.L[k * VI_D + d], b[k], v);
            b[d] = v / S.L[d * VI_D + d];
          }
        }
      }
      const float e = ws_e[i];
      if (A.method == SBI_AMD_VI_RKL) {
        c = 1.f / (float)n;
      } else if (A.method == SBI_AMD_VI_IW) {
        const float w = expf(e - ws_g[i / A.K]);
        c = (A.dreg ? w * w : w) / (float)(n / A.K);
      } else if (fkl) {
        c = expf(e - lnorm);
      } else if (A.unbiased) {
        c = A.beta * expf(A.beta * e - logn);
      } else {
        const float w = expf(A.beta * e - (lnorm - logn));
        c = (A.dreg ? w * w : w) / (float)n;
      }
#pragma unroll
      for (int d = 0; d < VI_D; ++d) {
        if (d < D) {
          float a = 0.f;
          if (!fkl) {
            float th, ld, J, h;
            vi_link(S, d, z[d], th, ld, J, h);
            a = __builtin_fmaf(J, r[(long long)i * D + d], h);
          }
          if (need_b) a += b[d];
          cav[d] = c * a;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < VI_D; ++d) {
      if (d < D) {
        ca[d * VI_TS + tid] = cav[d];
        ep[d * VI_TS + tid] = eps[d];
      }
    }
    ca[D * VI_TS + tid] = c;
    ep[D * VI_TS + tid] = i < n ? 1.f : 0.f;
    __syncthreads();
    if (owner) {
      const float* __restrict__ pa = ca + od * VI_TS;
      const float* __restrict__ pe = ep + ok * VI_TS;
#pragma unroll 4
      for (int j = i0; j < i1; ++j) acc = __builtin_fmaf(pa[j], pe[j], acc);
    }
    __syncthreads();
  }
  part[tid] = owner ? acc : 0.f;
  __syncthreads();
  if (tid < NE) {
    float s = 0.f;
    for (int q = 0; q < Q; ++q) s += part[q * NE + tid];
    G[tid] = s;
  }
  __syncthreads();

  // ---- the gradient of the surrogate loss
  const int P = A.P;
  float g = 0.f;
  if (tid < P) {
    const float sum_c = G[D * D1 + D];
    const float diagcoef = fkl ? 1.f : (A.stl ? 0.f : -sum_c);
    if (tid < D) {
      g = -G[tid * D1 + D];
    } else if (A.full) {
      const int d = (tid - D) / D, k = (tid - D) % D;
      if (k < d) g = -G[d * D1 + k];
      else if (k == d) g = -G[d * D1 + d] + diagcoef / S.L[d * VI_D + d];
    } else {
      const int d = tid - D;
      g = -G[d * D1 + d] * S.L[d * VI_D + d] + diagcoef;
    }
  }
  const bool finite_g = (g - g) == 0.f;            // false for NaN and +-inf
  const int bad = __syncthreads_or((!finite_g) || (tid == 0 && !((loss - loss) == 0.f)));
  if (bad) {                                       // restore, forget the moments, count; nothing else is written
    if (tid < P) {
      phi[tid] = snapshot[tid];
      exp_avg[tid] = 0.f;
      exp_avg_sq[tid] = 0.f;
    }
    if (tid == 0) status[0] += 1;
    return;
  }
  const float norm = sqrtf(vi_block_sum(tid < P ? g * g : 0.f, red));
  const float coef = A.clip > 0.f ? fminf(A.clip / (norm + 1e-6f), 1.f) : 1.f;      // clip_grad_norm_
  const AdamK k = {coef, A.beta1, A.beta2, A.eps, A.lr / A.bc1, A.bc2_sqrt};
  float pn = 0.f;
  if (tid < P) {
    float mi = exp_avg[tid], vi = exp_avg_sq[tid];
    pn = adam_apply_one(phi[tid], g, mi, vi, k);     // (roundings pinned: adam_math.h)
    phi[tid] = pn;
    exp_avg[tid] = mi;
    exp_avg_sq[tid] = vi;
    if (grad_out) grad_out[tid] = g;
  }
  if (tid == 0) {
    ring[(int)(A.t % A.ring_size)] = loss;
    status[2] = (int)A.t;
  }
  if (A.t % 50 == 0) {
    const int nonfinite = __syncthreads_or(tid < P && !((pn - pn) == 0.f));
    if (!nonfinite) {
      if (tid < P) snapshot[tid] = pn;
      if (tid == 0) status[1] += 1;
    }
  }
}

static size_t vi_step_lds(int D) { return (size_t)2 * (D + 1) * VI_TS * sizeof(float); }

extern "C" int sbi_amd_vi_gauss_plan(int32_t D, int64_t n_rows, int64_t* workspace_bytes) {
  if (D < 1 || n_rows < 1 || !workspace_bytes) return SBI_AMD_E_BADARG;
  if (D > SBI_AMD_VI_MAX_D || n_rows > SBI_AMD_VI_MAX_PARTICLES) return SBI_AMD_E_UNSUPPORTED;
  *workspace_bytes = 2 * n_rows * (int64_t)sizeof(float);
  return 0;
}

extern "C" int sbi_amd_vi_gauss_draw(int32_t D, int32_t full_cov, const float* phi, const float* link, int64_t n,
                                     uint64_t seed, uint32_t step, uint64_t row_offset, float* theta, float* log_q,
                                     float* eps_out, void* stream) {
  if (!phi || !theta || !log_q || D < 1 || n < 0) return SBI_AMD_E_BADARG;
  if (D > SBI_AMD_VI_MAX_D) return SBI_AMD_E_UNSUPPORTED;
  if (n == 0) return 0;
  const int64_t blocks = (n + VI_DRAW_THREADS - 1) / VI_DRAW_THREADS;
  if (blocks > 0x7fffffffll) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(vi_draw_kernel, dim3((unsigned)blocks), dim3(VI_DRAW_THREADS), 0, (hipStream_t)stream, (int)D,
                     (int)full_cov, phi, link, (long long)n, (unsigned long long)seed, (unsigned)step,
                     (unsigned long long)row_offset, theta, log_q, eps_out);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_vi_gauss_log_prob(int32_t D, int32_t full_cov, const float* phi, const float* link,
                                         const float* theta, int64_t n, float* log_q, void* stream) {
  if (!phi || !theta || !log_q || D < 1 || n < 0) return SBI_AMD_E_BADARG;
  if (D > SBI_AMD_VI_MAX_D) return SBI_AMD_E_UNSUPPORTED;
  if (n == 0) return 0;
  const int64_t blocks = (n + VI_DRAW_THREADS - 1) / VI_DRAW_THREADS;
  if (blocks > 0x7fffffffll) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(vi_log_prob_kernel, dim3((unsigned)blocks), dim3(VI_DRAW_THREADS), 0, (hipStream_t)stream, (int)D,
                     (int)full_cov, phi, link, theta, (long long)n, log_q);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_vi_gauss_step(const sbi_amd_vi_config* cfg, const float* p, const float* r, int64_t n, float* phi,
                                     float* exp_avg, float* exp_avg_sq, float* snapshot, const float* link,
                                     float clip_value, float lr_t, float beta1, float beta2, float eps, int64_t t,
                                     uint64_t seed, uint32_t step, float* workspace, float* ring, int32_t ring_size,
                                     int32_t* status, float* grad_out, void* stream) {
  if (!cfg || !p || !phi || !exp_avg || !exp_avg_sq || !snapshot || !workspace || !ring || !status || ring_size < 1 ||
      t < 1 || n < 1 || cfg->D < 1)
    return SBI_AMD_E_BADARG;
  if (cfg->D > SBI_AMD_VI_MAX_D || n > SBI_AMD_VI_MAX_PARTICLES) return SBI_AMD_E_UNSUPPORTED;
  if (cfg->method < SBI_AMD_VI_RKL || cfg->method > SBI_AMD_VI_FKL) return SBI_AMD_E_BADARG;
  if (cfg->method != SBI_AMD_VI_FKL && !r) return SBI_AMD_E_BADARG;
  if (cfg->method == SBI_AMD_VI_IW && (cfg->K < 1 || n % cfg->K != 0)) return SBI_AMD_E_BADARG;
  if (cfg->method == SBI_AMD_VI_ALPHA && cfg->alpha == 1.f) return SBI_AMD_E_BADARG;
  ViStepArgs A;
  A.D = cfg->D;
  A.full = cfg->full_cov != 0;
  A.method = cfg->method;
  A.K = cfg->method == SBI_AMD_VI_IW ? cfg->K : 1;
  A.stl = cfg->method != SBI_AMD_VI_FKL && (cfg->stick_the_landing != 0);
  A.dreg = cfg->dreg != 0;
  A.unbiased = cfg->method == SBI_AMD_VI_ALPHA && cfg->unbiased != 0;
  const float oma = 1.f - cfg->alpha;
  A.beta = A.unbiased ? oma * oma : oma;
  A.loss_scale = cfg->method == SBI_AMD_VI_ALPHA ? 1.f / oma : 0.f;
  A.n = (int)n;
  A.P = A.full ? A.D + A.D * A.D : 2 * A.D;
  A.clip = clip_value;
  A.lr = lr_t;
  A.beta1 = beta1;
  A.beta2 = beta2;
  A.eps = eps;
  A.bc1 = (float)(1.0 - pow((double)beta1, (double)t));            // as adam.hip's launcher
  A.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)t));
  A.t = t;
  A.seed = seed;
  A.step = step;
  A.ring_size = ring_size;
  // (more than 64 KiB of dynamic LDS has to be asked for, on the device that is current, as the other launchers do)
  // once per device: the step is launched every training iteration, a latency-bound path
  static std::atomic<bool> lds_asked[VI_MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= VI_MAX_DEVICES) return SBI_AMD_E_UNSUPPORTED;
  if (!lds_asked[dev].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute((const void*)vi_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)vi_step_lds(SBI_AMD_VI_MAX_D)) != hipSuccess)
      return SBI_AMD_E_UNSUPPORTED;
    lds_asked[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(vi_step_kernel, dim3(1), dim3(VI_STEP_THREADS), vi_step_lds(A.D), (hipStream_t)stream, A, p, r, phi,
                     exp_avg, exp_avg_sq, snapshot, link, workspace, ring, status, grad_out);
  return (int)hipGetLastError();
}
