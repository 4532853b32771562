// causal_cnn_kernel.h -- the dilated causal stack + average pool of CausalCNNEmbedding on gfx950: plan, device
// functions, kernels (launchers: causal_cnn.hip).  Contract: include/sbi_amd_causal_cnn.h.
//
// Execution model
//   * a workgroup is 8 waves (forward) or 16 (backward) and owns (sequence, segment) pairs: unit = group, group + G,
//     ...; a segment is segw whole pooling windows and is walked in tiles [a, b) of at most TS output steps.  The
//     weights are staged once per workgroup in LDS, rows padded to an odd stride.  When a segment is shorter than TS
//     (segw pool <= TS) it is the only tile, and the LDS image is laid out for its length.
//   * map l of a tile lives in LDS channel-major, row stride ms[l] (odd), index i <-> time a - H[l] + i, on n + H[l]
//     steps.  Layer l is then out[co][m] = sum_{ci, j} in[ci][m + j d] w[co][ci][j]: the halo shrinks by d (k - 1) and
//     the tap shift is a plain index offset.  Steps left of t = 0 are forced to 0 in every map (the causal pad).
//   * all three GEMMs run on v_mfma_f32_16x16x4_f32 with guarded operand loads (an element outside M, N or K is an
//     exact 0, never a stale value); a 16 x 16 output tile belongs to one wave and every element to one lane.
//       forward   M = time, N = C_out, K = (ci, j)      bias and LeakyReLU from the accumulators
//       dW, db    M = C_out, N = (ci, j) and one column of ones (the bias), K = time; accumulated in LDS
//       dgrad     M = time, N = C_in, K = (co, j)       LeakyReLU' from the stored output, 0 left of t = 0
//     MFMA operand layout: lane l gives A[m = l % 16][k = l / 16] and B[k = l / 16][n = l % 16]; it holds
//     D[4 (l / 16) + i][l % 16].
//   * forward: two alternating maps; the last layer's tile is summed into the segment's pool sums by one thread per
//     (channel, window) in ascending time.  backward: all maps of the cone stay, two alternating gradient maps.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_causal_cnn.h"
#include "../../include/sbi_amd_nsf.h"

namespace {

#define CC_THREADS 512              // forward: 8 waves
#define CC_BWD_THREADS 1024         // backward: 16 waves, one workgroup per CU at the LDS limit
#define CC_CHUNK 16                 // time steps of one MFMA chain of the weight gradient
#define CC_MAX_LAYERS 16
#define CC_MAX_CHANNELS 32
#define CC_GROUPS 512               // most workgroups of a backward launch: units beyond walk the grid again
#define CC_FWD_GROUPS 4096          // ... of a forward launch
#define CC_LDS_BUDGET (160 * 1024)
#define CC_MAX_TILE 2048
#define CC_MAX_T (1 << 20)

typedef float cc_f4 __attribute__((ext_vector_type(4)));

struct CcPlan {
  int C0, T, L, k, pool, Tp, R, TS, segw, nseg, P;
  float slope, inv_pool;
  int C[CC_MAX_LAYERS + 1];          // channels of map l
  int d[CC_MAX_LAYERS];
  int H[CC_MAX_LAYERS + 1];          // halo of map l
  int ms[CC_MAX_LAYERS + 1];         // row stride of map l (and of its gradient)
  int CK[CC_MAX_LAYERS], ws[CC_MAX_LAYERS];
  int p_w[CC_MAX_LAYERS], p_b[CC_MAX_LAYERS];                       // offsets in the flat parameters
  int o_w[CC_MAX_LAYERS], o_b[CC_MAX_LAYERS], o_g[CC_MAX_LAYERS];   // LDS offsets (floats)
  int o_map[CC_MAX_LAYERS + 1];      // backward: every map
  int o_gbuf[2];                     // backward: gradient map of layer l in o_gbuf[l & 1]
  int o_fbuf[2], o_pool;             // forward: map l in o_fbuf[l & 1], the segment's pool sums
  int fwd_floats, bwd_floats;
};

// sizes that do not depend on the tile
static int cc_plan_sizes(const sbi_amd_ccnn_config* cfg, CcPlan* out) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->in_channels < 1 || cfg->T < 1 || cfg->num_conv_layers < 1 || cfg->kernel_size < 1 ||
      cfg->pool_kernel_size < 1)
    return SBI_AMD_E_BADARG;
  if (cfg->num_conv_layers > CC_MAX_LAYERS) return SBI_AMD_E_UNSUPPORTED;
  for (int l = 0; l < cfg->num_conv_layers; ++l)
    if (cfg->out_channels[l] < 1 || cfg->dilation[l] < 1) return SBI_AMD_E_BADARG;
  if (cfg->in_channels > CC_MAX_CHANNELS || cfg->kernel_size < 2 || cfg->kernel_size > 4 || cfg->T > CC_MAX_T ||
      cfg->pool_kernel_size > cfg->T)
    return SBI_AMD_E_UNSUPPORTED;
  if (!(cfg->negative_slope >= 0.f) || isinf(cfg->negative_slope)) return SBI_AMD_E_UNSUPPORTED;
  CcPlan p = {};
  p.C0 = cfg->in_channels; p.T = cfg->T; p.L = cfg->num_conv_layers; p.k = cfg->kernel_size;
  p.pool = cfg->pool_kernel_size; p.Tp = p.T / p.pool;
  p.slope = cfg->negative_slope; p.inv_pool = 1.f / (float)p.pool;
  p.C[0] = p.C0;
  int off = 0;
  for (int l = 0; l < p.L; ++l) {
    if (cfg->out_channels[l] > CC_MAX_CHANNELS || cfg->dilation[l] >= cfg->T) return SBI_AMD_E_UNSUPPORTED;
    p.C[l + 1] = cfg->out_channels[l];
    p.d[l] = cfg->dilation[l];
    p.CK[l] = p.C[l] * p.k;
    p.ws[l] = p.CK[l] | 1;
    p.p_w[l] = off; off += p.C[l + 1] * p.CK[l];
    p.p_b[l] = off; off += p.C[l + 1];
  }
  p.P = off;
  p.H[p.L] = 0;
  for (int l = p.L - 1; l >= 0; --l) p.H[l] = p.H[l + 1] + p.d[l] * (p.k - 1);    // < 16 x 3 x 2^20: no overflow
  p.R = p.H[0];
  *out = p;
  return 0;
}

// LDS offsets for tiles of ts steps; `shrink`: for the steps a tile can really have, a whole segment when that is
// shorter
static void cc_layout(CcPlan* p, int ts, bool shrink) {
  p->TS = ts;
  p->segw = ts / p->pool > 1 ? ts / p->pool : 1;
  p->nseg = (p->Tp + p->segw - 1) / p->segw;
  if (shrink && p->pool <= ts) ts = p->segw * p->pool;
  long long o = 0;
  for (int l = 0; l < p->L; ++l) {
    p->o_w[l] = (int)o; o += p->C[l + 1] * p->ws[l];
    p->o_b[l] = (int)o; o += p->C[l + 1];
  }
  const long long weights = o;
  long long par[2] = {0, 0}, gpar[2] = {0, 0};
  for (int l = 0; l <= p->L; ++l) {
    p->ms[l] = (ts + p->H[l]) | 1;
    const long long sz = (long long)p->C[l] * p->ms[l];
    if (sz > par[l & 1]) par[l & 1] = sz;
    if (l >= 1 && sz > gpar[l & 1]) gpar[l & 1] = sz;
  }
  // forward
  p->o_fbuf[0] = (int)o; o += par[0];
  p->o_fbuf[1] = (int)o; o += par[1];
  p->o_pool = (int)o; o += (long long)p->C[p->L] * p->segw;
  p->fwd_floats = o > INT32_MAX / 4 ? INT32_MAX / 4 : (int)o;
  // backward
  o = weights;
  for (int l = 0; l < p->L; ++l) { p->o_g[l] = (int)o; o += p->C[l + 1] * (p->CK[l] + 1); }
  for (int l = 0; l <= p->L; ++l) {
    p->o_map[l] = (int)(o > INT32_MAX ? INT32_MAX : o);
    o += (long long)p->C[l] * p->ms[l];
  }
  p->o_gbuf[0] = (int)(o > INT32_MAX ? INT32_MAX : o); o += gpar[0];
  p->o_gbuf[1] = (int)(o > INT32_MAX ? INT32_MAX : o); o += gpar[1];
  p->bwd_floats = o > INT32_MAX / 4 ? INT32_MAX / 4 : (int)o;
}

static bool cc_fits(const CcPlan& p) {
  return (long long)p.bwd_floats * 4 <= CC_LDS_BUDGET && (long long)p.fwd_floats * 4 <= CC_LDS_BUDGET;
}

// the largest tile that fits, or E_LDS (the plan then describes the 16-step tile)
static int cc_build_plan(const sbi_amd_ccnn_config* cfg, CcPlan* out) {
  const int rc = cc_plan_sizes(cfg, out);
  if (rc) return rc;
  for (int ts = CC_MAX_TILE; ts >= 16; ts -= 16) {
    cc_layout(out, ts, false);
    if (cc_fits(*out)) {
      if (ts < out->R) return SBI_AMD_E_LDS;
      cc_layout(out, ts, true);
      return 0;
    }
  }
  return SBI_AMD_E_LDS;
}

static int cc_check_batch(const CcPlan& p, int64_t B) {
  if (B < 1) return SBI_AMD_E_BADARG;
  if (B * (int64_t)p.C0 * p.T >= (1ll << 31)) return SBI_AMD_E_UNSUPPORTED;
  return 0;
}

struct CcArgs {
  const float* params;     // the flat image
  const float* x;          // (B, C0, T)
  float* pooled;           // (B, C_L, Tp) (forward)
  const float* gpool;      // (B, C_L, Tp) (backward)
  float* partial;          // (G, P) (backward)
  long long units;         // B x nseg
};

// the weights, rows at an odd stride, and the biases
__device__ __forceinline__ void cc_stage(const CcPlan& pl, float* lds, const float* params, int tid) {
  for (int l = 0; l < pl.L; ++l) {
    const int CK = pl.CK[l], n = pl.C[l + 1] * CK;
    for (int e = tid; e < n; e += blockDim.x) {
      const int co = e / CK;
      lds[pl.o_w[l] + co * pl.ws[l] + (e - co * CK)] = params[pl.p_w[l] + e];
    }
    for (int e = tid; e < pl.C[l + 1]; e += blockDim.x) lds[pl.o_b[l] + e] = params[pl.p_b[l] + e];
  }
}

// map 0 of the tile [a, a + n): x on [a - R, a + n), zero left of t = 0.  a + n <= Tp pool <= T.
__device__ __forceinline__ void cc_load_x(const CcPlan& pl, float* dst, const float* xb, int a, int n, int tid) {
  const int n0 = n + pl.R;
  for (int e = tid; e < pl.C0 * n0; e += blockDim.x) {
    const int ci = e / n0, i = e - ci * n0, t = a - pl.R + i;
    dst[ci * pl.ms[0] + i] = t >= 0 ? xb[(long long)ci * pl.T + t] : 0.f;
  }
}

// out[co os + m] = leaky(bias[co] + sum_{ci, j} in[ci is + m + j d] w[co ws + ci k + j]) for m < n, 0 where t0 + m < 0
__device__ __forceinline__ void cc_layer(const float* in, int is, const float* w, int ws, const float* bias, float* out,
                                         int os, int Cin, int Cout, int k, int d, int n, int t0, float slope,
                                         int wave, int nwaves) {
  const int lane = threadIdx.x & 63;
  const int c = lane & 15, q = lane >> 4;
  const int CK = Cin * k, Nt = (Cout + 15) >> 4, tiles = ((n + 15) >> 4) * Nt;
  const int j4 = 4 % k, step = (4 / k) * is + j4 * d, wrap = is - k * d;    // K index + 4 in (ci, j) and as an offset
  for (int tile = wave; tile < tiles; tile += nwaves) {
    const int m0 = (tile / Nt) << 4, n0 = (tile % Nt) << 4;
    const int m = m0 + c, co = n0 + c;
    const bool m_ok = m < n, n_ok = co < Cout;
    const float* pw = w + co * ws;
    int j = q % k, off = (q / k) * is + j * d + m;    // in[ci is + j d + m] of K index k0 + q = ci k + j
    cc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < CK; k0 += 4) {
      const int kk = k0 + q;
      const bool k_ok = kk < CK;
      const float av = (m_ok && k_ok) ? in[off] : 0.f;
      const float bv = (n_ok && k_ok) ? pw[kk] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      j += j4; off += step;
      if (j >= k) { j -= k; off += wrap; }
    }
    if (n_ok) {
      const float b = bias[co];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mm = m0 + 4 * q + i;
        if (mm < n) {
          float v = acc[i] + b;
          v = v > 0.f ? v : slope * v;
          out[co * os + mm] = t0 + mm < 0 ? 0.f : v;
        }
      }
    }
  }
}

// acc[co (CK + 1) + nn] += sum_{m < n1} G[co gs + m] (nn < CK ? in[ci is + m + j d] : 1), nn = ci k + j.  The sum over
// time is cut into MFMA chains of CC_CHUNK steps whose results are added with a compensated (Kahan) sum, so the
// rounding error does not grow with the tile length.
__device__ __forceinline__ void cc_wgrad(const float* G, int gs, const float* in, int is, float* accum, int Cin,
                                         int Cout, int k, int d, int n1, int wave, int nwaves) {
  const int lane = threadIdx.x & 63;
  const int c = lane & 15, q = lane >> 4;
  const int CK = Cin * k, N = CK + 1, Nt = (N + 15) >> 4, tiles = ((Cout + 15) >> 4) * Nt;
  for (int tile = wave; tile < tiles; tile += nwaves) {
    const int m0 = (tile / Nt) << 4, n0 = (tile % Nt) << 4;
    const int co = m0 + c, nn = n0 + c;
    const bool m_ok = co < Cout, n_ok = nn < N, ones = nn == CK;
    const int ci = nn / k, j = nn - ci * k;
    const float* pa = G + co * gs;
    const float* pb = in + ci * is + j * d;
    cc_f4 acc = {0.f, 0.f, 0.f, 0.f}, lost = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < n1; c0 += CC_CHUNK) {
      cc_f4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t0 = 0; t0 < CC_CHUNK; t0 += 4) {
        const int t = c0 + t0 + q;
        const bool t_ok = t < n1;
        const float av = (m_ok && t_ok) ? pa[t] : 0.f;
        const float bv = (n_ok && t_ok) ? (ones ? 1.f : pb[t]) : 0.f;
        part = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, part, 0, 0, 0);
      }
      const cc_f4 y = part - lost, sum = acc + y;
      lost = (sum - acc) - y;
      acc = sum;
    }
    if (n_ok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = m0 + 4 * q + i;
        if (row < Cout) accum[row * N + nn] += acc[i];
      }
    }
  }
}

// Gout[ci os + i] = leaky'(A[ci os + i]) sum_{co, j} w[co ws + ci k + j] Gin[co gs + i - j d] (0 <= i - j d < n1) for
// i < n0, 0 where t0 + i < 0.  A is map l (the layer's input, an activation output), with Gout's stride.
__device__ __forceinline__ void cc_dgrad(const float* Gin, int gs, const float* w, int ws, const float* A, float* Gout,
                                         int os, int Cin, int Cout, int k, int d, int n0, int n1, int t0, float slope,
                                         int wave, int nwaves) {
  const int lane = threadIdx.x & 63;
  const int c = lane & 15, q = lane >> 4;
  const int K = Cout * k, Nt = (Cin + 15) >> 4, tiles = ((n0 + 15) >> 4) * Nt;
  const int j4 = 4 % k, c4 = 4 / k;
  for (int tile = wave; tile < tiles; tile += nwaves) {
    const int m0 = (tile / Nt) << 4, c0 = (tile % Nt) << 4;
    const int m = m0 + c, ci = c0 + c;
    const bool m_ok = m < n0, n_ok = ci < Cin;
    int co = q / k, j = q - co * k;
    cc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const bool k_ok = k0 + q < K;
      const int src = m - j * d;
      const float av = (m_ok && k_ok && src >= 0 && src < n1) ? Gin[co * gs + src] : 0.f;
      const float bv = (n_ok && k_ok) ? w[co * ws + ci * k + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      j += j4; co += c4;
      if (j >= k) { j -= k; ++co; }
    }
    if (n_ok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mm = m0 + 4 * q + i;
        if (mm < n0) {
          const float v = A[ci * os + mm] > 0.f ? acc[i] : slope * acc[i];
          Gout[ci * os + mm] = t0 + mm < 0 ? 0.f : v;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(CC_THREADS) cc_forward_kernel(CcPlan pl, CcArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int L = pl.L, CL = pl.C[L];
  cc_stage(pl, lds, a.params, tid);
  float* sums = lds + pl.o_pool;
  __syncthreads();
  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const long long b = unit / pl.nseg;
    const int seg = (int)(unit - b * pl.nseg);
    const int w0 = seg * pl.segw, w1 = min(pl.Tp, w0 + pl.segw), nw = w1 - w0;
    const float* xb = a.x + b * pl.C0 * pl.T;
    for (int e = tid; e < CL * nw; e += blockDim.x) sums[e] = 0.f;
    for (int ta = w0 * pl.pool; ta < w1 * pl.pool; ta += pl.TS) {
      const int n = min(pl.TS, w1 * pl.pool - ta);
      cc_load_x(pl, lds + pl.o_fbuf[0], xb, ta, n, tid);
      __syncthreads();
      for (int l = 0; l < L; ++l) {
        cc_layer(lds + pl.o_fbuf[l & 1], pl.ms[l], lds + pl.o_w[l], pl.ws[l], lds + pl.o_b[l],
                 lds + pl.o_fbuf[(l + 1) & 1], pl.ms[l + 1], pl.C[l], pl.C[l + 1], pl.k, pl.d[l], n + pl.H[l + 1],
                 ta - pl.H[l + 1], pl.slope, tid >> 6, CC_THREADS / 64);
        __syncthreads();
      }
      const float* top = lds + pl.o_fbuf[L & 1];
      for (int e = tid; e < CL * nw; e += blockDim.x) {
        const int c = e / nw, w = e - c * nw;
        const int lo = max(ta, (w0 + w) * pl.pool), hi = min(ta + n, (w0 + w + 1) * pl.pool);
        if (lo < hi) {
          float acc = sums[e];
          const float* row = top + c * pl.ms[L] - ta;
          for (int t = lo; t < hi; ++t) acc += row[t];
          sums[e] = acc;
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < CL * nw; e += blockDim.x) {
      const int c = e / nw, w = e - c * nw;
      a.pooled[(b * CL + c) * pl.Tp + w0 + w] = sums[e] * pl.inv_pool;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(CC_BWD_THREADS) cc_backward_kernel(CcPlan pl, CcArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, wave = tid >> 6;
  constexpr int BW = CC_BWD_THREADS / 64;
  const int L = pl.L, CL = pl.C[L];
  cc_stage(pl, lds, a.params, tid);
  for (int e = pl.o_g[0] + tid; e < pl.o_map[0]; e += blockDim.x) lds[e] = 0.f;     // the accumulators are contiguous
  __syncthreads();
  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const long long b = unit / pl.nseg;
    const int seg = (int)(unit - b * pl.nseg);
    const int w0 = seg * pl.segw, w1 = min(pl.Tp, w0 + pl.segw);
    const float* xb = a.x + b * pl.C0 * pl.T;
    const float* gp = a.gpool + b * CL * pl.Tp;
    for (int ta = w0 * pl.pool; ta < w1 * pl.pool; ta += pl.TS) {
      const int n = min(pl.TS, w1 * pl.pool - ta);
      cc_load_x(pl, lds + pl.o_map[0], xb, ta, n, tid);
      __syncthreads();
      for (int l = 0; l < L; ++l) {
        cc_layer(lds + pl.o_map[l], pl.ms[l], lds + pl.o_w[l], pl.ws[l], lds + pl.o_b[l], lds + pl.o_map[l + 1],
                 pl.ms[l + 1], pl.C[l], pl.C[l + 1], pl.k, pl.d[l], n + pl.H[l + 1], ta - pl.H[l + 1], pl.slope, wave,
                 BW);
        __syncthreads();
      }
      {
        // the seed: grad_pooled / pool through the last activation, on [a, b) only
        const float* top = lds + pl.o_map[L];
        float* g = lds + pl.o_gbuf[L & 1];
        for (int e = tid; e < CL * n; e += blockDim.x) {
          const int c = e / n, m = e - c * n;
          const float s = gp[(long long)c * pl.Tp + (ta + m) / pl.pool] * pl.inv_pool;
          g[c * pl.ms[L] + m] = top[c * pl.ms[L] + m] > 0.f ? s : pl.slope * s;
        }
      }
      __syncthreads();
      for (int l = L - 1; l >= 0; --l) {
        const float* g = lds + pl.o_gbuf[(l + 1) & 1];
        // the two are independent: the first ww waves take the weight gradient, the others the data gradient
        const int n0 = n + pl.H[l], n1 = n + pl.H[l + 1];
        int ww = BW;
        if (l > 0) {
          const int wt = ((pl.C[l + 1] + 15) >> 4) * ((pl.CK[l] + 16) >> 4);
          // MFMAs of either, up to the same factor
          const long long cw = (long long)wt * n1;
          const long long cd = (long long)((n0 + 15) >> 4) * ((pl.C[l] + 15) >> 4) * pl.C[l + 1] * pl.k;
          ww = (int)((BW * cw + (cw + cd) / 2) / (cw + cd));
          ww = min(max(ww, 1), min(wt, BW - 1));
        }
        if (wave < ww)
          cc_wgrad(g, pl.ms[l + 1], lds + pl.o_map[l], pl.ms[l], lds + pl.o_g[l], pl.C[l], pl.C[l + 1], pl.k, pl.d[l],
                   n1, wave, ww);
        else
          cc_dgrad(g, pl.ms[l + 1], lds + pl.o_w[l], pl.ws[l], lds + pl.o_map[l], lds + pl.o_gbuf[l & 1], pl.ms[l],
                   pl.C[l], pl.C[l + 1], pl.k, pl.d[l], n0, n1, ta - pl.H[l], pl.slope, wave - ww, BW - ww);
        __syncthreads();
      }
    }
  }
  float* mine = a.partial + (long long)blockIdx.x * pl.P;
  for (int l = 0; l < L; ++l) {
    const int N = pl.CK[l] + 1;
    for (int e = tid; e < pl.C[l + 1] * N; e += blockDim.x) {
      const int co = e / N, r = e - co * N;
      mine[r < pl.CK[l] ? pl.p_w[l] + co * pl.CK[l] + r : pl.p_b[l] + co] = lds[pl.o_g[l] + e];
    }
  }
}

// grad[i] = sum over workgroups, in workgroup order
__global__ void __launch_bounds__(256)
cc_reduce_kernel(const float* __restrict__ partial, int groups, int P, float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float acc = 0.f, lost = 0.f;              // compensated: the error does not grow with the number of workgroups
  for (int g = 0; g < groups; ++g) {
    const float y = partial[(long long)g * P + i] - lost, sum = acc + y;
    lost = (sum - acc) - y;
    acc = sum;
  }
  grad[i] = acc;
}

}  // namespace
