// sc_embed_kernel.h -- SpectralConvEmbedding on gfx950: plan, device functions, kernels (launchers: sc_embed.hip).
// Contract: include/sbi_amd_sc.h.
//
// Execution model
//   * a workgroup is 8 waves and owns whole samples b, b + G, ...; everything a sample needs lives in LDS: the twiddles,
//     its maps (point-major, map[n Cs + c] with Cs = C | 1), three small spectra (2 Mp x C: rows k < Mp the real /
//     cosine part of mode k, rows Mp + k the imaginary / sine part, Mp = modes rounded up to 4 so that a K walk of 4
//     never crosses from one part into the other) and the partial sums of the split chains.
//   * two MFMA routines (v_mfma_f32_16x16x4_f32; lane l gives A[m = l % 16][k = l / 16] and B[k = l / 16][n = l % 16]
//     and holds D[4 (l / 16) + i][l % 16]); every operand goes through a guarded loader, so an element outside the
//     matrix is an exact 0 and never a stale (possibly non-finite) value:
//       sc_point_sums   sums over the points: twiddle rows x map (the forward transform, M = 2 Mp, N = C, K = points)
//                       and map^T x map (a pointwise weight gradient with a column of ones for the bias).  The point
//                       range is cut into pl.parts contiguous ranges, one chain per (tile, range); the partial tiles go
//                       to LDS and are added in ascending order by one thread per element.
//       sc_point_gemm   one value per (point, channel): M = points, N = C, K = 2 Mp + C: cos rows, sin rows, then the
//                       pointwise convolution, one chain; bias and GELU from the accumulators.
//   * the per-mode complex channel mix, its backward, fc0, fc_last and GELU are VALU loops over LDS; the spectral
//     weights come through L2 (each is used once per sample and layer).
//   * backward: slot 0 holds h_0, slot l + 1 the pre-activation u_l; two scratch maps P / Q hold the running gradient
//     and the current layer's input h_l = gelu(u_{l-1}) and change roles after every layer.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_sc.h"

namespace {

#define SC_THREADS 512
#define SC_WAVES 8
#define SC_GROUPS 512               // most workgroups of a launch: samples beyond walk the grid again
#define SC_MAX_CHANNELS 32
#define SC_MAX_MODES 64
#define SC_MAX_LAYERS 8
#define SC_MAX_POINTS 65535
#define SC_LDS_BUDGET (160 * 1024)

typedef float sc_f4 __attribute__((ext_vector_type(4)));

struct ScPlan {
  int Cin, C, Cout, M, L, N, pos;
  int Mp, R2, Cs, tws, T1, T2, parts, plen, P;
  float inv_n;
  // offsets in the flat parameters
  int p_fc0w, p_fc0b, p_conv[SC_MAX_LAYERS], p_ww[SC_MAX_LAYERS], p_wb[SC_MAX_LAYERS], p_last, p_flw, p_flb;
  // LDS offsets (floats): forward, backward
  int msz;                                      // one map
  int f_buf[2], f_sa, f_sb, f_part, f_ww, f_wb;
  int b_slot, b_buf[2], b_sa, b_sb, b_sc, b_part, b_ww, b_wb, b_acc;
  int fwd_floats, bwd_floats;
};

// sizes and parameter offsets: do not depend on n_points
static int sc_plan_sizes(const sbi_amd_sc_config* cfg, ScPlan* out) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->in_channels < 1 || cfg->conv_channels < 1 || cfg->out_channels < 1 || cfg->modes < 1 ||
      cfg->num_layers < 1)
    return SBI_AMD_E_BADARG;
  if (cfg->in_channels > SC_MAX_CHANNELS || cfg->conv_channels > SC_MAX_CHANNELS ||
      cfg->out_channels > SC_MAX_CHANNELS || cfg->modes > SC_MAX_MODES || cfg->num_layers > SC_MAX_LAYERS)
    return SBI_AMD_E_UNSUPPORTED;
  ScPlan p = {};
  p.Cin = cfg->in_channels; p.C = cfg->conv_channels; p.Cout = cfg->out_channels; p.M = cfg->modes;
  p.L = cfg->num_layers;
  const int spectral = 2 * p.C * p.C * p.M;      // at most 2^17: 9 of them and the rest stay far below 2^31
  int off = 0;
  p.p_fc0w = off; off += p.C * p.Cin;
  p.p_fc0b = off; off += p.C;
  for (int l = 0; l < p.L; ++l) { p.p_conv[l] = off; off += spectral; }
  for (int l = 0; l < p.L; ++l) {
    p.p_ww[l] = off; off += p.C * p.C;
    p.p_wb[l] = off; off += p.C;
  }
  p.p_last = off; off += spectral;
  p.p_flw = off; off += p.Cout * p.C;
  p.p_flb = off; off += p.Cout;
  p.P = off;
  *out = p;
  return 0;
}

static int sc_r4(long long v) { return (int)((v + 3) & ~3ll); }

// the LDS images; SBI_AMD_E_LDS (with the plan filled in) when the backward image passes the budget
static int sc_build_plan(const sbi_amd_sc_config* cfg, ScPlan* out) {
  const int rc = sc_plan_sizes(cfg, out);
  if (rc) return rc;
  if (cfg->n_points < 1 || cfg->has_positions < 0 || cfg->has_positions > 1) return SBI_AMD_E_BADARG;
  if (cfg->n_points > SC_MAX_POINTS || cfg->modes > cfg->n_points / 2 + 1) return SBI_AMD_E_UNSUPPORTED;
  ScPlan& p = *out;
  p.N = cfg->n_points; p.pos = cfg->has_positions;
  p.inv_n = 1.f / (float)p.N;
  p.Mp = (p.M + 3) & ~3; p.R2 = 2 * p.Mp; p.Cs = p.C | 1; p.tws = p.N | 1;
  const int Ct = (p.C + 15) >> 4, big = p.C > p.Cin ? p.C : p.Cin;
  p.T1 = ((p.R2 + 15) >> 4) * Ct;
  p.T2 = Ct * ((big + 16) >> 4);
  p.parts = 8 / p.T1 > 1 ? 8 / p.T1 : 1;
  p.plen = 4 * ((p.N + 4 * p.parts - 1) / (4 * p.parts));
  p.msz = sc_r4((long long)p.N * p.Cs);
  const int tw = sc_r4(p.pos ? 2ll * p.M * p.tws : 2ll * p.N), spec = p.R2 * p.C;     // every offset a multiple of 4
  const int wsz = sc_r4(p.C * p.Cs), bsz = sc_r4(p.C);
  long long o = tw;
  p.f_buf[0] = (int)o; o += p.msz;
  p.f_buf[1] = (int)o; o += p.msz;
  p.f_sa = (int)o; o += spec;
  p.f_sb = (int)o; o += spec;
  p.f_part = (int)o; o += 256 * p.parts * p.T1;
  p.f_ww = (int)o; o += wsz;
  p.f_wb = (int)o; o += bsz;
  p.fwd_floats = (int)o;
  o = tw;
  p.b_slot = (int)o; o += (long long)(p.L + 1) * p.msz;
  p.b_buf[0] = (int)o; o += p.msz;
  p.b_buf[1] = (int)o; o += p.msz;
  p.b_sa = (int)o; o += spec;
  p.b_sb = (int)o; o += spec;
  p.b_sc = (int)o; o += spec;
  p.b_part = (int)o; o += 256 * p.parts * (2 * p.T1 + p.T2);
  p.b_ww = (int)o; o += wsz;
  p.b_wb = (int)o; o += bsz;
  p.b_acc = (int)o; o += p.P;
  p.bwd_floats = (int)o;                          // < 11 x 65535 x 33 + 2 x 64 x 65536 + 2^21: no overflow
  return (long long)p.bwd_floats * 4 > SC_LDS_BUDGET ? SBI_AMD_E_LDS : 0;
}

static int sc_check_batch(const ScPlan& p, int64_t B) {
  if (B < 1) return SBI_AMD_E_BADARG;
  if (B * (int64_t)p.Cin * p.N >= (1ll << 31)) return SBI_AMD_E_UNSUPPORTED;
  return 0;
}

struct ScArgs {
  const float* params;     // the flat image
  const float* x;          // x[b xbs + i xcs + n]
  const float* pos;        // pos[b pbs + n] or null
  long long xbs, xcs, pbs;
  float* out;              // (B, 2 M Cout) (forward)
  const float* gout;       // (B, 2 M Cout) (backward)
  float* partial;          // (G, P) (backward)
  long long B;
};

__device__ __forceinline__ float sc_gelu(float y) { return 0.5f * y * (1.f + erff(y * 0.70710678118654752440f)); }
__device__ __forceinline__ float sc_dgelu(float y) {
  return 0.5f * (1.f + erff(y * 0.70710678118654752440f)) + y * 0.39894228040143267794f * expf(-0.5f * y * y);
}

// ---- guarded operand loaders: get() is the lane's operand of the next MFMA of a chain (K advances by 4) ---------------
struct ScLd {
  const float* p;
  int step, left;          // `left` K indices remain from the lane's first one
  bool ok, one;            // !ok: outside M or N; one: a column of ones
  __device__ __forceinline__ float get() {
    const float v = (ok && left > 0) ? (one ? 1.f : *p) : 0.f;
    p += step; left -= 4;
    return v;
  }
};

struct ScTw {
  const float* p;          // positions: the element itself; equispaced: the cos or the sin table
  int step, idx, istep, N, left;
  bool eq, ok;
  __device__ __forceinline__ float get() {
    float v = 0.f;
    if (ok && left > 0) v = eq ? p[idx] : *p;
    if (eq) {
      idx += istep;
      if (idx >= N) idx -= N;
    } else {
      p += step;
    }
    left -= 4;
    return v;
  }
};

// cos (s = 0) or sin (s = 1) of theta[k, n], n = n0, n0 + 4, ... < n_end
__device__ __forceinline__ ScTw sc_tw_along_n(const ScPlan& pl, const float* tw, int s, int k, int n0, int n_end) {
  ScTw t;
  t.eq = !pl.pos; t.N = pl.N; t.left = n_end - n0; t.ok = k < pl.M;
  const int kk = t.ok ? k : 0;
  if (t.eq) {
    t.p = tw + s * pl.N; t.step = 0;
    t.idx = (int)(((long long)kk * n0) % pl.N); t.istep = (4 * kk) % pl.N;
  } else {
    t.p = tw + (s * pl.M + kk) * pl.tws + n0; t.step = 4; t.idx = 0; t.istep = 0;
  }
  return t;
}

// ... of theta[k, n], k = k0, k0 + 4, ... < M
__device__ __forceinline__ ScTw sc_tw_along_k(const ScPlan& pl, const float* tw, int s, int k0, int n) {
  ScTw t;
  t.eq = !pl.pos; t.N = pl.N; t.left = pl.M - k0; t.ok = n < pl.N;
  const int nn = t.ok ? n : 0;
  if (t.eq) {
    t.p = tw + s * pl.N; t.step = 0;
    t.idx = (int)(((long long)k0 * nn) % pl.N); t.istep = (4 * nn) % pl.N;
  } else {
    t.p = tw + (s * pl.M + k0) * pl.tws + nn; t.step = 4 * pl.tws; t.idx = 0; t.istep = 0;
  }
  return t;
}

// the twiddles of one sample; posb = its positions, or null
__device__ __forceinline__ void sc_build_tw(const ScPlan& pl, float* tw, const float* posb, int tid) {
  if (!pl.pos) {
    const float fn = (float)pl.N;
    for (int j = tid; j < pl.N; j += SC_THREADS) {
      // j / N = q + d with q = fl(j / N) and d the exact remainder / N: first order in d around q
      const float q = (float)j / fn, d = fmaf(-q, fn, (float)j) / fn, a = 6.28318530717958647692f * d;
      float s, c;
      sincospif(2.f * q, &s, &c);
      tw[j] = fmaf(-a, s, c);
      tw[pl.N + j] = fmaf(a, c, s);
    }
  } else {
    for (int e = tid; e < pl.M * pl.N; e += SC_THREADS) {
      const int k = e / pl.N, n = e - k * pl.N;
      const float kf = (float)k, t = posb[n];
      const float p = kf * t, err = fmaf(kf, t, -p), f = (p - rintf(p)) + err;
      float s, c;
      sincospif(2.f * f, &s, &c);
      tw[k * pl.tws + n] = c;
      tw[(pl.M + k) * pl.tws + n] = s;
    }
  }
}

// a pointwise weight gradient: accW[o Ck + j] += sum_n g[n Cs + o] h[n hks + j hcs], accB[o] += sum_n g[n Cs + o]
struct ScWg {
  const float* g;
  const float* h;
  int hks;
  long long hcs;
  int Ck;
  float* accW;
  float* accB;
};

// sums over the points.  srcA / srcB (maps, may be null): out[r C + c] = scale sum_n tw(r, n) src[n Cs + c] with the
// sine rows negated, i.e. (Re, Im) of sum_n exp(-i theta) src; rows of modes >= M are 0.  wg (may be null): see ScWg.
// Ends with a barrier.
__device__ __forceinline__ void sc_point_sums(const ScPlan& pl, const float* tw, const float* srcA, float* outA,
                                              float scaleA, const float* srcB, float* outB, float scaleB,
                                              const ScWg* wg, float* part, int tid) {
  const int wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
  const int Ct = (pl.C + 15) >> 4;
  const int nA = srcA ? pl.T1 : 0, nB = srcB ? pl.T1 : 0;
  const int WNt = wg ? (wg->Ck + 16) >> 4 : 0, nW = Ct * WNt;
  const int total = (nA + nB + nW) * pl.parts;
  for (int w = wave; w < total; w += SC_WAVES) {
    const int item = w / pl.parts, part_i = w - item * pl.parts;
    const int nb = part_i * pl.plen, ne = min(pl.N, nb + pl.plen), n = nb + q;
    sc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    if (item < nA + nB) {
      const float* src = item < nA ? srcA : srcB;
      const int t = item < nA ? item : item - nA;
      const int r = (t / Ct) * 16 + c, col = (t % Ct) * 16 + c;
      const int s = r >= pl.Mp ? 1 : 0;
      ScTw a = sc_tw_along_n(pl, tw, s, r - s * pl.Mp, n, ne);
      ScLd b = {src + n * pl.Cs + col, 4 * pl.Cs, ne - n, col < pl.C, false};
      for (int n0 = nb; n0 < ne; n0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.get(), b.get(), acc, 0, 0, 0);
    } else {
      const int t = item - nA - nB;
      const int o = (t / WNt) * 16 + c, j = (t % WNt) * 16 + c;
      ScLd a = {wg->g + n * pl.Cs + o, 4 * pl.Cs, ne - n, o < pl.C, false};
      ScLd b = {wg->h + (long long)n * wg->hks + (long long)j * wg->hcs, 4 * wg->hks, ne - n, j <= wg->Ck,
                j == wg->Ck};
      for (int n0 = nb; n0 < ne; n0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.get(), b.get(), acc, 0, 0, 0);
    }
    *reinterpret_cast<sc_f4*>(part + w * 256 + lane * 4) = acc;
  }
  __syncthreads();
  for (int which = 0; which < 2; ++which) {
    float* out = which ? outB : outA;
    if (!(which ? srcB : srcA)) continue;
    const float scale = which ? scaleB : scaleA;
    const int ib = which ? nA : 0;
    for (int e = tid; e < pl.R2 * pl.C; e += SC_THREADS) {
      const int r = e / pl.C, col = e - r * pl.C;
      const int t = ib + (r >> 4) * Ct + (col >> 4), ln = ((r & 15) >> 2) * 16 + (col & 15), i = r & 3;
      const float* pp = part + t * pl.parts * 256 + ln * 4 + i;
      float sum = 0.f;
      for (int p = 0; p < pl.parts; ++p) sum += pp[p * 256];
      const int s = r >= pl.Mp ? 1 : 0;
      out[e] = (r - s * pl.Mp) < pl.M ? (s ? -sum : sum) * scale : 0.f;
    }
  }
  if (wg) {
    const int Nc = wg->Ck + 1;
    for (int e = tid; e < pl.C * Nc; e += SC_THREADS) {
      const int o = e / Nc, j = e - o * Nc;
      const int t = nA + nB + (o >> 4) * WNt + (j >> 4), ln = ((o & 15) >> 2) * 16 + (j & 15), i = o & 3;
      const float* pp = part + t * pl.parts * 256 + ln * 4 + i;
      float sum = 0.f;
      for (int p = 0; p < pl.parts; ++p) sum += pp[p * 256];
      if (j < wg->Ck) wg->accW[o * wg->Ck + j] += sum;
      else wg->accB[o] += sum;
    }
  }
  __syncthreads();
}

// v[n, col] = sum_k cos(theta[k, n]) S[k C + col] + sin(theta[k, n]) S[(Mp + k) C + col]
//           + sum_{j < Kp} pA[n Cs + j] wB[col wcs + j wks] + bias[col]            for n < N, col < C
// dst_u[n Cs + col] = v and dst_h[n Cs + col] = gelu(v) (each may be null; pA and bias too).  No barrier.
__device__ __forceinline__ void sc_point_gemm(const ScPlan& pl, const float* tw, const float* S, const float* pA,
                                              int Kp, const float* wB, int wcs, int wks, const float* bias,
                                              float* dst_u, float* dst_h, int tid) {
  const int wave = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
  const int Ct = (pl.C + 15) >> 4, tiles = ((pl.N + 15) >> 4) * Ct;
  for (int tile = wave; tile < tiles; tile += SC_WAVES) {
    const int m0 = (tile / Ct) << 4, c0 = (tile % Ct) << 4;
    const int n = m0 + c, col = c0 + c;
    sc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < 2; ++s) {
      ScTw a = sc_tw_along_k(pl, tw, s, q, n);
      ScLd b = {S + (s * pl.Mp + q) * pl.C + col, 4 * pl.C, pl.M - q, col < pl.C, false};
      for (int k0 = 0; k0 < pl.Mp; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.get(), b.get(), acc, 0, 0, 0);
    }
    if (pA) {
      ScLd a = {pA + n * pl.Cs + q, 4, Kp - q, n < pl.N, false};
      ScLd b = {wB + col * wcs + q * wks, 4 * wks, Kp - q, col < pl.C, false};
      for (int k0 = 0; k0 < Kp; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.get(), b.get(), acc, 0, 0, 0);
    }
    if (col < pl.C) {
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int nn = m0 + 4 * q + i;
        if (nn < pl.N) {
          const float v = acc[i] + bv;
          if (dst_u) dst_u[nn * pl.Cs + col] = v;
          if (dst_h) dst_h[nn * pl.Cs + col] = sc_gelu(v);
        }
      }
    }
  }
}

// Y[k C + o] = Re, Y[(Mp + k) C + o] = sign Im of sum_i X[k, i] W[i, o, k];  X = (Re rows, Im rows).  No barrier.
__device__ __forceinline__ void sc_mix(const ScPlan& pl, const float* W, const float* X, float* Y, float sign,
                                       int tid) {
  for (int e = tid; e < pl.M * pl.C; e += SC_THREADS) {
    const int o = e / pl.M, k = e - o * pl.M;
    float re = 0.f, im = 0.f;
    for (int i = 0; i < pl.C; ++i) {
      const float* w = W + 2 * ((i * pl.C + o) * pl.M + k);
      const float wr = w[0], wi = w[1], xr = X[k * pl.C + i], xi = X[(pl.Mp + k) * pl.C + i];
      re = fmaf(xr, wr, re); re = fmaf(-xi, wi, re);
      im = fmaf(xr, wi, im); im = fmaf(xi, wr, im);
    }
    Y[k * pl.C + o] = re;
    Y[(pl.Mp + k) * pl.C + o] = sign * im;
  }
}

// backward of the mix, G = dL/dRe + i dL/dIm of Yhat: acc[i, o, k] += conj(X[k, i]) G[k, o], and
// Bx = (Re, -Im) of sum_o conj(W[i, o, k]) G[k, o] / N, the operand of the inverse transform that gives d h.  No barrier.
__device__ __forceinline__ void sc_mix_backward(const ScPlan& pl, const float* W, float* acc, const float* X,
                                                const float* G, float* Bx, int tid) {
  const int CC = pl.C * pl.C;
  for (int e = tid; e < CC * pl.M; e += SC_THREADS) {
    const int io = e / pl.M, k = e - io * pl.M, i = io / pl.C, o = io - i * pl.C;
    const float xr = X[k * pl.C + i], xi = X[(pl.Mp + k) * pl.C + i];
    const float gr = G[k * pl.C + o], gi = G[(pl.Mp + k) * pl.C + o];
    acc[2 * e] += fmaf(xr, gr, xi * gi);
    acc[2 * e + 1] += fmaf(xr, gi, -(xi * gr));
  }
  for (int e = tid; e < pl.M * pl.C; e += SC_THREADS) {
    const int i = e / pl.M, k = e - i * pl.M;
    float re = 0.f, im = 0.f;
    for (int o = 0; o < pl.C; ++o) {
      const float* w = W + 2 * ((i * pl.C + o) * pl.M + k);
      const float wr = w[0], wi = w[1], gr = G[k * pl.C + o], gi = G[(pl.Mp + k) * pl.C + o];
      re = fmaf(wr, gr, re); re = fmaf(wi, gi, re);
      im = fmaf(wr, gi, im); im = fmaf(-wi, gr, im);
    }
    Bx[k * pl.C + i] = re * pl.inv_n;
    Bx[(pl.Mp + k) * pl.C + i] = -im * pl.inv_n;
  }
}

// one pointwise layer's weights, rows at an odd stride, and its bias
__device__ __forceinline__ void sc_stage(const ScPlan& pl, const float* params, int l, float* ww, float* wb, int tid) {
  for (int e = tid; e < pl.C * pl.C; e += SC_THREADS) {
    const int o = e / pl.C;
    ww[o * pl.Cs + (e - o * pl.C)] = params[pl.p_ww[l] + e];
  }
  for (int e = tid; e < pl.C; e += SC_THREADS) wb[e] = params[pl.p_wb[l] + e];
}

// twiddles, h_0 into `first`, then the layers: layer l reads (l ? buf[l & 1] : first), writes h_{l+1} to
// buf[(l + 1) & 1] and, with slots, u_l to slots + (l + 1) msz; then Xhat of h_L in sa and Yhat_last = (Re, Im) in sb.
// Ends with a barrier.
__device__ __forceinline__ void sc_forward_sample(const ScPlan& pl, const ScArgs& a, long long b, float* tw,
                                                  float* first, float* buf0, float* buf1, float* slots, float* sa,
                                                  float* sb, float* part, float* ww, float* wb, int tid) {
  const float* xb = a.x + b * a.xbs;
  sc_build_tw(pl, tw, a.pos ? a.pos + b * a.pbs : nullptr, tid);
  for (int e = tid; e < pl.N * pl.C; e += SC_THREADS) {
    const int cc = e / pl.N, n = e - cc * pl.N;          // consecutive threads read consecutive points of x
    const float* w0 = a.params + pl.p_fc0w + cc * pl.Cin;
    float v = 0.f;
    for (int i = 0; i < pl.Cin; ++i) v = fmaf(w0[i], xb[i * a.xcs + n], v);
    first[n * pl.Cs + cc] = v + a.params[pl.p_fc0b + cc];
  }
  sc_stage(pl, a.params, 0, ww, wb, tid);
  __syncthreads();
  for (int l = 0; l < pl.L; ++l) {
    const float* in = l ? ((l & 1) ? buf1 : buf0) : first;
    float* outh = ((l + 1) & 1) ? buf1 : buf0;
    sc_point_sums(pl, tw, in, sa, pl.inv_n, nullptr, nullptr, 0.f, nullptr, part, tid);
    sc_mix(pl, a.params + pl.p_conv[l], sa, sb, -1.f, tid);
    __syncthreads();
    sc_point_gemm(pl, tw, sb, in, pl.C, ww, pl.Cs, 1, wb, slots ? slots + (l + 1) * pl.msz : nullptr, outh, tid);
    __syncthreads();
    if (l + 1 < pl.L) sc_stage(pl, a.params, l + 1, ww, wb, tid);      // visible after the barrier in sc_point_sums
  }
  const float* top = (pl.L & 1) ? buf1 : buf0;
  sc_point_sums(pl, tw, top, sa, pl.inv_n, nullptr, nullptr, 0.f, nullptr, part, tid);
  sc_mix(pl, a.params + pl.p_last, sa, sb, 1.f, tid);
  __syncthreads();
}

__global__ void __launch_bounds__(SC_THREADS) sc_forward_kernel(ScPlan pl, ScArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int rows = 2 * pl.M * pl.Cout;
  for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
    sc_forward_sample(pl, a, b, lds, lds + pl.f_buf[0], lds + pl.f_buf[0], lds + pl.f_buf[1], nullptr, lds + pl.f_sa,
                      lds + pl.f_sb, lds + pl.f_part, lds + pl.f_ww, lds + pl.f_wb, tid);
    const float* Z = lds + pl.f_sb;
    for (int e = tid; e < rows; e += SC_THREADS) {
      const int row = e / pl.Cout, oo = e - row * pl.Cout, k = row >> 1, r = row & 1;
      const float* wl = a.params + pl.p_flw + oo * pl.C;
      const float* z = Z + (r * pl.Mp + k) * pl.C;
      float v = 0.f;
      for (int cc = 0; cc < pl.C; ++cc) v = fmaf(wl[cc], z[cc], v);
      a.out[b * rows + e] = v + a.params[pl.p_flb + oo];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(SC_THREADS) sc_backward_kernel(ScPlan pl, ScArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int rows = 2 * pl.M * pl.Cout, L = pl.L, C = pl.C;
  float* tw = lds;
  float* slots = lds + pl.b_slot;
  float* sa = lds + pl.b_sa;
  float* sb = lds + pl.b_sb;
  float* sc = lds + pl.b_sc;
  float* part = lds + pl.b_part;
  float* ww = lds + pl.b_ww;
  float* wb = lds + pl.b_wb;
  float* acc = lds + pl.b_acc;
  for (int e = tid; e < pl.P; e += SC_THREADS) acc[e] = 0.f;
  __syncthreads();
  for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
    sc_forward_sample(pl, a, b, tw, slots, lds + pl.b_buf[0], lds + pl.b_buf[1], slots, sa, sb, part, ww, wb, tid);
    float* Q = lds + pl.b_buf[L & 1];               // h_L
    float* Pg = lds + pl.b_buf[(L + 1) & 1];        // free: receives d h_L
    const float* go = a.gout + b * rows;
    // fc_last: its gradients from Z = sb, and G = d Yhat_last into sc
    for (int e = tid; e < pl.Cout * (C + 1); e += SC_THREADS) {
      const int oo = e / (C + 1), cc = e - oo * (C + 1);
      float sum = 0.f;
      for (int row = 0; row < 2 * pl.M; ++row) {
        const float z = cc < C ? sb[((row & 1) * pl.Mp + (row >> 1)) * C + cc] : 1.f;
        sum = fmaf(go[row * pl.Cout + oo], z, sum);
      }
      acc[cc < C ? pl.p_flw + oo * C + cc : pl.p_flb + oo] += sum;
    }
    for (int e = tid; e < 2 * pl.M * C; e += SC_THREADS) {
      const int row = e / C, cc = e - row * C;
      float sum = 0.f;
      for (int oo = 0; oo < pl.Cout; ++oo) sum = fmaf(go[row * pl.Cout + oo], a.params[pl.p_flw + oo * C + cc], sum);
      sc[((row & 1) * pl.Mp + (row >> 1)) * C + cc] = sum;
    }
    __syncthreads();
    sc_mix_backward(pl, a.params + pl.p_last, acc + pl.p_last, sa, sc, sb, tid);
    __syncthreads();
    sc_point_gemm(pl, tw, sb, nullptr, 0, nullptr, 0, 0, nullptr, Pg, nullptr, tid);
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
      const float* u = slots + (l + 1) * pl.msz;
      const float* prev = slots + l * pl.msz;        // h_0 (l = 0) or u_{l-1}
      for (int e = tid; e < pl.N * C; e += SC_THREADS) {
        const int n = e / C, idx = n * pl.Cs + (e - n * C);
        Pg[idx] *= sc_dgelu(u[idx]);
        if (l) Q[idx] = sc_gelu(prev[idx]);
      }
      sc_stage(pl, a.params, l, ww, wb, tid);
      __syncthreads();
      const float* in = l ? Q : prev;
      const ScWg wg = {Pg, in, pl.Cs, 1, C, acc + pl.p_ww[l], acc + pl.p_wb[l]};
      sc_point_sums(pl, tw, in, sa, pl.inv_n, Pg, sc, 1.f, &wg, part, tid);
      sc_mix_backward(pl, a.params + pl.p_conv[l], acc + pl.p_conv[l], sa, sc, sb, tid);
      __syncthreads();
      // d h_l = (pointwise)^T of the gradient + the inverse transform of d Xhat / N; the layer's input is spent
      sc_point_gemm(pl, tw, sb, Pg, C, ww, 1, pl.Cs, nullptr, Q, nullptr, tid);
      __syncthreads();
      float* t = Pg; Pg = Q; Q = t;
    }
    const ScWg wg = {Pg, a.x + b * a.xbs, 1, a.xcs, pl.Cin, acc + pl.p_fc0w, acc + pl.p_fc0b};
    sc_point_sums(pl, tw, nullptr, nullptr, 0.f, nullptr, nullptr, 0.f, &wg, part, tid);
  }
  float* mine = a.partial + (long long)blockIdx.x * pl.P;
  for (int e = tid; e < pl.P; e += SC_THREADS) mine[e] = acc[e];
}

// grad[i] = sum over workgroups, in workgroup order
__global__ void __launch_bounds__(256)
sc_reduce_kernel(const float* __restrict__ partial, int groups, int P, float* __restrict__ grad) {
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
