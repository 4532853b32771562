// tr_embed_kernel.h -- kernels of TransformerEmbedding (include/sbi_amd_tr.h): plan, tile helpers, forward, backward.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_tr.h"
#include "philox.h"

#define TR_THREADS 256
#define TR_WAVES 4
#define TR_TOK SBI_AMD_TR_TOK
#define TR_LDS_LIMIT (160 * 1024)

struct TrPlan {
  int F, H, KV, hd, I, L, E, OP, pos, act, causal, scalar, group;
  float eps, scale;
  float div[32];
  // offsets into the flat parameter image
  int64_t p_spw, p_spb, p_layer0, PL, p_norm, p_aggw, p_aggb, P;
  // inside one block's PL parameters
  int o_ow, o_qkv, o_gu, o_down, o_ln1, o_ln2;
  int PS;      // one workgroup's partial image: a block's parameters and the scalar projection
  int lds[6];  // floats: qkv, attention, tail, tail backward, attention backward, qkv backward
};

struct TrShape {
  int64_t B, T, N, Q, K, S, LS;
  int64_t tiles, per, G;
};

static inline int tr_plan_sizes(const sbi_amd_tr_config* c, TrPlan* pl) {
  if (!c) return SBI_AMD_E_BADARG;
  const int F = c->feature_space_dim, H = c->num_attention_heads, KV = c->num_key_value_heads, hd = c->head_dim;
  const int I = c->intermediate_size, L = c->num_hidden_layers, E = c->final_emb_dimension;
  if (F < 1 || H < 1 || KV < 1 || hd < 1 || I < 1 || L < 1 || E < 1) return SBI_AMD_E_BADARG;
  if (F > 128 || hd < 2 || hd > 64 || (hd & 1) || (int64_t)H * hd != F || H % KV != 0 || I > 512 || L > 8 || E > 128)
    return SBI_AMD_E_UNSUPPORTED;
  if (c->pos_emb < 0 || c->pos_emb > 2 || c->activation < 0 || c->activation > 1 || c->is_causal < 0 ||
      c->is_causal > 1 || c->scalar_input < 0 || c->scalar_input > 1)
    return SBI_AMD_E_UNSUPPORTED;
  pl->F = F; pl->H = H; pl->KV = KV; pl->hd = hd; pl->I = I; pl->L = L; pl->E = E;
  pl->OP = (H + 2 * KV) * hd;
  pl->pos = c->pos_emb; pl->act = c->activation; pl->causal = c->is_causal; pl->scalar = c->scalar_input;
  pl->group = H / KV;
  pl->eps = c->rms_norm_eps;
  pl->scale = (float)(1.0 / sqrt((double)hd));
  for (int i = 0; i < 32; ++i) pl->div[i] = i < hd / 2 ? c->div_term[i] : 1.0f;
  pl->o_ow = 0;
  pl->o_qkv = F * F;
  pl->o_gu = pl->o_qkv + pl->OP * F;
  pl->o_down = pl->o_gu + 2 * I * F;
  pl->o_ln1 = pl->o_down + F * I;
  pl->o_ln2 = pl->o_ln1 + F;
  pl->PL = pl->o_ln2 + F;
  pl->PS = (int)pl->PL + 2 * F;
  pl->p_spw = 0;
  pl->p_spb = F;
  pl->p_layer0 = 2 * F;
  pl->p_norm = pl->p_layer0 + (int64_t)L * pl->PL;
  pl->p_aggw = pl->p_norm + F;
  pl->p_aggb = pl->p_aggw + (int64_t)E * F;
  pl->P = pl->p_aggb + E;
  return 0;
}

static inline int tr_build_plan(const sbi_amd_tr_config* c, int64_t B, int64_t T, TrPlan* pl, TrShape* sh) {
  const int rc = tr_plan_sizes(c, pl);
  if (rc) return rc;
  if (B < 1 || T < 1) return SBI_AMD_E_BADARG;
  if (T > 4096) return SBI_AMD_E_UNSUPPORTED;
  const int64_t wide = pl->F > 2 * pl->I ? pl->F : 2 * pl->I;
  if (B > (((int64_t)1 << 31) - 1) / T || B * T > (((int64_t)1 << 31) - 1) / wide) return SBI_AMD_E_UNSUPPORTED;
  const int F = pl->F, I = pl->I, OP = pl->OP, hd = pl->hd;
  pl->lds[0] = TR_TOK * (F + OP) + TR_TOK;
  pl->lds[1] = TR_WAVES * ((int)T + hd);
  pl->lds[2] = TR_TOK * (3 * F + 2 * I) + TR_TOK;
  pl->lds[3] = TR_TOK * (5 * F + 3 * I) + 2 * TR_TOK;
  pl->lds[4] = TR_WAVES * (2 * (int)T + 2 * hd);
  pl->lds[5] = TR_TOK * (4 * F + OP) + 2 * TR_TOK;
  sh->B = B; sh->T = T; sh->N = B * T;
  sh->Q = sh->N * F;
  sh->K = sh->N * pl->KV * hd;
  sh->S = B * pl->H * T;
  sh->LS = 4 * sh->Q + 2 * sh->K + sh->S;
  sh->tiles = (sh->N + TR_TOK - 1) / TR_TOK;
  sh->per = (sh->tiles + SBI_AMD_TR_MAX_PARTIALS - 1) / SBI_AMD_TR_MAX_PARTIALS;
  sh->G = (sh->tiles + sh->per - 1) / sh->per;
  for (int i = 0; i < 6; ++i)
    if (pl->lds[i] * 4 > TR_LDS_LIMIT) return SBI_AMD_E_LDS;
  return 0;
}

static inline int64_t tr_workspace_floats(const TrPlan& pl, const TrShape& sh, int training) {
  if (!training) return sh.LS;
  return pl.L * sh.LS + sh.Q + 3 * sh.Q + 2 * sh.K + sh.S + 2 * sh.B * pl.F + sh.G * (int64_t)pl.PS;
}

struct TrArgs {
  const float* params;
  const float* x;
  int64_t xbs, xts;
  int64_t B, T, N;
  float p, inv_keep;
  unsigned seed_lo, seed_hi;
  int layer, training;
  // one block's buffers
  float *h_in, *q, *k, *v, *attn, *lse, *h1, *h_out;
  // backward
  float *dh, *dO, *dq, *dk, *dv, *D, *ybuf, *cbuf, *partial;
  const float* gout;
  float* out;
  float* grad;
  int64_t per;   // tiles per workgroup in the backward tile kernels
};

// ---- dropout ----------------------------------------------------------------------------------------------------------
// keep decision of (layer, b, head, q, k): independent of B and T
__device__ __forceinline__ bool tr_keep(unsigned seed_lo, unsigned seed_hi, int lh, int b, int q, int k, float p) {
  unsigned r[4];
  philox4x32_10((unsigned)(k >> 2), (unsigned)q, (unsigned)b, (unsigned)lh, seed_lo, seed_hi, r);
  return u01(r[k & 3]) >= p;
}

// ---- small helpers ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tr_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float tr_wave_sum(float v) {      // a fixed tree: the same bits on every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float tr_act(float g, int act) {
  return act ? fmaxf(g, 0.0f) : 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f));
}
__device__ __forceinline__ float tr_dact(float g, int act) {
  if (act) return g > 0.0f ? 1.0f : 0.0f;
  return 0.5f * (1.0f + erff(g * 0.70710678118654752440f)) + g * 0.39894228040143267794f * expf(-0.5f * g * g);
}

// Every long sum below runs as four interleaved chains (index mod 4), each in ascending order, joined as
// (c0 + c1) + (c2 + c3): a fixed order with a quarter of the error growth of one chain.
#define TR_JOIN(a) (((a)[0] + (a)[1]) + ((a)[2] + (a)[3]))

// out[t ldo + j] = sum_k in[t ldi + k] W[j K + k] for the TR_TOK rows of a tile
__device__ __forceinline__ void tr_tile_linear(float* out, int ldo, const float* in, int ldi,
                                               const float* __restrict__ W, int J, int K) {
  for (int it = threadIdx.x; it < 2 * J; it += TR_THREADS) {
    const int j = it % J, t0 = (it / J) * 4;
    const float* w = W + (int64_t)j * K;
    float acc[4][4] = {};
    const float* r = in + t0 * ldi;
    int k = 0;
    for (; k + 4 <= K; k += 4) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float wv = w[k + c];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][c] = fmaf(r[t * ldi + k + c], wv, acc[t][c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (k + c < K) {
        const float wv = w[k + c];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][c] = fmaf(r[t * ldi + k + c], wv, acc[t][c]);
      }
#pragma unroll
    for (int t = 0; t < 4; ++t) out[(t0 + t) * ldo + j] = TR_JOIN(acc[t]);
  }
}
// out[t ldo + k] = sum_j in[t ldi + j] W[j K + k] (the transposed product: d input from d output)
__device__ __forceinline__ void tr_tile_linear_t(float* out, int ldo, const float* in, int ldi,
                                                 const float* __restrict__ W, int J, int K) {
  for (int it = threadIdx.x; it < 2 * K; it += TR_THREADS) {
    const int k = it % K, t0 = (it / K) * 4;
    float acc[4][4] = {};
    const float* r = in + t0 * ldi;
    int j = 0;
    for (; j + 4 <= J; j += 4) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float wv = W[(int64_t)(j + c) * K + k];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][c] = fmaf(r[t * ldi + j + c], wv, acc[t][c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (j + c < J) {
        const float wv = W[(int64_t)(j + c) * K + k];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][c] = fmaf(r[t * ldi + j + c], wv, acc[t][c]);
      }
#pragma unroll
    for (int t = 0; t < 4; ++t) out[(t0 + t) * ldo + k] = TR_JOIN(acc[t]);
  }
}
// sum_i a[i sa] b[i sb], i < n, as four chains
__device__ __forceinline__ float tr_dot(const float* a, int sa, const float* b, int sb, int n) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int i = 0;
  for (; i + 4 <= n; i += 4) {
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = fmaf(a[(int64_t)(i + c) * sa], b[(int64_t)(i + c) * sb], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (i + c < n) acc[c] = fmaf(a[(int64_t)(i + c) * sa], b[(int64_t)(i + c) * sb], acc[c]);
  return TR_JOIN(acc);
}
// sum_i a[i] b[i], i < n, rounded once: fp32 products are exact in fp64 and n <= 64 terms lose nothing that fp32 keeps.
// For dP = dO . v in the attention backward, whose terms cancel: dS = P (dP - D) is held relative to dS, not to |dO| |v|.
__device__ __forceinline__ float tr_dot_wide(const float* a, const float* b, int n) {
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc = fma((double)a[i], (double)b[i], acc);
  return (float)acc;
}
// partial[j K + k] (+)= sum_t A[t lda + j] Bm[t ldb + k], t ascending: thread-owned elements of the workgroup's image
__device__ __forceinline__ void tr_tile_wgrad(float* __restrict__ partial, const float* A, int lda, const float* Bm,
                                              int ldb, int J, int K, bool first) {
  for (int e = threadIdx.x; e < J * K; e += TR_THREADS) {
    const int j = e / K, k = e - j * K;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TR_TOK; ++t) s = fmaf(A[t * lda + j], Bm[t * ldb + k], s);
    partial[e] = first ? s : partial[e] + s;
  }
}
// rinv[t] = 1 / sqrt(mean(x[t]^2) + eps)
__device__ __forceinline__ void tr_tile_rinv(float* rinv, const float* x, int F, float eps) {
  if (threadIdx.x < TR_TOK) {
    const float ss = tr_dot(x + threadIdx.x * F, 1, x + threadIdx.x * F, 1, F);
    rinv[threadIdx.x] = 1.0f / sqrtf(ss / (float)F + eps);
  }
}
// RMSNorm backward on a tile: dx = r (dy w - xh mean(dy w xh)), xh = x r; the weight's partial gets sum_t dy xh.
// dacc[t F + f] += dx.  cdot: TR_TOK floats of scratch.
__device__ __forceinline__ void tr_tile_norm_bwd(float* dacc, const float* dy, const float* x, const float* rinv,
                                                 const float* __restrict__ w, float* cdot, float* __restrict__ pw,
                                                 int F, bool first) {
  if (threadIdx.x < TR_TOK) {
    const int t = threadIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < F; ++f) {
      const float term = (dy[t * F + f] * w[f]) * (x[t * F + f] * rinv[t]);
      if ((f & 3) == 0) acc[0] += term;
      else if ((f & 3) == 1) acc[1] += term;
      else if ((f & 3) == 2) acc[2] += term;
      else acc[3] += term;
    }
    cdot[t] = TR_JOIN(acc) / (float)F;
  }
  for (int f = threadIdx.x; f < F; f += TR_THREADS) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TR_TOK; ++t) s = fmaf(dy[t * F + f], x[t * F + f] * rinv[t], s);
    pw[f] = first ? s : pw[f] + s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
    const int t = e / F, f = e - t * F;
    const float xh = x[e] * rinv[t];
    dacc[e] += rinv[t] * (dy[e] * w[f] - xh * cdot[t]);
  }
}

// cos / sin of the position term of column d of a head at position t
__device__ __forceinline__ void tr_angle(const TrPlan& pl, int d, int t, float* c, float* s) {
  const int i = pl.pos == 0 ? d % (pl.hd / 2) : d / 2;
  sincosf((float)t / pl.div[i], s, c);
}

// ---- forward ----------------------------------------------------------------------------------------------------------
// h_0: the scalar projection, or a copy of the strided features
__global__ __launch_bounds__(TR_THREADS) void tr_input_kernel(TrPlan pl, TrArgs a) {
  const int64_t e = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (e >= a.N * pl.F) return;
  const int64_t n = e / pl.F;
  const int f = (int)(e - n * pl.F);
  const int64_t b = n / a.T, t = n - b * a.T;
  const float* xp = a.x + b * a.xbs + t * a.xts;
  a.h_in[e] = pl.scalar ? fmaf(xp[0], a.params[pl.p_spw + f], a.params[pl.p_spb + f]) : xp[f];
}

__global__ __launch_bounds__(TR_THREADS) void tr_qkv_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int F = pl.F, OP = pl.OP, hd = pl.hd;
  float* xs = lds;
  float* raw = xs + TR_TOK * F;
  float* rinv = raw + TR_TOK * OP;
  const float* lp = a.params + pl.p_layer0 + (int64_t)a.layer * pl.PL;
  const int64_t n0 = (int64_t)blockIdx.x * TR_TOK;
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
    const int64_t n = n0 + e / F;
    xs[e] = n < a.N ? a.h_in[n * F + e % F] : 0.f;
  }
  __syncthreads();
  tr_tile_rinv(rinv, xs, F, pl.eps);
  __syncthreads();
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) xs[e] = lp[pl.o_ln1 + e % F] * (xs[e] * rinv[e / F]);
  __syncthreads();
  tr_tile_linear(raw, OP, xs, F, lp + pl.o_qkv, OP, F);
  __syncthreads();
  const int qw = pl.H * hd, kw = pl.KV * hd;
  for (int e = threadIdx.x; e < TR_TOK * OP; e += TR_THREADS) {
    const int tt = e / OP, c = e - tt * OP;
    const int64_t n = n0 + tt;
    if (n >= a.N) continue;
    const int64_t b = n / a.T;
    const int t = (int)(n - b * a.T);
    const float* row = raw + tt * OP;
    float val = row[c];
    if (c < qw + kw && pl.pos != 2) {
      const int cc = c < qw ? c : c - qw;
      const int d = cc % hd;
      float cs, sn;
      tr_angle(pl, d, t, &cs, &sn);
      if (pl.pos == 0) {
        const float rot = d < hd / 2 ? -row[c + hd / 2] : row[c - hd / 2];
        val = val * cs + rot * sn;
      } else {
        val = val + ((d & 1) ? sn : cs);
      }
    }
    if (c < qw) {
      const int head = c / hd, d = c % hd;
      a.q[((b * pl.H + head) * a.T + t) * hd + d] = val;
    } else if (c < qw + kw) {
      const int cc = c - qw, head = cc / hd, d = cc % hd;
      a.k[((b * pl.KV + head) * a.T + t) * hd + d] = val;
    } else {
      const int cc = c - qw - kw, head = cc / hd, d = cc % hd;
      a.v[((b * pl.KV + head) * a.T + t) * hd + d] = val;
    }
  }
}

// one wave per (b, head, query)
__global__ __launch_bounds__(TR_THREADS) void tr_attn_fwd_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int hd = pl.hd, T = (int)a.T;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* sc = lds + wave * (T + hd);
  float* qs = sc + T;
  const int64_t w = (int64_t)blockIdx.x * TR_WAVES + wave;
  const bool active = w < a.B * pl.H * a.T;
  const int64_t wc = active ? w : 0;
  const int q = (int)(wc % T);
  const int head = (int)((wc / T) % pl.H);
  const int64_t b = wc / ((int64_t)T * pl.H);
  const int kvh = head / pl.group;
  const int nk = active ? (pl.causal ? q + 1 : T) : 0;
  const float* kp = a.k + (b * pl.KV + kvh) * (int64_t)T * hd;
  const float* vp = a.v + (b * pl.KV + kvh) * (int64_t)T * hd;
  if (lane < hd) qs[lane] = a.q[wc * hd + lane];
  __syncthreads();
  float m = -INFINITY;
  for (int k = lane; k < nk; k += 64) {
    const float s = tr_dot(qs, 1, kp + (int64_t)k * hd, 1, hd) * pl.scale;
    sc[k] = s;
    m = fmaxf(m, s);
  }
  m = tr_wave_max(m);
  float l = 0.f;
  for (int k = lane; k < nk; k += 64) {
    const float p = expf(sc[k] - m);
    sc[k] = p;
    l += p;
  }
  l = tr_wave_sum(l);
  const int lh = a.layer * pl.H + head;
  for (int k = lane; k < nk; k += 64) {
    float p = sc[k] / l;
    if (a.p > 0.f) p = tr_keep(a.seed_lo, a.seed_hi, lh, (int)b, q, k, a.p) ? p * a.inv_keep : 0.f;
    sc[k] = p;
  }
  if (active && lane == 0 && a.training) a.lse[w] = m + logf(l);
  __syncthreads();
  if (active && lane < hd) {
    a.attn[(b * T + q) * pl.F + head * hd + lane] = tr_dot(sc, 1, vp + lane, hd, nk);
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_tail_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int F = pl.F, I = pl.I;
  float* as = lds;
  float* hs = as + TR_TOK * F;
  float* xn = hs + TR_TOK * F;
  float* gu = xn + TR_TOK * F;
  float* rinv = gu + TR_TOK * 2 * I;
  const float* lp = a.params + pl.p_layer0 + (int64_t)a.layer * pl.PL;
  const int64_t n0 = (int64_t)blockIdx.x * TR_TOK;
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
    const int64_t n = n0 + e / F;
    as[e] = n < a.N ? a.attn[n * F + e % F] : 0.f;
    hs[e] = n < a.N ? a.h_in[n * F + e % F] : 0.f;
  }
  __syncthreads();
  tr_tile_linear(xn, F, as, F, lp + pl.o_ow, F, F);
  __syncthreads();
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
    hs[e] += xn[e];
    const int64_t n = n0 + e / F;
    if (a.training && n < a.N) a.h1[n * F + e % F] = hs[e];
  }
  __syncthreads();
  tr_tile_rinv(rinv, hs, F, pl.eps);
  __syncthreads();
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) xn[e] = lp[pl.o_ln2 + e % F] * (hs[e] * rinv[e / F]);
  __syncthreads();
  tr_tile_linear(gu, 2 * I, xn, F, lp + pl.o_gu, 2 * I, F);
  __syncthreads();
  for (int e = threadIdx.x; e < TR_TOK * I; e += TR_THREADS) {
    const int t = e / I, i = e - t * I;
    gu[t * 2 * I + i] = gu[t * 2 * I + I + i] * tr_act(gu[t * 2 * I + i], pl.act);
  }
  __syncthreads();
  tr_tile_linear(xn, F, gu, 2 * I, lp + pl.o_down, F, I);
  __syncthreads();
  for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
    const int64_t n = n0 + e / F;
    if (n < a.N) a.h_out[n * F + e % F] = hs[e] + xn[e];
  }
}

// out[b] = Wagg (w_n * xh) + b_agg on the last token; one workgroup per sequence
__global__ __launch_bounds__(128) void tr_final_kernel(TrPlan pl, TrArgs a) {
  __shared__ float y[128];
  __shared__ float rs;
  const int F = pl.F;
  const int64_t b = blockIdx.x;
  const float* x = a.h_in + (b * a.T + a.T - 1) * F;
  if (threadIdx.x == 0) {
    rs = 1.0f / sqrtf(tr_dot(x, 1, x, 1, F) / (float)F + pl.eps);
  }
  __syncthreads();
  if (threadIdx.x < F) y[threadIdx.x] = a.params[pl.p_norm + threadIdx.x] * (x[threadIdx.x] * rs);
  __syncthreads();
  if (threadIdx.x < pl.E) {
    const float* w = a.params + pl.p_aggw + (int64_t)threadIdx.x * F;
    a.out[b * pl.E + threadIdx.x] = tr_dot(y, 1, w, 1, F) + a.params[pl.p_aggb + threadIdx.x];
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// last token: d h_L, and the rows the norm / aggregator gradients are summed from
__global__ __launch_bounds__(128) void tr_final_bwd_kernel(TrPlan pl, TrArgs a) {
  __shared__ float dy[128];
  __shared__ float xh[128];
  __shared__ float rs, cm;
  const int F = pl.F, E = pl.E;
  const int64_t b = blockIdx.x;
  const float* x = a.h_in + (b * a.T + a.T - 1) * F;
  if (threadIdx.x == 0) {
    rs = 1.0f / sqrtf(tr_dot(x, 1, x, 1, F) / (float)F + pl.eps);
  }
  __syncthreads();
  if (threadIdx.x < F) {
    const int f = threadIdx.x;
    const float acc = tr_dot(a.gout + b * E, 1, a.params + pl.p_aggw + f, F, E);
    dy[f] = acc;
    xh[f] = x[f] * rs;
    a.ybuf[b * F + f] = a.params[pl.p_norm + f] * xh[f];
    a.cbuf[b * F + f] = acc * xh[f];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float c = 0.f;
    for (int f = 0; f < F; ++f) c = fmaf(dy[f] * a.params[pl.p_norm + f], xh[f], c);
    cm = c / (float)F;
  }
  __syncthreads();
  if (threadIdx.x < F) {
    const int f = threadIdx.x;
    a.dh[(b * a.T + a.T - 1) * F + f] = rs * (dy[f] * a.params[pl.p_norm + f] - xh[f] * cm);
  }
}
// norm.weight, aggregator.weight, aggregator.bias: one thread per element, the sequences as four chains
__global__ __launch_bounds__(TR_THREADS) void tr_final_wgrad_kernel(TrPlan pl, TrArgs a) {
  const int F = pl.F, E = pl.E;
  const int e = blockIdx.x * TR_THREADS + threadIdx.x;
  if (e >= F + E * F + E) return;
  const float one = 1.0f;
  if (e < F) {
    a.grad[pl.p_norm + e] = tr_dot(a.cbuf + e, F, &one, 0, (int)a.B);
  } else if (e < F + E * F) {
    const int o = (e - F) / F, f = (e - F) % F;
    a.grad[pl.p_aggw + e - F] = tr_dot(a.gout + o, E, a.ybuf + f, F, (int)a.B);
  } else {
    const int o = e - F - E * F;
    a.grad[pl.p_aggb + o] = tr_dot(a.gout + o, E, &one, 0, (int)a.B);
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_tail_bwd_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int F = pl.F, I = pl.I;
  float* hs = lds;                    // h'
  float* dh = hs + TR_TOK * F;        // d h'' on entry, d h' on exit
  float* xn = dh + TR_TOK * F;        // u'
  float* as = xn + TR_TOK * F;        // attention output
  float* dxn = as + TR_TOK * F;
  float* gu = dxn + TR_TOK * F;       // (gate | up), then their gradients
  float* da = gu + TR_TOK * 2 * I;    // up act(gate), then its gradient
  float* rinv = da + TR_TOK * I;
  float* cdot = rinv + TR_TOK;
  const float* lp = a.params + pl.p_layer0 + (int64_t)a.layer * pl.PL;
  float* part = a.partial + (int64_t)blockIdx.x * pl.PS;
  const int64_t tile0 = (int64_t)blockIdx.x * a.per;
  const int64_t ntiles = (a.N + TR_TOK - 1) / TR_TOK;
  for (int64_t tile = tile0; tile < tile0 + a.per && tile < ntiles; ++tile) {
    const bool first = tile == tile0;
    const int64_t n0 = tile * TR_TOK;
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
      const int64_t n = n0 + e / F;
      const bool ok = n < a.N;
      hs[e] = ok ? a.h1[n * F + e % F] : 0.f;
      dh[e] = ok ? a.dh[n * F + e % F] : 0.f;
      as[e] = ok ? a.attn[n * F + e % F] : 0.f;
    }
    __syncthreads();
    tr_tile_rinv(rinv, hs, F, pl.eps);
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) xn[e] = lp[pl.o_ln2 + e % F] * (hs[e] * rinv[e / F]);
    __syncthreads();
    tr_tile_linear(gu, 2 * I, xn, F, lp + pl.o_gu, 2 * I, F);
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * I; e += TR_THREADS) {
      const int t = e / I, i = e - t * I;
      da[e] = gu[t * 2 * I + I + i] * tr_act(gu[t * 2 * I + i], pl.act);
    }
    __syncthreads();
    tr_tile_wgrad(part + pl.o_down, dh, F, da, I, F, I, first);
    __syncthreads();
    tr_tile_linear_t(da, I, dh, F, lp + pl.o_down, F, I);
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * I; e += TR_THREADS) {
      const int t = e / I, i = e - t * I;
      const float g = gu[t * 2 * I + i], u = gu[t * 2 * I + I + i], d = da[e];
      gu[t * 2 * I + i] = d * u * tr_dact(g, pl.act);
      gu[t * 2 * I + I + i] = d * tr_act(g, pl.act);
    }
    __syncthreads();
    tr_tile_wgrad(part + pl.o_gu, gu, 2 * I, xn, F, 2 * I, F, first);
    tr_tile_linear_t(dxn, F, gu, 2 * I, lp + pl.o_gu, 2 * I, F);
    __syncthreads();
    tr_tile_norm_bwd(dh, dxn, hs, rinv, lp + pl.o_ln2, cdot, part + pl.o_ln2, F, first);
    __syncthreads();
    tr_tile_wgrad(part + pl.o_ow, dh, F, as, F, F, F, first);
    tr_tile_linear_t(dxn, F, dh, F, lp + pl.o_ow, F, F);
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
      const int64_t n = n0 + e / F;
      if (n < a.N) {
        a.dh[n * F + e % F] = dh[e];
        a.dO[n * F + e % F] = dxn[e];
      }
    }
  }
}

// one wave per (b, head, query): D = sum_k P dP and d q
__global__ __launch_bounds__(TR_THREADS) void tr_attn_bwd_dq_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int hd = pl.hd, T = (int)a.T;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* ds = lds + wave * (2 * T + 2 * hd);
  float* qs = ds + 2 * T;
  float* dos = qs + hd;
  const int64_t w = (int64_t)blockIdx.x * TR_WAVES + wave;
  const bool active = w < a.B * pl.H * a.T;
  const int64_t wc = active ? w : 0;
  const int q = (int)(wc % T);
  const int head = (int)((wc / T) % pl.H);
  const int64_t b = wc / ((int64_t)T * pl.H);
  const int kvh = head / pl.group;
  const int nk = active ? (pl.causal ? q + 1 : T) : 0;
  const float* kp = a.k + (b * pl.KV + kvh) * (int64_t)T * hd;
  const float* vp = a.v + (b * pl.KV + kvh) * (int64_t)T * hd;
  const int64_t orow = (b * T + q) * pl.F + head * hd;
  if (lane < hd) {
    qs[lane] = a.q[wc * hd + lane];
    dos[lane] = a.dO[orow + lane];
  }
  __syncthreads();
  const float lse = a.lse[wc];
  const int lh = a.layer * pl.H + head;
  // D = rowsum(dO o O) = sum_k P[k] dP[k], taken as the P-weighted mean of dP around key 0's: its error is relative
  // to the spread of dP over the row, not to |dO| |O|, a common factor of the rebuilt P cancels, and a row with one
  // key gives dP - D = 0 exactly, as its softmax demands.
  float ref = tr_dot_wide(dos, vp, hd);
  if (a.p > 0.f) ref = tr_keep(a.seed_lo, a.seed_hi, lh, (int)b, q, 0, a.p) ? ref * a.inv_keep : 0.f;
  float num = 0.f, den = 0.f;
  for (int k = lane; k < nk; k += 64) {
    const float s = tr_dot(qs, 1, kp + (int64_t)k * hd, 1, hd);
    const float dp = tr_dot_wide(dos, vp + (int64_t)k * hd, hd);
    const float p = expf(s * pl.scale - lse);
    float pd = dp;
    if (a.p > 0.f) pd = tr_keep(a.seed_lo, a.seed_hi, lh, (int)b, q, k, a.p) ? dp * a.inv_keep : 0.f;
    ds[k] = p;
    ds[T + k] = pd;
    num = fmaf(p, pd - ref, num);
    den += p;
  }
  num = tr_wave_sum(num);
  den = tr_wave_sum(den);
  const float Dv = den > 0.f ? ref + num / den : ref;
  if (active && lane == 0) a.D[w] = Dv;
  for (int k = lane; k < nk; k += 64) ds[k] = ds[k] * (ds[T + k] - Dv);
  __syncthreads();
  if (active && lane < hd) {
    a.dq[wc * hd + lane] = tr_dot(ds, 1, kp + lane, hd, nk) * pl.scale;
  }
}

// one wave per (b, key/value head, key): d k and d v, the query heads of the group in ascending order
__global__ __launch_bounds__(TR_THREADS) void tr_attn_bwd_dkv_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int hd = pl.hd, T = (int)a.T;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* ds = lds + wave * (2 * T + 2 * hd);
  float* pd = ds + T;
  float* ks = pd + T;
  float* vs = ks + hd;
  const int64_t w = (int64_t)blockIdx.x * TR_WAVES + wave;
  const bool active = w < a.B * pl.KV * a.T;
  const int64_t wc = active ? w : 0;
  const int j = (int)(wc % T);
  const int kvh = (int)((wc / T) % pl.KV);
  const int64_t b = wc / ((int64_t)T * pl.KV);
  const int q0 = active ? (pl.causal ? j : 0) : T;
  if (lane < hd) {
    ks[lane] = a.k[wc * hd + lane];
    vs[lane] = a.v[wc * hd + lane];
  }
  float accK[4] = {0.f, 0.f, 0.f, 0.f}, accV[4] = {0.f, 0.f, 0.f, 0.f};      // the group's heads as four chains
  for (int g = 0; g < pl.group; ++g) {
    const int head = kvh * pl.group + g;
    const int lh = a.layer * pl.H + head;
    const float* qp = a.q + (b * pl.H + head) * (int64_t)T * hd;
    const float* lsep = a.lse + (b * pl.H + head) * (int64_t)T;
    const float* Dp = a.D + (b * pl.H + head) * (int64_t)T;
    const float* dop = a.dO + b * (int64_t)T * pl.F + head * hd;
    __syncthreads();
    for (int q = q0 + lane; q < T; q += 64) {
      const float s = tr_dot(qp + (int64_t)q * hd, 1, ks, 1, hd);
      const float dp = tr_dot_wide(dop + (int64_t)q * pl.F, vs, hd);
      const float p = expf(s * pl.scale - lsep[q]);
      float kf = 1.0f;
      if (a.p > 0.f) kf = tr_keep(a.seed_lo, a.seed_hi, lh, (int)b, q, j, a.p) ? a.inv_keep : 0.f;
      ds[q] = p * ((a.p > 0.f ? dp * kf : dp) - Dp[q]);
      pd[q] = p * kf;
    }
    __syncthreads();
    if (lane < hd) {
      const float dK = tr_dot(ds + q0, 1, qp + (int64_t)q0 * hd + lane, hd, T - q0);
      const float dV = tr_dot(pd + q0, 1, dop + (int64_t)q0 * pl.F + lane, pl.F, T - q0);
      if ((g & 3) == 0) { accK[0] += dK; accV[0] += dV; }
      else if ((g & 3) == 1) { accK[1] += dK; accV[1] += dV; }
      else if ((g & 3) == 2) { accK[2] += dK; accV[2] += dV; }
      else { accK[3] += dK; accV[3] += dV; }
    }
  }
  if (active && lane < hd) {
    a.dk[wc * hd + lane] = TR_JOIN(accK) * pl.scale;
    a.dv[wc * hd + lane] = TR_JOIN(accV);
  }
}

__global__ __launch_bounds__(TR_THREADS) void tr_qkv_bwd_kernel(TrPlan pl, TrArgs a) {
  extern __shared__ float lds[];
  const int F = pl.F, OP = pl.OP, hd = pl.hd;
  float* hs = lds;                     // the block's input
  float* dh = hs + TR_TOK * F;         // d h' on entry, d h on exit
  float* xn = dh + TR_TOK * F;         // u
  float* dxn = xn + TR_TOK * F;
  float* dqkv = dxn + TR_TOK * F;
  float* rinv = dqkv + TR_TOK * OP;
  float* cdot = rinv + TR_TOK;
  const float* lp = a.params + pl.p_layer0 + (int64_t)a.layer * pl.PL;
  float* part = a.partial + (int64_t)blockIdx.x * pl.PS;
  const int64_t tile0 = (int64_t)blockIdx.x * a.per;
  const int64_t ntiles = (a.N + TR_TOK - 1) / TR_TOK;
  const int qw = pl.H * hd, kw = pl.KV * hd;
  for (int64_t tile = tile0; tile < tile0 + a.per && tile < ntiles; ++tile) {
    const bool first = tile == tile0;
    const int64_t n0 = tile * TR_TOK;
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
      const int64_t n = n0 + e / F;
      const bool ok = n < a.N;
      hs[e] = ok ? a.h_in[n * F + e % F] : 0.f;
      dh[e] = ok ? a.dh[n * F + e % F] : 0.f;
    }
    // the gradients of q, k, v with the position term undone (the transposed rotation; the additive term passes)
    for (int e = threadIdx.x; e < TR_TOK * OP; e += TR_THREADS) {
      const int tt = e / OP, c = e - tt * OP;
      const int64_t n = n0 + tt;
      float val = 0.f;
      if (n < a.N) {
        const int64_t b = n / a.T;
        const int t = (int)(n - b * a.T);
        if (c < qw + kw) {
          const bool isq = c < qw;
          const int cc = isq ? c : c - qw;
          const int head = cc / hd, d = cc % hd;
          const float* src = isq ? a.dq + ((b * pl.H + head) * a.T + t) * hd : a.dk + ((b * pl.KV + head) * a.T + t) * hd;
          val = src[d];
          if (pl.pos == 0) {
            float cs, sn;
            tr_angle(pl, d, t, &cs, &sn);
            const float other = d < hd / 2 ? src[d + hd / 2] : -src[d - hd / 2];
            val = val * cs + other * sn;
          }
        } else {
          const int cc = c - qw - kw, head = cc / hd, d = cc % hd;
          val = a.dv[((b * pl.KV + head) * a.T + t) * hd + d];
        }
      }
      dqkv[e] = val;
    }
    __syncthreads();
    tr_tile_rinv(rinv, hs, F, pl.eps);
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) xn[e] = lp[pl.o_ln1 + e % F] * (hs[e] * rinv[e / F]);
    __syncthreads();
    tr_tile_wgrad(part + pl.o_qkv, dqkv, OP, xn, F, OP, F, first);
    tr_tile_linear_t(dxn, F, dqkv, OP, lp + pl.o_qkv, OP, F);
    __syncthreads();
    tr_tile_norm_bwd(dh, dxn, hs, rinv, lp + pl.o_ln1, cdot, part + pl.o_ln1, F, first);
    __syncthreads();
    for (int e = threadIdx.x; e < TR_TOK * F; e += TR_THREADS) {
      const int64_t n = n0 + e / F;
      if (n < a.N) a.dh[n * F + e % F] = dh[e];
    }
    if (a.layer == 0 && pl.scalar) {
      // scalar_projection: d w[f] = sum_t d h_0[t, f] x[t], d b[f] = sum_t d h_0[t, f]
      for (int f = threadIdx.x; f < F; f += TR_THREADS) {
        float sw = 0.f, sb = 0.f;
        for (int t = 0; t < TR_TOK; ++t) {
          const int64_t n = n0 + t;
          if (n < a.N) {
            const int64_t b = n / a.T;
            sw = fmaf(dh[t * F + f], a.x[b * a.xbs + (n - b * a.T) * a.xts], sw);
            sb += dh[t * F + f];
          }
        }
        part[pl.PL + f] = first ? sw : part[pl.PL + f] + sw;
        part[pl.PL + F + f] = first ? sb : part[pl.PL + F + f] + sb;
      }
    }
  }
}

// dst[i] = sum_g partial[g stride + src0 + i], the workgroups as four chains
__global__ __launch_bounds__(TR_THREADS) void tr_reduce_kernel(const float* __restrict__ partial, int G, int stride,
                                                               int src0, int n, float* __restrict__ dst) {
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n) return;
  const float one = 1.0f;
  dst[i] = tr_dot(partial + src0 + i, stride, &one, 0, G);
}

__global__ __launch_bounds__(TR_THREADS) void tr_mask_kernel(TrPlan pl, TrArgs a, uint8_t* keep) {
  const int64_t e = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (e >= a.B * pl.H * a.T * a.T) return;
  const int k = (int)(e % a.T);
  const int q = (int)((e / a.T) % a.T);
  const int head = (int)((e / (a.T * a.T)) % pl.H);
  const int64_t b = e / (a.T * a.T * pl.H);
  keep[e] = a.p > 0.f ? (uint8_t)tr_keep(a.seed_lo, a.seed_hi, a.layer * pl.H + head, (int)b, q, k, a.p) : (uint8_t)1;
}
