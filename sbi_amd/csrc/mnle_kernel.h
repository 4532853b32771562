#pragma once
// mnle_kernel.h -- the mixed discrete / continuous likelihood estimator (MNLE) on gfx950 (C ABI: include/sbi_amd_mnle.h).
//
// Execution model = the MDN kernels' (mdn_kernel.h): one wavefront owns 16 rows, lane = (row j, k-slot g); every linear
// runs on v_mfma_f32_16x16x4_f32 with M = output feature, N = row, K = input feature, activations chained through
// registers (lane (j, g), register r of tile mt holds feature 16 mt + 4 r + g).  The networks are context-only and
// small, but their weights (a residual MADE, the combined embedding, T spline-context MLPs) are ~250 KB at the defaults:
// it is cut into STAGES of three zero-padded 64 x 66 matrices (51 KB: a residual block, the embedding, one transform)
// and a workgroup streams one stage at a time from L2 through LDS.  One scheme at every shape.
//   mnle_logp_kernel<K>     log p of paired rows (parts mask; the trials entry point maps row -> (trial, condition))
//   mnle_sample_kernel<K>   V autoregressive passes, value lookup, inverse spline chain
//   mnle_bwd_kernel<K>      training: forward with stashed layer inputs, reverse pass, gradient planes for
//                           maf_dw_kernel / maf_reduce_kernel
#include <hip/hip_runtime.h>
#include <math.h>
#include "mdn_kernel.h"   // the MFMA GEMM pieces (mdn_gemm_*), maf_kernel.h (store_frag_*, weight-gradient interface)
#include "../../include/sbi_amd_mnle.h"

#define MNLE_LD 66                        // row stride of every matrix (= MDN_LDH: the mdn_gemm_* pieces assume it)
#define MNLE_MAT (64 * MNLE_LD + 64)      // weights, then 64 biases
#define MNLE_STAGE (3 * MNLE_MAT)
#define MNLE_CSW 66                       // per-wave condition rows
#define MNLE_DW 18                        // per-wave discrete rows: [0, idx_0 .. idx_3, 0 ..] at 0, raw values at 8
#define MNLE_DA 16                        // the same rows in HBM
#define MNLE_SW 68                        // per-wave output rows (logits / spline parameters)
#define MNLE_ZW 17                        // per-wave spline inputs
#define MNLE_KSH 16
#define MNLE_MAX_LIN 72

struct MnlePlan {
  int V, F, C, Hd, NB, E, Hc, K, T, L, P, PT, Kmax, VK, PF;
  int nc[4];
  int KSC;
  int n_stages, st_final, st_emb, st_tr0;
  int n_lin, n_params, n_virtual, img_floats;
  int sc_cs, sc_din, sc_sc, sc_z, sc_total;
  int log_x;
  float B, min_w, min_h, min_d, inv_sqrt_h, one_minus_kw, one_minus_kh, d_const;   // the spline device functions' PL
  float log_z;
};
struct MnleLayout {
  int g_w[MNLE_MAX_LIN], g_b[MNLE_MAX_LIN];
};

static_assert(MNLE_LD == MDN_LDH, "the shared GEMM pieces hard-code the row stride");

// ------------------------------------------------------------------ small pieces
__device__ __forceinline__ void mnle_stage(float* __restrict__ lds, const float* __restrict__ packed, int s, int tid,
                                           int nthreads) {
  __syncthreads();
  stage_layer(lds, packed + (long long)s * MNLE_STAGE, MNLE_STAGE, tid, nthreads);
  __syncthreads();
}
__device__ __forceinline__ void mnle_relu(f4 (&h)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) h[mt][r] = fmaxf(h[mt][r], 0.f);
}
__device__ __forceinline__ void mnle_zero(f4 (&h)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) h[mt] = {0.f, 0.f, 0.f, 0.f};
}
// g <- g where a > 0 else 0
__device__ __forceinline__ void mnle_relu_bwd(f4 (&g)[4], const f4 (&a)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) g[mt][r] = a[mt][r] > 0.f ? g[mt][r] : 0.f;
}
__device__ __forceinline__ float mnle_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ void load_frag_rows(const float* __restrict__ src, long long row, const LaneId& id,
                                               f4 (&v)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const float4 q = *reinterpret_cast<const float4*>(src + row * 64 + 16 * mt + 4 * id.g);
    v[mt] = {q.x, q.y, q.z, q.w};
  }
}
// out = W in + b, `in` in registers / in a per-wave LDS row buffer
__device__ __forceinline__ void mnle_lin_reg(const float* __restrict__ M, const LaneId& id, const f4 (&in)[4],
                                             f4 (&out)[4]) {
  mdn_bias_h(M + 64 * MNLE_LD, id, out);
  mdn_gemm_reg<MNLE_KSH>(M, id, in, out);
}
__device__ __forceinline__ void mnle_lin_lds(const float* __restrict__ M, const LaneId& id,
                                             const float* __restrict__ brow, int ks, f4 (&out)[4]) {
  mdn_bias_h(M + 64 * MNLE_LD, id, out);
  mdn_gemm_lds(M, MNLE_LD, id, brow, ks, out);
}
// natural-order output rows [0, 16 mtiles) of `M in + b` -> the wave's row buffer
__device__ __forceinline__ void mnle_rows_out(const float* __restrict__ M, const LaneId& id, const f4 (&in)[4],
                                              int mtiles, float* __restrict__ sc) {
  for (int mt = 0; mt < mtiles; ++mt) {
    const f4 v = mdn_head_tile<MNLE_KSH>(M, M + 64 * MNLE_LD, id, in, mt);
    *reinterpret_cast<float4*>(sc + id.j * MNLE_SW + 16 * mt + 4 * id.g) = float4{v[0], v[1], v[2], v[3]};
  }
}
// acc (input feature 16 mt + 4 r + g) += sum_k W[k][feature] g[k], g = the wave's row buffer, 4 ks rows of W
__device__ __forceinline__ void mnle_gemm_T_lds(const float* __restrict__ M, const LaneId& id,
                                                const float* __restrict__ sc, int ks, f4 (&acc)[4]) {
  const float* a0 = M + id.g * MNLE_LD + id.iperm;
  const float* b0 = sc + id.j * MNLE_SW + id.g;
  for (int s = 0; s < ks; ++s) {
    const float bv = b0[4 * s];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a0[4 * s * MNLE_LD + 16 * mt], bv, acc[mt]);
  }
}

struct MnleRows {
  float* cs;    // 16 x MNLE_CSW standardised condition
  float* din;   // 16 x MNLE_DW
  float* sc;    // 16 x MNLE_SW
  float* zz;    // 16 x MNLE_ZW
};
struct MnleStash {
  float* act;            // slot-major (slot, npad, 64) layer inputs, fragment order
  long long stride;      // npad * 64
  long long row;
  bool valid;
};

__device__ __forceinline__ void mnle_load_cond(const MnlePlan& P, const LaneId& id, const float* __restrict__ zstats,
                                               const float* __restrict__ c, long long cr, float* __restrict__ cs) {
  const float* cm = zstats + 2;
  const float* csd = cm + P.C;
  for (int q = id.g; q < 4 * P.KSC; q += 4)
    cs[id.j * MNLE_CSW + q] = q < P.C ? (c[cr * P.C + q] - cm[q]) / csd[q] : 0.f;
}
__device__ __forceinline__ void mnle_load_disc(const MnlePlan& P, const LaneId& id, const int* __restrict__ d_idx,
                                               const float* __restrict__ d_val, long long xr,
                                               float* __restrict__ din) {
  for (int q = id.g; q < 16; q += 4) {
    float v = 0.f;
    if (q >= 1 && q <= P.V && d_idx) {
      int k = d_idx[xr * P.V + q - 1];
      const int top = P.nc[q - 1] - 1;
      k = k < 0 ? 0 : (k > top ? top : k);
      v = (float)k;
    } else if (q >= 8 && q < 8 + P.V && d_val) {
      v = d_val[xr * P.V + q - 8];
    }
    din[id.j * MNLE_DW + q] = v;
  }
}

// ------------------------------------------------------------------ discrete net: logits of the V variables -> R.sc
// (stages 0 .. st_final; on return the final stage is resident and h holds the final layer's input)
template <bool STASH>
__device__ __forceinline__ void mnle_disc_fwd(const MnlePlan& P, float* __restrict__ lds,
                                              const float* __restrict__ packed, const LaneId& id, int tid, int nthreads,
                                              const MnleRows& R, const MnleStash& S, f4 (&h)[4]) {
  const float* M0 = lds;
  const float* M1 = lds + MNLE_MAT;
  const float* M2 = lds + 2 * MNLE_MAT;
  const float* crow = R.cs + id.j * MNLE_CSW + id.g;
  f4 t[4], a[4];
  mnle_stage(lds, packed, 0, tid, nthreads);
  mnle_lin_lds(M0, id, R.din + id.j * MNLE_DW + id.g, 2, h);
  mnle_lin_lds(M1, id, crow, P.KSC, t);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) h[mt][r] += fmaxf(t[mt][r], 0.f);
  for (int b = 0; b < P.NB; ++b) {
    mnle_stage(lds, packed, 1 + b, tid, nthreads);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) a[mt] = h[mt];
    mnle_relu(a);
    if (STASH) store_frag_rows(S.act + (2 * b) * S.stride, 64, S.row, S.valid, id, a);
    mnle_lin_reg(M0, id, a, t);
    mnle_relu(t);
    if (STASH) store_frag_rows(S.act + (2 * b + 1) * S.stride, 64, S.row, S.valid, id, t);
    mnle_lin_reg(M1, id, t, a);
    mnle_lin_lds(M2, id, crow, P.KSC, t);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) h[mt][r] = fmaf(a[mt][r], mnle_sigmoid(t[mt][r]), h[mt][r]);
  }
  mnle_stage(lds, packed, P.st_final, tid, nthreads);
  if (STASH) store_frag_rows(S.act + (2 * P.NB) * S.stride, 64, S.row, S.valid, id, h);
  mnle_rows_out(M0, id, h, (P.VK + 15) >> 4, R.sc);
  wave_lds_fence();
}
// lane g == v: log-softmax of variable v at its index (idx from R.din), lse returned; the row's sum over v in order
__device__ __forceinline__ float mnle_disc_logp(const MnlePlan& P, const LaneId& id, const MnleRows& R, float& lse,
                                                int& idx) {
  float lp = 0.f;
  lse = 0.f;
  idx = 0;
  if (id.g < P.V) {
    const float* lg = R.sc + id.j * MNLE_SW + id.g * P.Kmax;
    const int nc = P.nc[id.g];
    idx = (int)R.din[id.j * MNLE_DW + 1 + id.g];
    float m = lg[0];
    for (int k = 1; k < nc; ++k) m = fmaxf(m, lg[k]);
    float s = 0.f;
    for (int k = 0; k < nc; ++k) s += expf(lg[k] - m);
    lse = m + logf(s);
    lp = lg[idx] - lse;
  }
  const float a0 = __shfl(lp, id.j), a1 = __shfl(lp, id.j + 16), a2 = __shfl(lp, id.j + 32),
              a3 = __shfl(lp, id.j + 48);
  return ((a0 + a1) + a2) + a3;
}

// ------------------------------------------------------------------ continuous net
// combined embedding e (stage st_emb); e1 = the first layer's output
template <bool STASH>
__device__ __forceinline__ void mnle_embed(const MnlePlan& P, float* __restrict__ lds,
                                           const float* __restrict__ packed, const LaneId& id, int tid, int nthreads,
                                           const MnleRows& R, const MnleStash& S, int slot0, f4 (&e)[4]) {
  const float* M0 = lds;
  const float* M1 = lds + MNLE_MAT;
  const float* M2 = lds + 2 * MNLE_MAT;
  f4 e1[4];
  mnle_stage(lds, packed, P.st_emb, tid, nthreads);
  mnle_lin_lds(M0, id, R.cs + id.j * MNLE_CSW + id.g, P.KSC, e1);
  mdn_gemm_lds(M1, MNLE_LD, id, R.din + id.j * MNLE_DW + 8 + id.g, 1, e1);
  mnle_relu(e1);
  if (STASH) store_frag_rows(S.act + slot0 * S.stride, 64, S.row, S.valid, id, e1);
  mnle_lin_reg(M2, id, e1, e);
  mnle_relu(e);
  if (STASH) store_frag_rows(S.act + (slot0 + 1) * S.stride, 64, S.row, S.valid, id, e);
}
// transform t's spline parameters -> R.sc (stage st_tr0 + t); hh = the final layer's input
template <bool STASH>
__device__ __forceinline__ void mnle_params(const MnlePlan& P, float* __restrict__ lds,
                                            const float* __restrict__ packed, const LaneId& id, int tid, int nthreads,
                                            const MnleRows& R, const MnleStash& S, int slot0, int t, const f4 (&e)[4]) {
  const float* M0 = lds;
  const float* M1 = lds + MNLE_MAT;
  const float* M2 = lds + 2 * MNLE_MAT;
  f4 hh[4], t2[4];
  mnle_stage(lds, packed, P.st_tr0 + t, tid, nthreads);
  mnle_lin_reg(M0, id, e, hh);
  mnle_relu(hh);
  if (STASH) store_frag_rows(S.act + (slot0 + t * (P.L + 1)) * S.stride, 64, S.row, S.valid, id, hh);
  for (int l = 0; l < P.L; ++l) {
    mnle_lin_reg(M1, id, hh, t2);
    mnle_relu(t2);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) hh[mt] = t2[mt];
    if (STASH) store_frag_rows(S.act + (slot0 + t * (P.L + 1) + l + 1) * S.stride, 64, S.row, S.valid, id, hh);
  }
  mnle_rows_out(M2, id, hh, P.PT, R.sc);
  wave_lds_fence();
}
// the spline chain on a scalar per row (all four lanes of a row hold the same value): forward returns z_T and adds the
// log|det| terms, the inverse runs t = T-1 .. 0
template <int K, bool INV, bool STASH>
__device__ __forceinline__ float mnle_chain(const MnlePlan& P, float* __restrict__ lds,
                                            const float* __restrict__ packed, const LaneId& id, int tid, int nthreads,
                                            const MnleRows& R, const MnleStash& S, int slot0, const f4 (&e)[4],
                                            float z, float& ld_acc) {
  for (int i = 0; i < P.T; ++i) {
    const int t = INV ? P.T - 1 - i : i;
    mnle_params<STASH>(P, lds, packed, id, tid, nthreads, R, S, slot0, t, e);
    if (STASH && id.g == 0) R.zz[id.j * MNLE_ZW + t] = z;
    float y, ld;
    rq_spline_pair<K, INV>(R.sc + id.j * MNLE_SW, z, P, id.g >> 1, y, ld);
    z = y;
    ld_acc += ld;
    wave_lds_fence();
  }
  return z;
}
// The flow's input and the closing sum in double: beyond the tails (|z| > tail_bound) the density is -z^2 / 2 of a
// value of magnitude 10+, where one fp32 ulp of z already moves the result by 1e-5.
__device__ __forceinline__ float mnle_flow_input(const MnlePlan& P, const float* __restrict__ zstats, float x,
                                                 double& xl) {
  xl = P.log_x ? log((double)x) : (double)x;
  return (float)(xl * (double)zstats[1] + (double)zstats[0]);
}
__device__ __forceinline__ double mnle_cont_logp(const MnlePlan& P, const float* __restrict__ zstats, float z,
                                                 float ld_acc, double xl) {
  double lp = ((-0.5 * ((double)z * (double)z) - (double)P.log_z) + (double)ld_acc) + log(fabs((double)zstats[1]));
  if (P.log_x) lp -= xl;
  return lp;
}

// ------------------------------------------------------------------ log_prob (paired rows; trials: x row = row / x_div)
template <int K>
__global__ void __launch_bounds__(256)
mnle_logp_kernel(const MnlePlan P, const float* __restrict__ packed, const float* __restrict__ zstats,
                 const float* __restrict__ x_cont, const int* __restrict__ d_idx, const float* __restrict__ d_val,
                 const float* __restrict__ c, long long n, long long c_rows, long long x_div, int parts,
                 float* __restrict__ logp_out, float* __restrict__ logits_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* scr = lds + MNLE_STAGE + wave * P.sc_total;
  const MnleRows R = {scr + P.sc_cs, scr + P.sc_din, scr + P.sc_sc, scr + P.sc_z};
  const MnleStash S = {nullptr, 0, 0, false};
  const long long row = (long long)blockIdx.x * (16 * nw) + 16 * wave + id.j;
  const bool valid = row < n;
  const long long rs = valid ? row : 0;
  const long long xr = rs / x_div;
  mnle_load_cond(P, id, zstats, c, rs % c_rows, R.cs);
  mnle_load_disc(P, id, d_idx, d_val, xr, R.din);
  wave_lds_fence();
  float total = 0.f;
  if (parts & 1) {
    f4 h[4];
    mnle_disc_fwd<false>(P, lds, packed, id, tid, nthreads, R, S, h);
    float lse;
    int idx;
    total = mnle_disc_logp(P, id, R, lse, idx);
    if (logits_out && valid && id.g < P.V) {
      const float* lg = R.sc + id.j * MNLE_SW + id.g * P.Kmax;
      for (int k = 0; k < P.Kmax; ++k)
        logits_out[(row * P.V + id.g) * P.Kmax + k] = k < P.nc[id.g] ? lg[k] : -INFINITY;
    }
    wave_lds_fence();
  }
  if (parts & 2) {
    f4 e[4];
    mnle_embed<false>(P, lds, packed, id, tid, nthreads, R, S, 0, e);
    double xl;
    const float z0 = mnle_flow_input(P, zstats, x_cont[xr], xl);
    float ld = 0.f;
    const float z = mnle_chain<K, false, false>(P, lds, packed, id, tid, nthreads, R, S, 0, e, z0, ld);
    const double lc = mnle_cont_logp(P, zstats, z, ld, xl);
    total = (float)((parts & 1) ? (double)total + lc : lc);
  }
  if (valid && id.g == 0) logp_out[row] = total;
}

#ifdef MNLE_MAIN_TU   // non-template kernels: defined by mnle.hip only
// out[j] = sum_t ws[t * N + j], t ascending
__global__ void __launch_bounds__(256)
mnle_trial_sum_kernel(const float* __restrict__ ws, long long T, long long N, float* __restrict__ out) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  float s = 0.f;
  for (long long t = 0; t < T; ++t) s += ws[t * N + j];
  out[j] = s;
}
#endif

// ------------------------------------------------------------------ sample
template <int K>
__global__ void __launch_bounds__(256)
mnle_sample_kernel(const MnlePlan P, const float* __restrict__ packed, const float* __restrict__ zstats,
                   const float* __restrict__ u, const float* __restrict__ noise, const float* __restrict__ c,
                   long long n, long long c_rows, int* __restrict__ d_idx_out, float* __restrict__ x_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* scr = lds + MNLE_STAGE + wave * P.sc_total;
  const MnleRows R = {scr + P.sc_cs, scr + P.sc_din, scr + P.sc_sc, scr + P.sc_z};
  const MnleStash S = {nullptr, 0, 0, false};
  const long long row = (long long)blockIdx.x * (16 * nw) + 16 * wave + id.j;
  const bool valid = row < n;
  const long long rs = valid ? row : 0;
  const float* lookup = zstats + 2 + 2 * P.C;
  mnle_load_cond(P, id, zstats, c, rs % c_rows, R.cs);
  mnle_load_disc(P, id, nullptr, nullptr, 0, R.din);
  wave_lds_fence();
  for (int v = 0; v < P.V; ++v) {
    f4 h[4];
    mnle_disc_fwd<false>(P, lds, packed, id, tid, nthreads, R, S, h);
    if (id.g == v) {
      const float* lg = R.sc + id.j * MNLE_SW + v * P.Kmax;
      const int nc = P.nc[v];
      const float uv = u[rs * P.V + v];
      float m = lg[0];
      for (int k = 1; k < nc; ++k) m = fmaxf(m, lg[k]);
      float s = 0.f;
      for (int k = 0; k < nc; ++k) s += expf(lg[k] - m);
      float cum = 0.f;
      int pick = 0;
      for (int k = 0; k < nc; ++k) {
        cum += expf(lg[k] - m) / s;
        pick += cum < uv ? 1 : 0;
      }
      pick = pick < nc - 1 ? pick : nc - 1;
      R.din[id.j * MNLE_DW + 1 + v] = (float)pick;
      R.din[id.j * MNLE_DW + 8 + v] = lookup[v * 16 + pick];
      if (valid) d_idx_out[row * P.V + v] = pick;
    }
    wave_lds_fence();
  }
  f4 e[4];
  mnle_embed<false>(P, lds, packed, id, tid, nthreads, R, S, 0, e);
  float ld = 0.f;
  const float z = mnle_chain<K, true, false>(P, lds, packed, id, tid, nthreads, R, S, 0, e, noise[rs], ld);
  float x = (z - zstats[0]) / zstats[1];
  if (P.log_x) x = expf(x);
  if (valid && id.g == 0) x_out[row] = x;
}

// ------------------------------------------------------------------ training
struct MnleBwdArgs {
  const float* packed;
  const float* zstats;
  const float* x_cont;
  const int* d_idx;
  const float* d_val;
  const float* c;
  const float* row_w;
  float uni_w;
  long long n, c_rows, npad;
  float* loss;        // optional (n)
  float* grad_cond;   // optional (n, C)
  float* CTX;         // (npad, 64) standardised condition, natural order
  float* DIN;         // (npad, 16) [0, idx .., 0 | values .., 0]
  float* ACT;         // (slots, npad, 64) layer inputs, fragment order: blocks 2b, 2b+1 | 2NB final | e1, e | T x (L+1)
  float* G;           // (gslots, 4 planes) gradients wrt 64-wide pre-activations, fragment order:
                      //   0 initial, 1 context, 2+3b L0 / L1 / block context, then Wa, Wb, per transform W0, W1 x L
  float* GF;          // PF planes: gradient wrt the (V+1) Kmax final outputs, natural order
  float* GP;          // (T, PT planes): gradient wrt the spline parameters, natural order
};

template <int K>
__global__ void __launch_bounds__(256)
mnle_bwd_kernel(const MnlePlan P, const MnleBwdArgs a) {
  constexpr int PT = (3 * K - 1 + 15) / 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* scr = lds + MNLE_STAGE + wave * P.sc_total;
  const MnleRows R = {scr + P.sc_cs, scr + P.sc_din, scr + P.sc_sc, scr + P.sc_z};
  const long long n = a.n, npad = a.npad;
  const long long row0 = (long long)blockIdx.x * (16 * nw) + 16 * wave;
  const long long row = row0 + id.j;
  const bool valid = row < n;
  const long long rs = valid ? row : 0;
  const MnleStash S = {a.ACT, npad * 64, row, valid};
  const float* M0 = lds;
  const float* M1 = lds + MNLE_MAT;
  const float* M2 = lds + 2 * MNLE_MAT;
  const float* crow = R.cs + id.j * MNLE_CSW + id.g;
  const long long gs = 4 * npad * 16;      // floats per 64-wide gradient slot
  mnle_load_cond(P, id, a.zstats, a.c, rs % a.c_rows, R.cs);
  mnle_load_disc(P, id, a.d_idx, a.d_val, rs, R.din);
  wave_lds_fence();
  if (valid) {
    for (int q = id.g; q < 64; q += 4) a.CTX[row * 64 + q] = q < 4 * P.KSC ? R.cs[id.j * MNLE_CSW + q] : 0.f;
    for (int q = id.g; q < MNLE_DA; q += 4) a.DIN[row * MNLE_DA + q] = R.din[id.j * MNLE_DW + q];
  }
  const float wn = valid ? (a.row_w ? a.row_w[row] : a.uni_w) : 0.f;
  f4 gc[4];          // gradient wrt the standardised condition
  mnle_zero(gc);
  // ================================================================ discrete part
  float lp_d;
  {
    f4 h[4], gh[4];
    mnle_disc_fwd<true>(P, lds, a.packed, id, tid, nthreads, R, S, h);
    float lse;
    int idx;
    lp_d = mnle_disc_logp(P, id, R, lse, idx);
    wave_lds_fence();
    if (id.g < P.V) {
      float* lg = R.sc + id.j * MNLE_SW + id.g * P.Kmax;
      const int nc = P.nc[id.g];
      for (int k = 0; k < P.Kmax; ++k)
        lg[k] = k < nc ? wn * (expf(lg[k] - lse) - (k == idx ? 1.f : 0.f)) : 0.f;
    }
    wave_lds_fence();
    // the 16 x (V+1) Kmax block -> GF (dummy columns and padding: zero)
    for (int q = id.lane; q < 16 * 16 * P.PF; q += 64) {
      const int rl = q / (16 * P.PF), col = q - rl * (16 * P.PF);
      const long long rr = row0 + rl;
      if (rr < n) {
        const int src = col - P.Kmax;
        const float v = (src >= 0 && src < P.VK) ? R.sc[rl * MNLE_SW + src] : 0.f;
        a.GF[((long long)(col >> 4) * npad + rr) * 16 + (col & 15)] = v;
      }
    }
    mnle_zero(gh);
    mnle_gemm_T_lds(M0, id, R.sc, (P.VK + 3) >> 2, gh);
    wave_lds_fence();
    for (int b = P.NB - 1; b >= 0; --b) {
      mnle_stage(lds, a.packed, 1 + b, tid, nthreads);
      f4 a0[4], a1[4], t1[4], gt[4], g1[4], gg[4];
      load_frag_rows(a.ACT + (2 * b) * S.stride, rs, id, a0);
      load_frag_rows(a.ACT + (2 * b + 1) * S.stride, rs, id, a1);
      if (!valid) {
        mnle_zero(a0);
        mnle_zero(a1);
      }
      mnle_lin_reg(M1, id, a1, t1);
      mnle_lin_lds(M2, id, crow, P.KSC, gt);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sg = mnle_sigmoid(gt[mt][r]);
          g1[mt][r] = gh[mt][r] * sg;
          gg[mt][r] = gh[mt][r] * t1[mt][r] * (sg * (1.f - sg));
        }
      store_frag_planes(a.G + (long long)(3 + 3 * b) * gs, npad, row, valid, id, g1);
      store_frag_planes(a.G + (long long)(4 + 3 * b) * gs, npad, row, valid, id, gg);
      mdn_gemm_T_reg<MNLE_KSH>(M2, id, gg, gc);
      mnle_zero(t1);
      mdn_gemm_T_reg<MNLE_KSH>(M1, id, g1, t1);
      mnle_relu_bwd(t1, a1);
      store_frag_planes(a.G + (long long)(2 + 3 * b) * gs, npad, row, valid, id, t1);
      mnle_zero(gt);
      mdn_gemm_T_reg<MNLE_KSH>(M0, id, t1, gt);
      mnle_relu_bwd(gt, a0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) gh[mt] += gt[mt];
    }
    mnle_stage(lds, a.packed, 0, tid, nthreads);
    store_frag_planes(a.G, npad, row, valid, id, gh);
    f4 c1[4];
    mnle_lin_lds(M1, id, crow, P.KSC, c1);
    mnle_relu_bwd(gh, c1);
    store_frag_planes(a.G + gs, npad, row, valid, id, gh);
    mdn_gemm_T_reg<MNLE_KSH>(M1, id, gh, gc);
  }
  // ================================================================ continuous part
  const int slot0 = 2 * P.NB + 1;          // e1, e, then the transforms' layer inputs
  const int gslot0 = 2 + 3 * P.NB;         // Wa, Wb, then per transform W0, W1 x L
  {
    f4 e[4], ge[4];
    mnle_embed<true>(P, lds, a.packed, id, tid, nthreads, R, S, slot0, e);
    double xl;
    const float z0 = mnle_flow_input(P, a.zstats, a.x_cont[rs], xl);
    float ld = 0.f;
    const float z = mnle_chain<K, false, true>(P, lds, a.packed, id, tid, nthreads, R, S, slot0 + 2, e, z0, ld);
    const double lp_c = mnle_cont_logp(P, a.zstats, z, ld, xl);
    if (a.loss && valid && id.g == 0) a.loss[row] = -(float)((double)lp_d + lp_c);
    float gy = wn * z;
    const float gld = -wn;
    mnle_zero(ge);
    for (int t = P.T - 1; t >= 0; --t) {
      mnle_stage(lds, a.packed, P.st_tr0 + t, tid, nthreads);
      const int as = slot0 + 2 + t * (P.L + 1);
      const int gsl = gslot0 + 2 + t * (P.L + 1);
      f4 hh[4], ghh[4], g2[4];
      load_frag_rows(a.ACT + (long long)(as + P.L) * S.stride, rs, id, hh);
      if (!valid) mnle_zero(hh);
      mnle_rows_out(M2, id, hh, PT, R.sc);
      wave_lds_fence();
      float yv, gxv = 0.f;
      if ((id.g & 1) == 0)
        rq_spline_pair_bwd<K>(R.sc + id.j * MNLE_SW, 16 * PT, R.zz[id.j * MNLE_ZW + t], gy, gld, P, id.g >> 1, yv,
                              gxv);
      gy = __shfl(gxv, id.j);
      wave_lds_fence();
      store_param_planes<PT>(a.GP + (long long)t * PT * npad * 16, npad, row, valid, id, R.sc, 0, MNLE_SW, 0, 1);
      mnle_zero(ghh);
      mnle_gemm_T_lds(M2, id, R.sc, 4 * PT, ghh);
      wave_lds_fence();
      for (int l = P.L; l >= 1; --l) {
        mnle_relu_bwd(ghh, hh);
        store_frag_planes(a.G + (long long)(gsl + l) * gs, npad, row, valid, id, ghh);
        mnle_zero(g2);
        mdn_gemm_T_reg<MNLE_KSH>(M1, id, ghh, g2);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) ghh[mt] = g2[mt];
        load_frag_rows(a.ACT + (long long)(as + l - 1) * S.stride, rs, id, hh);
        if (!valid) mnle_zero(hh);
      }
      mnle_relu_bwd(ghh, hh);
      store_frag_planes(a.G + (long long)gsl * gs, npad, row, valid, id, ghh);
      mdn_gemm_T_reg<MNLE_KSH>(M0, id, ghh, ge);
    }
    mnle_stage(lds, a.packed, P.st_emb, tid, nthreads);
    f4 e1[4], g1[4];
    mnle_relu_bwd(ge, e);
    store_frag_planes(a.G + (long long)(gslot0 + 1) * gs, npad, row, valid, id, ge);
    mnle_zero(g1);
    mdn_gemm_T_reg<MNLE_KSH>(M2, id, ge, g1);
    load_frag_rows(a.ACT + (long long)slot0 * S.stride, rs, id, e1);
    if (!valid) mnle_zero(e1);
    mnle_relu_bwd(g1, e1);
    store_frag_planes(a.G + (long long)gslot0 * gs, npad, row, valid, id, g1);
    mdn_gemm_T_reg<MNLE_KSH>(M0, id, g1, gc);
  }
  if (a.grad_cond && valid) {
    const float* csd = a.zstats + 2 + P.C;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * mt + 4 * r + id.g;
        if (f < P.C) a.grad_cond[row * P.C + f] = gc[mt][r] / csd[f];
      }
  }
}

#ifdef MNLE_MAIN_TU
// grad[i] = g[i] (+ the later applications of a transform's shared context layer, in application order)
__global__ void __launch_bounds__(256)
mnle_fold_kernel(const MnlePlan P, const MnleLayout Ly, const float* __restrict__ g, float* __restrict__ grad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n_params) return;
  float v = g[i];
  if (P.L > 1) {
    const int blk = P.Hc * P.Hc + P.Hc;
    const int lin0 = 5 + 3 * P.NB;
    for (int t = 0; t < P.T; ++t) {
      const int w0 = Ly.g_w[lin0 + 3 * t + 1];
      if (i >= w0 && i < w0 + blk)
        for (int l = 1; l < P.L; ++l) v += g[P.n_params + (t * (P.L - 1) + (l - 1)) * blk + (i - w0)];
    }
  }
  grad[i] = v;
}
#endif

__global__ void __launch_bounds__(256)
mnle_pack_kernel(const MnlePlan P, const MnleLayout Ly, const float* __restrict__ p, float* __restrict__ img);
__global__ void __launch_bounds__(256)
mnle_mask_kernel(const MnlePlan P, const MnleLayout Ly, float* __restrict__ mask);

// ------------------------------------------------------------------ per-K launchers (one translation unit per K)
struct MnleCall {
  int mode;                 // 0 log_prob, 1 sample, 2 training
  int nw, lds_bytes;
  const float* packed;
  const float* zstats;
  const float* x_cont;      // mode 1: noise
  const int* d_idx;
  const float* d_val;       // mode 1: uniforms
  const float* c;
  long long n, c_rows, x_div;
  int parts;
  float* out0;              // log_prob | x_cont_out
  float* out1;              // logits_out
  int* idx_out;
  const MnleBwdArgs* bwd;
};
template <int K>
int mnle_dispatch_k(const MnlePlan& P, const MnleCall& q, hipStream_t st) {
  const unsigned grid = (unsigned)((q.n + 16 * q.nw - 1) / (16 * q.nw));
  const void* fn = q.mode == 0 ? (const void*)mnle_logp_kernel<K>
                               : (q.mode == 1 ? (const void*)mnle_sample_kernel<K> : (const void*)mnle_bwd_kernel<K>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, q.lds_bytes);
  if (e != hipSuccess) return (int)e;
  if (q.mode == 0)
    hipLaunchKernelGGL(mnle_logp_kernel<K>, dim3(grid), dim3(64 * q.nw), (size_t)q.lds_bytes, st, P, q.packed,
                       q.zstats, q.x_cont, q.d_idx, q.d_val, q.c, q.n, q.c_rows, q.x_div, q.parts, q.out0, q.out1);
  else if (q.mode == 1)
    hipLaunchKernelGGL(mnle_sample_kernel<K>, dim3(grid), dim3(64 * q.nw), (size_t)q.lds_bytes, st, P, q.packed,
                       q.zstats, q.d_val, q.x_cont, q.c, q.n, q.c_rows, q.idx_out, q.out0);
  else
    hipLaunchKernelGGL(mnle_bwd_kernel<K>, dim3(grid), dim3(64 * q.nw), (size_t)q.lds_bytes, st, P, *q.bwd);
  return (int)hipGetLastError();
}
