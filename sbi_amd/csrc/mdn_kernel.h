#pragma once
// mdn_kernel.h -- the mixture-density-network posterior estimator on gfx950 (C ABI: include/sbi_amd_mdn.h).
//
// Execution model = the NSF / MAF kernels' (nsf_device.h): one wavefront owns 16 rows, lane = (row j, k-slot g); the
// two hidden linears run on v_mfma_f32_16x16x4_f32 with M = output feature, N = row, K = input feature, activations
// chained through registers (lane (j, g), register r of tile mt holds feature 16 mt + 4 r + g).  The head (K (1 + 2D
// + U) outputs) is never materialised per row: the kernels loop over the components, a workgroup stages ONE
// component's slice of the head (<= 160 rows x 66 floats, 43 KB) from L2 into LDS, every wave runs that slice's GEMM
// for its 16 rows into a per-wave LDS row buffer and the four lanes of a row share the triangular mat-vec, the
// quadratic form and the online log-sum-exp.  One scheme at every shape (always stream): the whole head is 150 KB at
// the defaults and 630 KB at the envelope's corner, so it cannot live in LDS next to the row buffers anyway.
//   mdn_flow_kernel<KSH, MODE>   MODE 0 log_prob, 1 sample, 2 components            (paired rows)
//   mdn_bcast_kernel<KSH, MODE>  MODE 0 log_prob, 1 sample; x_rows == 1: the network runs once per workgroup, the rows
//                                then cost K quadratic forms / one gather + back-substitution (same device functions
//                                as the paired kernel => bit-identical results)
//   mdn_bwd_kernel<KSH>          training: forward (pass A: per-component terms), then per component the head gradient
//                                (pass B), W^T back-propagation, gradient planes for maf_dw_kernel / maf_reduce_kernel
#include <hip/hip_runtime.h>
#include <math.h>
#include "maf_kernel.h"   // nsf_device.h + store_frag_rows / store_frag_planes + the weight-gradient kernels' interface
#include "../../include/sbi_amd_mdn.h"

#define MDN_LDH 66         // row stride of the (H <= 64 column) images: 2 * odd, conflict-free ds_read_b32
#define MDN_ZW 17          // per-wave row buffers of <= 16 floats
#define MDN_AW 64          // activation / condition rows in HBM

struct MdnPlan {
  int D, C, H, K, U, R, RP, MT;   // R = 1 + 2D + U rows per component slice, RP = 16 MT
  int KS1, ld1;                   // first layer: K-steps, row stride
  int o_w1, o_b1, o_w2, o_b2, o_lg, o_lgb, hid_floats;   // image: hidden layers + logits tile
  int slice_floats, img_floats;   // component slices start at hid_floats
  int g_w[6], g_b[6], n_params;   // flat offsets: hidden.0, hidden.2, logits, means, diagonal, upper
  int SW;                         // per-wave head row buffer stride
  int sc_z, sc_y, sc_t, sc_c, sc_s, sc_total;   // per-wave scratch (floats)
  int bc_z, bc_c, bc_x, bc_total;               // per-wave scratch of the one-observation kernels
  float eps, log_z;
};

__global__ void __launch_bounds__(256)
mdn_pack_kernel(const MdnPlan P, const float* __restrict__ p, float* __restrict__ img);

// ------------------------------------------------------------------ GEMM pieces (all images zero padded: no guards)
__device__ __forceinline__ void mdn_bias_h(const float* __restrict__ b, const LaneId& id, f4 (&acc)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[mt][r] = b[16 * mt + 4 * r + id.g];
}
// hidden layout out, B operand from a per-wave LDS row (brow = &buf[j * stride + g])
__device__ __forceinline__ void mdn_gemm_lds(const float* __restrict__ w, int ld, const LaneId& id,
                                             const float* __restrict__ brow, int ks, f4 (&acc)[4]) {
  const float* a0 = w + id.iperm * ld + id.g;
  for (int s = 0; s < ks; ++s) {
    const float bv = brow[4 * s];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a0[16 * mt * ld + 4 * s], bv, acc[mt]);
  }
}
// hidden layout out, B operand = the previous layer's D fragments
template <int KSH>
__device__ __forceinline__ void mdn_gemm_reg(const float* __restrict__ w, const LaneId& id, const f4 (&b)[4],
                                             f4 (&acc)[4]) {
  const float* a0 = w + id.iperm * MDN_LDH + id.g;
#pragma unroll
  for (int s = 0; s < KSH; ++s) {
    const float bv = b[s >> 2][s & 3];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a0[16 * mt * MDN_LDH + 4 * s], bv, acc[mt]);
  }
}
// acc[mt] (input feature 16 mt + 4 r + g) += sum_k W[k][feature] g[k], g = D fragments of the layer's output gradient
template <int KSH>
__device__ __forceinline__ void mdn_gemm_T_reg(const float* __restrict__ w, const LaneId& id, const f4 (&gb)[4],
                                               f4 (&acc)[4]) {
  const float* a0 = w + id.g * MDN_LDH + id.iperm;
#pragma unroll
  for (int s = 0; s < KSH; ++s) {
    const float bv = gb[s >> 2][s & 3];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = MFMA16(a0[4 * s * MDN_LDH + 16 * mt], bv, acc[mt]);
  }
}
// one 16-row tile of a component slice: rows 16 mt + 4 g + r of lane (j, g) (natural order), B = h2 fragments.
// The bias is added LAST: a chain that starts from it rounds every K-step at the bias's magnitude, and the raw
// diagonal's bias can dwarf W h (raw entries near softplus's threshold of 20: 7 ulp of 20 against half an ulp).
template <int KSH>
__device__ __forceinline__ f4 mdn_head_tile(const float* __restrict__ wk, const float* __restrict__ bk,
                                            const LaneId& id, const f4 (&h)[4], int mt) {
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* a0 = wk + (16 * mt + id.j) * MDN_LDH + id.g;
#pragma unroll
  for (int s = 0; s < KSH; ++s) acc = MFMA16(a0[4 * s], h[s >> 2][s & 3], acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] += bk[16 * mt + 4 * id.g + r];
  return acc;
}
// all tiles of a slice -> the wave's row buffer sc[j][0 .. RP)
template <int KSH>
__device__ __forceinline__ void mdn_head_rows(const float* __restrict__ wk, const MdnPlan& P, const LaneId& id,
                                              const f4 (&h)[4], float* __restrict__ sc) {
  const float* bk = wk + P.RP * MDN_LDH;
  for (int mt = 0; mt < P.MT; ++mt) {
    const f4 v = mdn_head_tile<KSH>(wk, bk, id, h, mt);
    *reinterpret_cast<float4*>(sc + id.j * P.SW + 16 * mt + 4 * id.g) = float4{v[0], v[1], v[2], v[3]};
  }
}

// standardised condition rows -> cs (zero padded to 4 KS1 columns), then h1, h2
template <int KSH>
__device__ __forceinline__ void mdn_hidden(const float* __restrict__ lds, const MdnPlan& P, const LaneId& id,
                                           const float* __restrict__ cs, f4 (&h1)[4], f4 (&h2)[4]) {
  mdn_bias_h(lds + P.o_b1, id, h1);
  mdn_gemm_lds(lds + P.o_w1, P.ld1, id, cs + id.j * P.ld1 + id.g, P.KS1, h1);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) h1[mt][r] = fmaxf(h1[mt][r], 0.f);
  mdn_bias_h(lds + P.o_b2, id, h2);
  mdn_gemm_reg<KSH>(lds + P.o_w2, id, h1, h2);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) h2[mt][r] = fmaxf(h2[mt][r], 0.f);
}

// ------------------------------------------------------------------ per-row mixture arithmetic (pinned: libm expf /
// logf / log1pf, explicit fmaf -- the paired and the broadcast kernels must produce the same bits)
// p: the row's component parameters [logit | mu (D) | raw diagonal (D) | upper (U)], z: the row's standardised theta.
// The four lanes of a row take the factor's rows i = g, g + 4, ...; returns log w~_k + log N_k with w~ the RAW logit.
__device__ __forceinline__ float mdn_term(const MdnPlan& P, const float* __restrict__ p, const float* __restrict__ z,
                                          int g, float* __restrict__ ys) {
  const int D = P.D;
  float q = 0.f, dd = 0.f, ldet = 0.f;
  for (int i = g; i < D; i += 4) {
    const float a = softplus_f(p[1 + D + i]);
    const float di = z[i] - p[1 + i];
    float y = a * di;
    const float* up = p + 1 + 2 * D + (i * (2 * D - i - 1)) / 2 - i - 1;   // up[j] = A[i][j], j > i
    for (int j = i + 1; j < D; ++j) y = fmaf(up[j], z[j] - p[1 + j], y);
    q = fmaf(y, y, q);
    dd = fmaf(di, di, dd);
    ldet += logf(a);
    if (ys) ys[i] = y;
  }
  float v = fmaf(-0.5f, fmaf(P.eps, dd, q), ldet);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return (p[0] + v) - P.log_z;
}
struct MdnLse {
  float m, s;
};
__device__ __forceinline__ void lse_push(MdnLse& L, float v) {
  if (v > L.m) {
    L.s = fmaf(L.s, expf(L.m - v), 1.f);
    L.m = v;
  } else {
    L.s += expf(v - L.m);
  }
}
__device__ __forceinline__ float lse_value(const MdnLse& L) { return L.m + logf(L.s); }
__device__ __forceinline__ float mdn_log_scale_sum(const MdnPlan& P, const float* __restrict__ zstats) {
  float s = 0.f;
  for (int d = 0; d < P.D; ++d) s += logf(fabsf(zstats[P.D + d]));
  return s;
}
// component of a row from u: the number of cumulative softmax weights <= u, clamped; lg: K logits, stride `st`
__device__ __forceinline__ int mdn_pick(const MdnPlan& P, const float* __restrict__ lg, int st, float u) {
  float m = lg[0];
  for (int k = 1; k < P.K; ++k) m = fmaxf(m, lg[k * st]);
  float S = 0.f;
  for (int k = 0; k < P.K; ++k) S += expf(lg[k * st] - m);
  float cum = 0.f;
  int c = 0;
  for (int k = 0; k < P.K; ++k) {
    cum += expf(lg[k * st] - m) / S;
    c += cum <= u ? 1 : 0;
  }
  return c < P.K - 1 ? c : P.K - 1;
}
// theta = (mu + A^{-1} zeta) scale + shift by back-substitution; xs: D floats of private scratch
__device__ __forceinline__ void mdn_backsub(const MdnPlan& P, const float* __restrict__ p,
                                            const float* __restrict__ zeta, const float* __restrict__ zstats,
                                            float* __restrict__ xs, float* __restrict__ out, bool write) {
  const int D = P.D;
  for (int i = D - 1; i >= 0; --i) {
    float acc = zeta[i];
    const float* up = p + 1 + 2 * D + (i * (2 * D - i - 1)) / 2 - i - 1;
    for (int j = i + 1; j < D; ++j) acc = fmaf(-up[j], xs[j], acc);
    xs[i] = acc / softplus_f(p[1 + D + i]);
  }
  if (write)
    for (int i = 0; i < D; ++i) out[i] = fmaf(p[1 + i] + xs[i], zstats[D + i], zstats[i]);
}

// rows of this wave: standardised theta -> zs, standardised condition -> cs
__device__ __forceinline__ void mdn_load_rows(const MdnPlan& P, const LaneId& id, const float* __restrict__ zstats,
                                              const float* __restrict__ theta, const float* __restrict__ x,
                                              long long row, bool valid, long long x_rows, float* __restrict__ zs,
                                              float* __restrict__ cs) {
  const int D = P.D, C = P.C;
  if (theta)
    for (int d = id.g; d < D; d += 4)
      zs[id.j * MDN_ZW + d] = valid ? (theta[row * D + d] - zstats[d]) / zstats[D + d] : 0.f;
  if (cs) {
    const long long xr = valid ? row % x_rows : 0;
    const float* xm = zstats + 2 * D;
    const float* xsd = xm + C;
    for (int c = id.g; c < 4 * P.KS1; c += 4)
      cs[id.j * P.ld1 + c] = (c < C && valid) ? (x[xr * C + c] - xm[c]) / xsd[c] : 0.f;
  }
}

// ------------------------------------------------------------------ paired kernel
template <int KSH, int MODE>
__global__ void __launch_bounds__(256)
mdn_flow_kernel(const MdnPlan P, const float* __restrict__ packed, const float* __restrict__ zstats,
                const float* __restrict__ theta /* MODE 1: zeta */, const float* __restrict__ x,
                const float* __restrict__ u, const int* __restrict__ comp, long long n, long long x_rows,
                float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ out2) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* slice = lds + P.hid_floats;
  float* scr = slice + P.slice_floats + wave * P.sc_total;
  float* zs = scr + P.sc_z;
  float* ys = scr + P.sc_y;
  float* cs = scr + P.sc_c;
  float* sc = scr + P.sc_s;
  const long long row = (long long)blockIdx.x * (16 * nw) + 16 * wave + id.j;
  const bool valid = row < n;
  const int D = P.D, K = P.K;
  stage_layer(lds, packed, P.hid_floats, tid, nthreads);
  mdn_load_rows(P, id, zstats, MODE == 0 ? theta : nullptr, x, row, valid, MODE == 2 ? n : x_rows, zs, cs);
  __syncthreads();
  f4 h1[4], h2[4];
  mdn_hidden<KSH>(lds, P, id, cs, h1, h2);
  int mine = 0;
  if (MODE == 1) {
    if (comp) {
      mine = valid ? comp[row] : 0;
      mine = mine < 0 ? 0 : (mine > K - 1 ? K - 1 : mine);
    } else {
      const f4 v = mdn_head_tile<KSH>(lds + P.o_lg, lds + P.o_lgb, id, h2, 0);
      *reinterpret_cast<float4*>(sc + id.j * P.SW + 4 * id.g) = float4{v[0], v[1], v[2], v[3]};
      wave_lds_fence();
      mine = mdn_pick(P, sc + id.j * P.SW, 1, valid ? u[row] : 0.f);
      wave_lds_fence();
    }
  }
  MdnLse lt = {-INFINITY, 0.f}, ll = {-INFINITY, 0.f};
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    stage_layer(slice, packed + P.hid_floats + (long long)k * P.slice_floats, P.slice_floats, tid, nthreads);
    __syncthreads();
    mdn_head_rows<KSH>(slice, P, id, h2, sc);
    wave_lds_fence();
    const float* p = sc + id.j * P.SW;
    if (MODE == 0) {
      const float t = mdn_term(P, p, zs + id.j * MDN_ZW, id.g, nullptr);
      lse_push(lt, t);
      lse_push(ll, p[0]);
    } else if (MODE == 1) {
      // (every component's slice passes by and a row acts on its own only: K slice GEMMs per tile for one needed;
      //  the four g-lanes of a row run the same back-substitution into the same ys row -- equal values, lane g == 0
      //  writes the result -- so that the one-observation kernel's one-lane-per-row form is the same arithmetic)
      if (mine == k)
        mdn_backsub(P, p, theta + (valid ? row : 0) * D, zstats, ys + id.j * MDN_ZW, out0 + (valid ? row : 0) * D,
                    valid && id.g == 0);
    } else if (valid) {
      if (id.g == 0) out0[row * K + k] = p[0];
      for (int d = id.g; d < D; d += 4) {
        out1[(row * K + k) * D + d] = p[1 + d];
        out2[(row * K + k) * (D + P.U) + d] = softplus_f(p[1 + D + d]);
      }
      for (int e = id.g; e < P.U; e += 4) out2[(row * K + k) * (D + P.U) + D + e] = p[1 + 2 * D + e];
    }
    wave_lds_fence();
  }
  if (MODE == 0 && valid && id.g == 0) out0[row] = (lse_value(lt) - lse_value(ll)) - mdn_log_scale_sum(P, zstats);
}

// ------------------------------------------------------------------ one observation
template <int KSH, int MODE>
__global__ void __launch_bounds__(256)
mdn_bcast_kernel(const MdnPlan P, const float* __restrict__ packed, const float* __restrict__ zstats,
                 const float* __restrict__ theta /* MODE 1: zeta */, const float* __restrict__ x,
                 const float* __restrict__ u, const int* __restrict__ comp, long long n, float* __restrict__ out0) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* pbuf = lds + P.hid_floats;                  // K x RP: every component's parameters for the one condition
  float* slice = pbuf + P.K * P.RP;                  // staging buffer of one component slice
  float* scr = slice + P.slice_floats + wave * P.bc_total;
  float* zs = scr + P.bc_z;
  float* cs = scr + P.bc_c;
  float* xs = scr + P.bc_x;                          // MODE 1: 64 x MDN_ZW back-substitution rows
  const int D = P.D, K = P.K;
  stage_layer(lds, packed, P.hid_floats, tid, nthreads);
  mdn_load_rows(P, id, zstats, nullptr, x, 0, true, 1, nullptr, cs);
  __syncthreads();
  {
    // once per workgroup: the hidden net (every wave, 16 equal columns), then the head slice by slice through the
    // staging buffer (coalesced 16-byte copies from L2), the slice's m-tiles shared among the waves
    f4 h1[4], h2[4];
    mdn_hidden<KSH>(lds, P, id, cs, h1, h2);
    for (int k = 0; k < K; ++k) {
      if (k > 0) __syncthreads();
      stage_layer(slice, packed + P.hid_floats + (long long)k * P.slice_floats, P.slice_floats, tid, nthreads);
      __syncthreads();
      const float* bk = slice + P.RP * MDN_LDH;
      for (int mt = wave; mt < P.MT; mt += nw) {
        const f4 v = mdn_head_tile<KSH>(slice, bk, id, h2, mt);
        if (id.j == 0)
          *reinterpret_cast<float4*>(pbuf + k * P.RP + 16 * mt + 4 * id.g) = float4{v[0], v[1], v[2], v[3]};
      }
    }
  }
  __syncthreads();
  const float lsc = mdn_log_scale_sum(P, zstats);
  if (MODE == 0) {
    MdnLse ll = {-INFINITY, 0.f};
    for (int k = 0; k < K; ++k) lse_push(ll, pbuf[k * P.RP]);
    const float lw = lse_value(ll);
    const long long ntiles = (n + 15) / 16;
    for (long long t = (long long)blockIdx.x * nw + wave; t < ntiles; t += (long long)gridDim.x * nw) {
      const long long row = 16 * t + id.j;
      const bool valid = row < n;
      mdn_load_rows(P, id, zstats, theta, nullptr, row, valid, 1, zs, nullptr);
      wave_lds_fence();
      MdnLse lt = {-INFINITY, 0.f};
      for (int k = 0; k < K; ++k) lse_push(lt, mdn_term(P, pbuf + k * P.RP, zs + id.j * MDN_ZW, id.g, nullptr));
      if (valid && id.g == 0) out0[row] = (lse_value(lt) - lw) - lsc;
      wave_lds_fence();
    }
  } else {
    const long long ngroups = (n + 63) / 64;         // one lane per row: a gather and a back-substitution
    for (long long t = (long long)blockIdx.x * nw + wave; t < ngroups; t += (long long)gridDim.x * nw) {
      const long long row = 64 * t + id.lane;
      const bool valid = row < n;
      const long long rs = valid ? row : 0;
      int mine;
      if (comp) {
        mine = comp[rs];
        mine = mine < 0 ? 0 : (mine > K - 1 ? K - 1 : mine);
      } else {
        mine = mdn_pick(P, pbuf, P.RP, u[rs]);
      }
      mdn_backsub(P, pbuf + mine * P.RP, theta + rs * D, zstats, xs + id.lane * MDN_ZW, out0 + rs * D, valid);
    }
  }
}

// ------------------------------------------------------------------ training
struct MdnBwdArgs {
  const float* packed;
  const float* zstats;
  const float* theta;
  const float* x;
  const float* row_w;
  float uni_w;
  long long n, x_rows, npad;
  float* loss;          // optional (n)
  float* grad_theta;    // optional (n, D)
  float* CTX;           // (npad, 64) standardised condition rows, natural order
  float* ACT1;          // (npad, 64) h1, fragment order (store_frag_rows)
  float* ACT2;          // (npad, 64) h2
  float* G1;            // 4 planes d/d(pre-activation 1), fragment order (store_frag_planes)
  float* G2;            // 4 planes d/d(pre-activation 2)
  float* GH[4];         // gradient planes of logits (K cols), means (K D), diagonal (K D), upper (K U): natural order
};

template <int KSH>
__global__ void __launch_bounds__(256)
mdn_bwd_kernel(const MdnPlan P, const MdnBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* slice = lds + P.hid_floats;
  float* scr = slice + P.slice_floats + wave * P.sc_total;
  float* zs = scr + P.sc_z;
  float* ys = scr + P.sc_y;
  float* tk = scr + P.sc_t;
  float* cs = scr + P.sc_c;
  float* sc = scr + P.sc_s;
  const long long n = a.n;
  const long long row0 = (long long)blockIdx.x * (16 * nw) + 16 * wave;
  const long long row = row0 + id.j;
  const bool valid = row < n;
  const int D = P.D, K = P.K, U = P.U, R = P.R;
  stage_layer(lds, a.packed, P.hid_floats, tid, nthreads);
  mdn_load_rows(P, id, a.zstats, a.theta, a.x, row, valid, a.x_rows, zs, cs);
  __syncthreads();
  if (valid)
    for (int c = id.g; c < MDN_AW; c += 4) a.CTX[row * MDN_AW + c] = c < 4 * P.KS1 ? cs[id.j * P.ld1 + c] : 0.f;
  f4 h1[4], h2[4];
  mdn_hidden<KSH>(lds, P, id, cs, h1, h2);
  store_frag_rows(a.ACT1, MDN_AW, row, valid, id, h1);
  store_frag_rows(a.ACT2, MDN_AW, row, valid, id, h2);
  const float* zrow = zs + id.j * MDN_ZW;
  const float* p = sc + id.j * P.SW;
  // ---- pass A: log w~_k + log N_k of every component, the two log-sum-exps
  MdnLse lt = {-INFINITY, 0.f}, ll = {-INFINITY, 0.f};
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    stage_layer(slice, a.packed + P.hid_floats + (long long)k * P.slice_floats, P.slice_floats, tid, nthreads);
    __syncthreads();
    mdn_head_rows<KSH>(slice, P, id, h2, sc);
    wave_lds_fence();
    const float t = mdn_term(P, p, zrow, id.g, nullptr);
    lse_push(lt, t);
    lse_push(ll, p[0]);
    if (id.g == 0) tk[id.j * MDN_ZW + k] = t;
    wave_lds_fence();
  }
  const float lse_t = lse_value(lt), lse_l = lse_value(ll);
  if (a.loss && valid && id.g == 0) a.loss[row] = mdn_log_scale_sum(P, a.zstats) - (lse_t - lse_l);
  const float wn = valid ? (a.row_w ? a.row_w[row] : a.uni_w) : 0.f;
  // ---- pass B: head gradient per component, g_h2 += W_k^T g_k, gradient planes
  f4 gh[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) gh[mt] = {0.f, 0.f, 0.f, 0.f};
  float gz[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    stage_layer(slice, a.packed + P.hid_floats + (long long)k * P.slice_floats, P.slice_floats, tid, nthreads);
    __syncthreads();
    mdn_head_rows<KSH>(slice, P, id, h2, sc);
    wave_lds_fence();
    mdn_term(P, p, zrow, id.g, ys + id.j * MDN_ZW);      // y = A d of this component
    wave_lds_fence();
    const float logit = p[0];
    const float rk = expf(tk[id.j * MDN_ZW + k] - lse_t);
    const float wk_ = expf(logit - lse_l);
    const float cw = wn * rk;
    const float* yrow = ys + id.j * MDN_ZW;
    float* pw = sc + id.j * P.SW;
    wave_lds_fence();
    // lane g owns the columns jj = g, g + 4, ... of the factor: everything it overwrites is read by it alone
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int jj = id.g + 4 * uu;
      if (jj < D) {
        const float raw = pw[1 + D + jj];
        const float ajj = softplus_f(raw);
        const float dj = zrow[jj] - pw[1 + jj];
        float v = fmaf(P.eps, dj, ajj * yrow[jj]);
        for (int i = 0; i < jj; ++i) {
          float* e = pw + 1 + 2 * D + (i * (2 * D - i - 1)) / 2 + (jj - i - 1);
          v = fmaf(*e, yrow[i], v);
          *e = cw * yrow[i] * dj;
        }
        const float sg = raw > 20.f ? 1.f : 1.f / (1.f + expf(-raw));
        pw[1 + D + jj] = cw * (yrow[jj] * dj - 1.f / ajj) * sg;
        pw[1 + jj] = -cw * v;
        gz[uu] = fmaf(cw, v, gz[uu]);
      }
    }
    if (id.g == 0) pw[0] = wn * (wk_ - rk);
    wave_lds_fence();
    // g_h2 += W_k^T g_k: M = hidden feature, K = slice row (rows >= R: zero weights meet zero gradients)
    {
      const float* a0 = slice + id.g * MDN_LDH + id.iperm;
      const float* b0 = sc + id.j * P.SW + id.g;
      for (int s = 0; s < 4 * P.MT; ++s) {
        const float bv = b0[4 * s];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) gh[mt] = MFMA16(a0[4 * s * MDN_LDH + 16 * mt], bv, gh[mt]);
      }
    }
    // the 16 x R gradient block -> the four heads' planes (consecutive lanes: consecutive columns)
    for (int idx = id.lane; idx < 16 * R; idx += 64) {
      const int rl = idx / R, c = idx - rl * R;
      const long long rr = row0 + rl;
      if (rr < n) {
        int which, col;
        if (c == 0) { which = 0; col = k; }
        else if (c < 1 + D) { which = 1; col = k * D + c - 1; }
        else if (c < 1 + 2 * D) { which = 2; col = k * D + c - 1 - D; }
        else { which = 3; col = k * U + c - 1 - 2 * D; }
        a.GH[which][((long long)(col >> 4) * a.npad + rr) * 16 + (col & 15)] = sc[rl * P.SW + c];
      }
    }
    wave_lds_fence();
  }
  // ---- back through the two ReLU layers
  f4 g2[4], g1[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool live = 16 * mt + 4 * r + id.g < P.H;
      g2[mt][r] = (live && h2[mt][r] > 0.f) ? gh[mt][r] : 0.f;
      g1[mt][r] = 0.f;
    }
  store_frag_planes(a.G2, a.npad, row, valid, id, g2);
  mdn_gemm_T_reg<KSH>(lds + P.o_w2, id, g2, g1);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool live = 16 * mt + 4 * r + id.g < P.H;
      g1[mt][r] = (live && h1[mt][r] > 0.f) ? g1[mt][r] : 0.f;
    }
  store_frag_planes(a.G1, a.npad, row, valid, id, g1);
  if (a.grad_theta && valid) {
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
      const int jj = id.g + 4 * uu;
      if (jj < D) a.grad_theta[row * D + jj] = gz[uu] / a.zstats[D + jj];
    }
  }
}
