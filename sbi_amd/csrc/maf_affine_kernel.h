#pragma once
// maf_affine_kernel.h -- sbi's default `maf` on gfx950: masked autoregressive flow with AFFINE transforms
// (sbi build_maf, flow.py:115-209; arithmetic = nflows 0.14 MaskedAffineAutoregressiveTransform + RandomPermutation).
//
// The conditioner is the MADE of maf_kernel.h (made_gate / made_hidden: every linear on v_mfma_f32_16x16x4_f32,
// weights in the LDS image staged once per transform, activations chained through registers).  What differs is the
// head.  The final layer is packed DE-INTERLEAVED as two dense m-tiles
//     image row 16 * tile + d  =  nflows row 2 d + tile      (tile 0: scale logits u_d, tile 1: shifts s_d)
// so ONE two-tile GEMM leaves, in lane (row j, slot g), u and s of the dims 4 r + g in registers r = 0..3 of two D
// fragments.  The transform, its log-det and its reverse mode are VALU on those registers: no per-dimension
// parameter staging in LDS, 2 instead of D * PT m-tiles on the MFMA pipe.  Backward: the D fragments (g_u | g_shift)
// are the B operand of the transposed GEMM Wf^T g (K = the 32 image rows), chained without LDS staging.
//   maf_aff_pack_kernel            : flat nflows params -> masked images
//   maf_aff_flow_kernel<KSH,false> : theta, x -> log p [+ noise] [+ per-transform input stash]
//   maf_aff_flow_kernel<KSH,true > : noise, x -> theta [+ logabsdet]   D passes per transform (pass i fixes dim i)
//   maf_aff_trials_kernel<KSH>     : sum over iid trials of log q(x_i | theta_c), terms bit-identical to the paired kernel
//   maf_aff_bwd_kernel<KSH>        : per transform, row-parallel backward; operands of maf_dw_kernel left in HBM
//   maf_aff_reduce_kernel          : fixed-order sum of the split-K partials, final layer back to nflows' row order
#include "maf_kernel.h"
#include "../../include/sbi_amd_maf_affine.h"

#define MAF_AFF_TC 8       // trials whose flow states a wave keeps in LDS at once (trials kernel)

struct MafAffPlan {
  MafPlan m;               // n.shape[0].lin[fin]: the two-tile final layer (32 image rows); n.P = 2; sc_pst unused
  float eps;
  int sc_tz, sc_tld;       // trials kernel: MAF_AFF_TC flow states (16 rows x ZW each) and log-det accumulators
  int tz_stride;
};

// softplus(u) + eps and sigmoid(u) = d softplus / du, no overflow for any finite u: t = exp(-|u|) <= 1
__device__ __forceinline__ float aff_scale(float u, float eps, float& sig) {
  const float t = exp_f(-fabsf(u));
  const float inv = rcp_nr(1.f + t);
  sig = u >= 0.f ? inv : t * inv;
  return (fmaxf(u, 0.f) + log1pf(t)) + eps;
}

// [u ; s] = Wf h + bf as ONE two-tile GEMM: lane (j, g) register r <- dim 4 r + g of row j
template <int KSH>
__device__ __forceinline__ void aff_final(const float* __restrict__ lds, const LinDesc& L, const LaneId& id,
                                          const f4 (&h)[NSF_HT], f4& u, f4& s) {
  const int ro0 = L.l_w + id.iperm * L.ldk + id.g, ro1 = ro0 + 16 * L.ldk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    u[r] = lds[L.l_b + 4 * r + id.g];
    s[r] = lds[L.l_b + 16 + 4 * r + id.g];
  }
#pragma unroll
  for (int k = 0; k < KSH; ++k) {
    const float bv = h[k >> 2][k & 3];
    u = MFMA16(lds[ro0 + 4 * k], bv, u);
    s = MFMA16(lds[ro1 + 4 * k], bv, s);
  }
}

// one transform of the forward direction on the wave's state rows `zs`: conditioner on the current state, affine
// map on all D dims, permutation.  Shared by the paired and the trials kernel (explicit fmaf: no contraction choice
// is left to the compiler, so both produce the same bits).
template <int KSH>
__device__ __forceinline__ void aff_transform_fwd(const float* __restrict__ lds, const MafAffPlan& ap,
                                                  const LaneId& id, float* __restrict__ zs, float* __restrict__ cin,
                                                  const f4 (&gate)[NSF_HT], float& ld_acc) {
  const NsfPlan& pl = ap.m.n;
  const ShapeDesc& S = pl.shape[0];
  const int D = pl.D;
  for (int k = id.g; k < D; k += 4) cin[id.j * pl.CINW + k] = zs[id.j * pl.ZW + k];
  wave_lds_fence();
  f4 h[NSF_HT], u, s;
  made_hidden<KSH, 0>(lds, pl, S, id, cin + id.j * pl.CINW + id.g, gate, h);
  aff_final<KSH>(lds, S.lin[S.fin], id, h, u, s);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int d = 4 * r + id.g;
    if (d < D) {
      float sig;
      const float sc = aff_scale(u[r], ap.eps, sig);
      const int zi = id.j * pl.ZW + d;
      zs[zi] = fmaf(sc, zs[zi], s[r]);
      ld_acc += logf(sc);
    }
  }
  wave_lds_fence();
  permute_rows(zs, pl.ZW, D, lds + ap.m.l_perm, id);
}

// base density of the wave's final states: log N(z; 0, I) + accumulated log-det, summed over the four k-slots
__device__ __forceinline__ float aff_base_logp(const NsfPlan& pl, const LaneId& id, const float* __restrict__ zs,
                                               float ld_acc) {
  float part = 0.f;
  for (int d = id.g; d < pl.D; d += 4) {
    const float z = zs[id.j * pl.ZW + d];
    part = fmaf(z, z, part);
  }
  float v = fmaf(-0.5f, part, ld_acc);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v - pl.log_z;
}

// z-scoring of one input row into the state rows; returns this lane's share of log|det|
__device__ __forceinline__ float aff_load_input(const NsfPlan& pl, const LaneId& id, const float* __restrict__ zstats,
                                                const float* __restrict__ in_row, bool valid,
                                                float* __restrict__ zs) {
  float ld = 0.f;
  for (int d = id.g; d < pl.D; d += 4) {
    const float v = valid ? in_row[d] : 0.f;
    zs[id.j * pl.ZW + d] = fmaf(v, zstats[pl.D + d], zstats[d]);
    ld += logf(fabsf(zstats[pl.D + d]));
  }
  return ld;
}

__device__ __forceinline__ void aff_load_context(const NsfPlan& pl, const LaneId& id, const float* __restrict__ zstats,
                                                 const float* __restrict__ x_row, bool valid,
                                                 float* __restrict__ cin) {
  const float* x_mean = zstats + 2 * pl.D;
  const float* x_std = x_mean + pl.C;
  for (int c = id.g; c < pl.C; c += 4)
    cin[id.j * pl.CINW + pl.D + c] = ((valid ? x_row[c] : 0.f) - x_mean[c]) / x_std[c];
}

template <int KSH, bool INV>
__global__ void __launch_bounds__(512)
maf_aff_flow_kernel(const MafAffPlan ap, const float* __restrict__ packed, const float* __restrict__ zstats,
                    const float* __restrict__ in, const float* __restrict__ x, long long n, long long x_rows,
                    float* __restrict__ out_main, float* __restrict__ out_aux, float* __restrict__ z_stash) {
  const MafPlan& mp = ap.m;
  const NsfPlan& pl = mp.n;
  const ShapeDesc& S = pl.shape[0];
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* sc = lds + pl.lds_w_floats + wave * mp.sc_total;
  float* zs = sc + mp.sc_zs;
  float* us = sc + mp.sc_us;
  float* cin = sc + mp.sc_cin;
  const long long row = (long long)blockIdx.x * (16 * nw) + 16 * wave + id.j;
  const bool valid = row < n;
  const long long rs = valid ? row : 0;
  const int D = pl.D;
  float ld_acc = 0.f;
  for (int i = id.lane; i < mp.sc_total; i += 64) sc[i] = 0.f;
  wave_lds_fence();
  {
    const long long xr = (x_rows == n) ? rs : (x_rows == 1 ? 0 : rs % x_rows);
    if (!INV) ld_acc = aff_load_input(pl, id, zstats, in + rs * D, valid, zs);
    else
      for (int d = id.g; d < D; d += 4) zs[id.j * pl.ZW + d] = valid ? in[rs * D + d] : 0.f;
    aff_load_context(pl, id, zstats, x + xr * pl.C, valid, cin);
  }
  wave_lds_fence();
  const float* cin_row = cin + id.j * pl.CINW + id.g;

  for (int li = 0; li < pl.T; ++li) {
    const int t = INV ? (pl.T - 1 - li) : li;
    __syncthreads();
    stage_layer(lds, packed + (long long)t * pl.img_floats, pl.img_floats, tid, nthreads);
    __syncthreads();
    f4 gate[NSF_HT];
    made_gate<KSH>(lds, S, id, cin_row + D, gate);
    if (!INV) {
      if (z_stash) {
        for (int d = id.g; d < D; d += 4)
          if (valid) z_stash[((long long)t * n + row) * D + d] = zs[id.j * pl.ZW + d];
      }
      aff_transform_fwd<KSH>(lds, ap, id, zs, cin, gate, ld_acc);
    } else {
      permute_rows(zs, pl.ZW, D, lds + mp.l_iperm, id);   // inverse of the permutation that FOLLOWS the transform
      for (int k = id.g; k < D; k += 4) cin[id.j * pl.CINW + k] = 0.f;
      wave_lds_fence();
      // autoregressive inverse (D passes from zeros): pass i sees the exact outputs of the dims < i, which is all
      // dim i depends on; its (u, s) sit in register i >> 2 of the lanes with slot g == (i & 3)
      for (int i = 0; i < D; ++i) {
        f4 h[NSF_HT], u, s;
        made_hidden<KSH, 0>(lds, pl, S, id, cin_row, gate, h);
        aff_final<KSH>(lds, S.lin[S.fin], id, h, u, s);
        const int ri = i >> 2;
        const float uu = ri == 0 ? u[0] : (ri == 1 ? u[1] : (ri == 2 ? u[2] : u[3]));
        const float ss = ri == 0 ? s[0] : (ri == 1 ? s[1] : (ri == 2 ? s[2] : s[3]));
        if (id.g == (i & 3)) {
          float sig;
          const float scl = aff_scale(uu, ap.eps, sig);
          const float z = (zs[id.j * pl.ZW + i] - ss) / scl;
          cin[id.j * pl.CINW + i] = z;
          us[id.j * pl.ZW + i] = z;
          ld_acc -= logf(scl);
        }
        wave_lds_fence();
      }
      for (int k = id.g; k < D; k += 4) zs[id.j * pl.ZW + k] = us[id.j * pl.ZW + k];
      wave_lds_fence();
    }
  }

  if (!INV) {
    if (out_aux && valid)
      for (int d = id.g; d < D; d += 4) out_aux[row * D + d] = zs[id.j * pl.ZW + d];
    const float v = aff_base_logp(pl, id, zs, ld_acc);
    if (id.g == 0 && valid) out_main[row] = v;
  } else {
    for (int d = id.g; d < D; d += 4) {
      const float z = zs[id.j * pl.ZW + d];
      ld_acc -= logf(fabsf(zstats[D + d]));
      if (valid) out_main[row * D + d] = (z - zstats[d]) / zstats[D + d];
    }
    float v = ld_acc;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (out_aux && id.g == 0 && valid) out_aux[row] = v;
  }
}

// iid trials: a wave owns 16 thetas (the CONDITION rows); the trials (the flow INPUTS) are walked in blocks of
// MAF_AFF_TC whose states live in the wave's LDS, transforms outermost inside a block: one image staging and one
// context gate per (theta tile, transform, trial block).  Each term runs aff_load_input / aff_transform_fwd /
// aff_base_logp exactly as the paired kernel does, and the terms are added in trial order.
template <int KSH>
__global__ void __launch_bounds__(512)
maf_aff_trials_kernel(const MafAffPlan ap, const float* __restrict__ packed, const float* __restrict__ zstats,
                      const float* __restrict__ x_trials, long long num_trials, const float* __restrict__ theta,
                      long long num_theta, float* __restrict__ out) {
  const MafPlan& mp = ap.m;
  const NsfPlan& pl = mp.n;
  const ShapeDesc& S = pl.shape[0];
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* sc = lds + pl.lds_w_floats + wave * mp.sc_total;
  float* cin = sc + mp.sc_cin;
  float* tz = sc + ap.sc_tz;
  float* tld = sc + ap.sc_tld;
  const long long row = (long long)blockIdx.x * (16 * nw) + 16 * wave + id.j;
  const bool valid = row < num_theta;
  const long long rs = valid ? row : 0;
  const int D = pl.D;
  for (int i = id.lane; i < mp.sc_total; i += 64) sc[i] = 0.f;
  wave_lds_fence();
  aff_load_context(pl, id, zstats, theta + rs * pl.C, valid, cin);
  wave_lds_fence();
  const float* cin_row = cin + id.j * pl.CINW + id.g;
  float total = 0.f;
  for (long long c0 = 0; c0 < num_trials; c0 += MAF_AFF_TC) {
    const int nt = num_trials - c0 < MAF_AFF_TC ? (int)(num_trials - c0) : MAF_AFF_TC;   // uniform over the grid
    for (int i = 0; i < nt; ++i)
      tld[64 * i + id.lane] = aff_load_input(pl, id, zstats, x_trials + (c0 + i) * D, true, tz + i * ap.tz_stride);
    wave_lds_fence();
    for (int t = 0; t < pl.T; ++t) {
      __syncthreads();
      stage_layer(lds, packed + (long long)t * pl.img_floats, pl.img_floats, tid, nthreads);
      __syncthreads();
      f4 gate[NSF_HT];
      made_gate<KSH>(lds, S, id, cin_row + D, gate);
      for (int i = 0; i < nt; ++i) {
        float ld = tld[64 * i + id.lane];
        aff_transform_fwd<KSH>(lds, ap, id, tz + i * ap.tz_stride, cin, gate, ld);
        tld[64 * i + id.lane] = ld;
      }
    }
    for (int i = 0; i < nt; ++i) total += aff_base_logp(pl, id, tz + i * ap.tz_stride, tld[64 * i + id.lane]);
    wave_lds_fence();
  }
  if (id.g == 0 && valid) out[row] = total;
}

// ------------------------------------------------------------------ training: row-parallel backward
// MafBwdArgs as in maf_kernel.h; GP holds TWO m-tile planes (g_u | g_shift of dims 0..15) in fragment order.
// grad_x (optional, (n, C), needs x_rows == n): d loss / d x.  The context enters a transform through its gate only,
// so the contribution is Wc^T gc scaled by the kernel's own z-scoring; the last transform (the first launch)
// overwrites, the others add, always by the lane that owns (row, c): launch order is the summation order.  The
// read-modify-write relies on the host enqueueing the T launches on ONE stream, each after the previous one.
template <int KSH>
__global__ void __launch_bounds__(512)
maf_aff_bwd_kernel(const MafAffPlan ap, const MafBwdArgs a, float* __restrict__ grad_x) {
  const MafPlan& mp = ap.m;
  const NsfPlan& pl = mp.n;
  const ShapeDesc& S = pl.shape[0];
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int wave = tid >> 6, nw = nthreads >> 6;
  const LaneId id = make_lane();
  float* sc = lds + pl.lds_w_floats + wave * mp.sc_total;
  float* cin = sc + mp.sc_cin;
  const int D = pl.D, C = pl.C, NB = pl.NB;
  const long long n = a.n;
  const long long row = (long long)blockIdx.x * (16 * nw) + 16 * wave + id.j;
  const bool valid = row < n;
  const long long rs = valid ? row : 0;
  const float* x_mean = a.zstats + 2 * D;
  const float* x_std = x_mean + C;
  const float wn = valid ? (a.row_w ? a.row_w[rs] : a.uni_w) : 0.f;
  stage_layer(lds, a.packed + (long long)a.t * pl.img_floats, pl.img_floats, tid, nthreads);
  for (int i = id.lane; i < mp.sc_total; i += 64) sc[i] = 0.f;
  __syncthreads();
  float zv[4], gy[4];
  {
    const long long xr = (a.x_rows == n) ? rs : (a.x_rows == 1 ? 0 : rs % a.x_rows);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = 4 * r + id.g;
      zv[r] = 0.f;
      gy[r] = 0.f;
      if (d < D) {
        const float z = valid ? a.z_in[rs * D + d] : 0.f;
        zv[r] = z;
        cin[id.j * pl.CINW + d] = z;
        if (valid) a.CTX[row * MAF_CW + d] = z;
        // undo the permutation on the way back: out[d] = in[perm[d]]  =>  g_in[k] = g_out[iperm[k]]
        const int src = __float_as_int(lds[mp.l_iperm + d]);
        const float g = valid ? a.gz_up[rs * D + src] : 0.f;
        gy[r] = a.is_last ? wn * g : g;
      }
    }
    for (int c = id.g; c < C; c += 4) {
      const float v = ((valid ? a.x[xr * C + c] : 0.f) - x_mean[c]) / x_std[c];
      cin[id.j * pl.CINW + D + c] = v;
      if (valid) a.CTX[row * MAF_CW + D + c] = v;
    }
  }
  wave_lds_fence();
  const float* cin_row = cin + id.j * pl.CINW + id.g;
  // ---- recompute the conditioner (activations stay in registers)
  f4 gate[NSF_HT], h[NSF_HT], hs[MAF_MAX_NB + 1][NSF_HT];
  made_gate<KSH>(lds, S, id, cin_row + D, gate);
  made_hidden<KSH, 0>(lds, pl, S, id, cin_row, gate, h, hs);
#pragma unroll
  for (int b = 0; b <= MAF_MAX_NB; ++b)
    if (b <= NB) store_frag_rows(a.ACT + 64 * b, (MAF_MAX_NB + 1) * MAF_AW, row, valid, id, hs[b]);
  // ---- affine head, forward + reverse mode in registers
  const LinDesc& LF = S.lin[S.fin];
  f4 u, s;
  aff_final<KSH>(lds, LF, id, h, u, s);
  f4 gb[NSF_HT];
  float gx[4];
#pragma unroll
  for (int mt = 0; mt < NSF_HT; ++mt) gb[mt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int d = 4 * r + id.g;
    float sig;
    const float scl = aff_scale(u[r], ap.eps, sig);
    const bool live = d < D;
    // loss = -w log p: d/d(log scale) = -w;  y = scale z + shift
    gb[0][r] = live ? (gy[r] * zv[r] - wn / scl) * sig : 0.f;
    gb[1][r] = live ? gy[r] : 0.f;
    gx[r] = gy[r] * scl;                                    // direct path through the transform's argument
  }
  if (valid) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
      *reinterpret_cast<float4*>(a.GP + (mt * a.npad + row) * 16 + 4 * id.g) =
          float4{gb[mt][0], gb[mt][1], gb[mt][2], gb[mt][3]};
  }
  // g_h = Wf^T [g_u ; g_shift]: the two D fragments ARE the B operand of the transposed GEMM's 8 K-steps
  f4 gh[NSF_HT];
#pragma unroll
  for (int mt = 0; mt < NSF_HT; ++mt) gh[mt] = {0.f, 0.f, 0.f, 0.f};
  gemm_T_breg<8, NSF_HT>(lds, LF, id, gb, gh);
  // ---- back through the feed-forward blocks: G_b = g (1 - h_{b+1}^2), g <- W_b^T G_b
#pragma unroll
  for (int b = MAF_MAX_NB - 1; b >= 0; --b) {
    if (b < NB) {
      f4 gbb[NSF_HT];
#pragma unroll
      for (int mt = 0; mt < NSF_HT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hv = hs[b + 1][mt][r];
          gbb[mt][r] = gh[mt][r] * (1.f - hv * hv);
          gh[mt][r] = 0.f;
        }
      store_frag_planes(a.G + (long long)(4 * (2 + b)) * a.npad * 16, a.npad, row, valid, id, gbb);
      gemm_T_breg<KSH, NSF_HT>(lds, S.lin[2 + b], id, gbb, gh);
    }
  }
  {
    f4 g0[NSF_HT], gc[NSF_HT], gin[1];
#pragma unroll
    for (int mt = 0; mt < NSF_HT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hv = hs[0][mt][r];
        g0[mt][r] = gh[mt][r] * (1.f - hv * hv);          // d / d(W0 z + b0 + gate)
        const float gt = gate[mt][r];
        gc[mt][r] = g0[mt][r] * (1.f - gt * gt);          // d / d(Wc c + bc)
      }
    store_frag_planes(a.G, a.npad, row, valid, id, g0);
    store_frag_planes(a.G + 4 * a.npad * 16, a.npad, row, valid, id, gc);
    gin[0] = {0.f, 0.f, 0.f, 0.f};
    gemm_T_breg<KSH, 1>(lds, S.lin[0], id, g0, gin);     // through the (masked) initial layer: dims < their own
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * r + id.g;
      if (k < D && valid) {
        const float g = gx[r] + gin[0][r];
        if (a.t > 0) a.gz_dn[row * D + k] = g;
        else if (a.grad_theta) a.grad_theta[row * D + k] = g * a.zstats[D + k];
      }
    }
    if (grad_x) {                                         // wave-uniform
      f4 gcx[2];
      gcx[0] = {0.f, 0.f, 0.f, 0.f};
      gcx[1] = {0.f, 0.f, 0.f, 0.f};
      gemm_T_breg<KSH, 2>(lds, S.lin[1], id, gc, gcx);   // slots >= C come back cleared
      if (valid) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 16 * mt + 4 * r + id.g;
            if (c < C) {
              const float v = gcx[mt][r] / x_std[c];
              float* dst = grad_x + row * C + c;
              *dst = a.is_last ? v : *dst + v;
            }
          }
      }
    }
  }
}
