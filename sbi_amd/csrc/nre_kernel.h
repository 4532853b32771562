// nre_kernel.h -- device side of the NRE ratio classifier (csrc/nre.hip).
//
// The network is sbi's build_resnet_classifier (sbi/neural_nets/net_builders/classifier.py:172-235): z-scored theta and
// x, concatenated [z_theta ; z_x], through nflows' ResidualNet(in = D + C, out = 1, hidden H, no context, NB blocks,
// relu).  One lane evaluates one (theta, x) pair: the residual stream h and the block's hidden pre-activation u
// live in registers (HP = H rounded up to 16, or 56 for H = 49 ... 56; fully unrolled); the weights are read at
// wave-uniform addresses from the packed image (scalar loads through the constant cache: every lane of a wave
// multiplies its own activations by the same weight), so no LDS staging and no cross-lane traffic is needed on the per-pair paths.
//
// Packed image (nre_pk_* offsets, floats; rows beyond H are zero, so the unrolled loops over HP need no guards):
//   b_init [HP] | W_init^T x-columns [C][HP] | W_init^T theta-columns [D][HP]
//   per block b, per linear i in {0, 1}: W^T [HP][HP] (W^T[j][i] = W[i][j]) | bias [HP]
//   w_final [HP] | b_final [1]
// The transposed storage serves both directions: the forward reads row j of W^T to add W[:, j] * a_j, the backward reads
// the same row to form (W^T g)_j.
//
// Training stash (feature-major per 256-pair tile, nre_st_base: a wave's stores are coalesced):
//   z (D + C: theta then x, standardized) | h_b (b = 0 .. NB, H each) | u_b (b < NB, H each)
//   | g_init (H) | g_lin0_b (b < NB, H each) | g_lin1_b (b < NB, H each)
// followed by the weight-gradient partials (one flat gradient per row chunk).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct NreDims {
  int D, C, H, NB;
  int HS;   // features per stashed activation / gradient: H rounded up to the kernels' padded width HP
};

// The weight image and the z-score statistics are read through the constant address space: loads there at
// wave-uniform addresses become scalar loads even in the kernels that also store (the training stash), where the
// compiler cannot prove a global-memory load unclobbered by the stores in front of it.
// The weight image and the z-score statistics are read through the constant address space: loads there at
// wave-uniform addresses are scalar loads even in the kernels that also store (the training stash), where the compiler
// cannot prove a global-memory load unclobbered by the stores in front of it.
typedef const float __attribute__((address_space(4))) nre_cfloat;
__device__ inline const nre_cfloat* nre_const(const float* p) { return (const nre_cfloat*)p; }

template <int HP>
__host__ __device__ inline int64_t nre_pk_blk(const NreDims& d, int b, int lin) {
  return (int64_t)HP * (1 + d.C + d.D) + (int64_t)(2 * b + lin) * (HP * HP + HP);
}
template <int HP>
__host__ __device__ inline int64_t nre_pk_final(const NreDims& d) {
  return (int64_t)HP * (1 + d.C + d.D) + (int64_t)2 * d.NB * (HP * HP + HP);
}

// stash rows (units of n floats)
// (activations and gradients are stored at the padded width HS = HP, padding included: no per-feature guards)
__host__ __device__ inline int64_t nre_st_h(const NreDims& d, int b) { return d.D + d.C + (int64_t)b * d.HS; }
__host__ __device__ inline int64_t nre_st_u(const NreDims& d, int b) {
  return d.D + d.C + (int64_t)(d.NB + 1) * d.HS + (int64_t)b * d.HS;
}
__host__ __device__ inline int64_t nre_st_g0(const NreDims& d) { return d.D + d.C + (int64_t)(2 * d.NB + 1) * d.HS; }
__host__ __device__ inline int64_t nre_st_gl(const NreDims& d, int b, int lin) {
  return nre_st_g0(d) + d.HS + (int64_t)(lin * d.NB + b) * d.HS;
}
__host__ __device__ inline int64_t nre_st_rows(const NreDims& d) { return d.D + d.C + (int64_t)(4 * d.NB + 2) * d.HS; }
// tile-major: the pairs of one 256-pair tile keep their features together, feature k of pair r at
// nre_st_base(d, r) + 256 k -- every per-feature offset is a compile-time constant, not a 64-bit k * n held in SGPRs
__host__ __device__ inline int64_t nre_st_base(const NreDims& d, int64_t r) {
  return (r >> 8) * nre_st_rows(d) * 256 + (r & 255);
}
__host__ __device__ inline int64_t nre_st_floats(const NreDims& d, int64_t n) { return (n + 255) / 256 * 256 * nre_st_rows(d); }

// Forward pass of pair r.  theta row = r / theta_div (1: paired; num_trials: the trials layout), x row = r % x_rows.
// FOLD (inference with one x): W_x z_x + b was computed once per workgroup into LDS by the same fma sequence the
// per-lane path runs, so both give identical bits.  TRAIN: the activations go to the stash.
template <int HP, bool TRAIN, bool FOLD>
__global__ void __launch_bounds__(256)
nre_forward_kernel(NreDims d, const float* __restrict__ pk_, const float* __restrict__ zs_,
                   const float* __restrict__ theta, const float* __restrict__ x, int64_t n, int64_t x_rows,
                   int64_t theta_div, float* __restrict__ logit_out, float* __restrict__ ws) {
  const nre_cfloat* pk = nre_const(pk_);
  const nre_cfloat* zs = nre_const(zs_);
  __shared__ float cx[HP];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const nre_cfloat* WxT = pk + HP;
  const nre_cfloat* WtT = pk + HP + (int64_t)d.C * HP;
  if constexpr (FOLD) {
    if (threadIdx.x < HP) {
      float a = pk[threadIdx.x];
      for (int k = 0; k < d.C; ++k) {
        const float z = (x[k] - zs[2 * d.D + k]) / zs[2 * d.D + d.C + k];
        a = fmaf(WxT[k * HP + threadIdx.x], z, a);
      }
      cx[threadIdx.x] = a;
    }
    __syncthreads();
  }
  if (r >= n) return;
  float* wsr = TRAIN ? ws + nre_st_base(d, r) : nullptr;
  float h[HP];
  if constexpr (FOLD) {
#pragma unroll
    for (int i = 0; i < HP; ++i) h[i] = cx[i];
  } else {
#pragma unroll
    for (int i = 0; i < HP; ++i) h[i] = pk[i];
    const float* xr = x + (n <= 0x7fffffff ? (int64_t)((uint32_t)r % (uint32_t)x_rows) : r % x_rows) * d.C;
    for (int k = 0; k < d.C; ++k) {
      const float z = (xr[k] - zs[2 * d.D + k]) / zs[2 * d.D + d.C + k];
      if constexpr (TRAIN) wsr[(d.D + k) * 256] = z;
      #pragma unroll
      for (int i = 0; i < HP; ++i) h[i] = fmaf((WxT + k * HP)[i], z, h[i]);
    }
  }
  const float* tr = theta + (n <= 0x7fffffff ? (int64_t)((uint32_t)r / (uint32_t)theta_div) : r / theta_div) * d.D;
  for (int k = 0; k < d.D; ++k) {
    const float z = (tr[k] - zs[k]) / zs[d.D + k];
    if constexpr (TRAIN) wsr[k * 256] = z;
    #pragma unroll
    for (int i = 0; i < HP; ++i) h[i] = fmaf((WtT + k * HP)[i], z, h[i]);
  }
  for (int b = 0; b < d.NB; ++b) {
    const nre_cfloat* L0 = pk + nre_pk_blk<HP>(d, b, 0);
    const nre_cfloat* L1 = pk + nre_pk_blk<HP>(d, b, 1);
    if constexpr (TRAIN) {
      float* st = wsr + nre_st_h(d, b) * 256;
#pragma unroll
      for (int i = 0; i < HP; ++i)
        st[i * 256] = h[i];
    }
    float u[HP];
#pragma unroll
    for (int i = 0; i < HP; ++i) u[i] = L0[HP * HP + i];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const float a = h[j] > 0.f ? h[j] : 0.f;
      #pragma unroll
      for (int i = 0; i < HP; ++i) u[i] = fmaf((L0 + j * HP)[i], a, u[i]);
    }
    if constexpr (TRAIN) {
      float* st = wsr + nre_st_u(d, b) * 256;
#pragma unroll
      for (int i = 0; i < HP; ++i)
        st[i * 256] = u[i];
    }
    // the block output is accumulated straight into the residual stream (bias first): h and u are the only live
    // arrays
#pragma unroll
    for (int i = 0; i < HP; ++i) h[i] += L1[HP * HP + i];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const float c = u[j] > 0.f ? u[j] : 0.f;
      #pragma unroll
      for (int i = 0; i < HP; ++i) h[i] = fmaf((L1 + j * HP)[i], c, h[i]);
    }
  }
  const nre_cfloat* F = pk + nre_pk_final<HP>(d);
  if constexpr (TRAIN) {
    float* st = wsr + nre_st_h(d, d.NB) * 256;
#pragma unroll
    for (int i = 0; i < HP; ++i)
      if (i < d.H) st[i * 256] = h[i];
  }
  float lg = 0.f;
#pragma unroll
  for (int i = 0; i < HP; ++i) lg = fmaf(F[i], h[i], lg);
  logit_out[r] = lg + F[HP];
}

// Backward pass of pair r from its upstream weight w[r] = d loss / d logit_r: the per-layer output gradients go to the
// stash (the weight gradients are reduced from there by nre_dw_kernel), grad_theta (optional) = w d logit / d theta.
template <int HP>
__global__ void __launch_bounds__(256)
nre_backward_kernel(NreDims d, const float* __restrict__ pk_, const float* __restrict__ zs_, int64_t n,
                    const float* __restrict__ w, float* __restrict__ grad_theta, float* __restrict__ ws) {
  const nre_cfloat* pk = nre_const(pk_);
  const nre_cfloat* zs = nre_const(zs_);
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  float* wsr = ws + nre_st_base(d, r);
  const nre_cfloat* F = pk + nre_pk_final<HP>(d);
  const float wr = w[r];
  float g[HP];
#pragma unroll
  for (int i = 0; i < HP; ++i) g[i] = wr * F[i];
  for (int b = d.NB - 1; b >= 0; --b) {
    const nre_cfloat* L0 = pk + nre_pk_blk<HP>(d, b, 0);
    const nre_cfloat* L1 = pk + nre_pk_blk<HP>(d, b, 1);
    {
      float* st = wsr + nre_st_gl(d, b, 1) * 256;
#pragma unroll
      for (int i = 0; i < HP; ++i)
        st[i * 256] = g[i];
    }
    float du[HP];
    const float* us = wsr + nre_st_u(d, b) * 256;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      float acc = 0.f;
      #pragma unroll
      for (int i = 0; i < HP; ++i) acc = fmaf((L1 + j * HP)[i], g[i], acc);
      const float uj = j < d.H ? us[j * 256] : 0.f;
      du[j] = uj > 0.f ? acc : 0.f;
    }
    {
      float* st = wsr + nre_st_gl(d, b, 0) * 256;
#pragma unroll
      for (int i = 0; i < HP; ++i)
        st[i * 256] = du[i];
    }
    const float* hs = wsr + nre_st_h(d, b) * 256;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      float acc = 0.f;
      #pragma unroll
      for (int i = 0; i < HP; ++i) acc = fmaf((L0 + j * HP)[i], du[i], acc);
      const float hj = j < d.H ? hs[j * 256] : 0.f;
      g[j] += hj > 0.f ? acc : 0.f;
    }
  }
  {
    float* st = wsr + nre_st_g0(d) * 256;
#pragma unroll
    for (int i = 0; i < HP; ++i)
      if (i < d.H) st[i * 256] = g[i];
  }
  if (grad_theta) {
    const nre_cfloat* WtT = pk + HP + (int64_t)d.C * HP;
    for (int k = 0; k < d.D; ++k) {
      float acc = 0.f;
      #pragma unroll
      for (int i = 0; i < HP; ++i) acc = fmaf((WtT + k * HP)[i], g[i], acc);
      grad_theta[r * d.D + k] = acc / zs[d.D + k];
    }
  }
}

// The logit of ONE pair in two halves, for a lane that keeps its x: nre_x_part is W_x z_x + b (the first half of
// nre_forward_kernel<HP, false, false>'s chain, in the same order), nre_logit_from_x_part continues from a copy of it with
// the theta columns, the blocks and the final layer -- the same fma sequence, identical bits.
template <int HP>
__device__ __forceinline__ void nre_x_part(const NreDims& d, const nre_cfloat* pk, const nre_cfloat* zs,
                                           const float* __restrict__ xr, float (&hx)[HP]) {
  const nre_cfloat* WxT = pk + HP;
#pragma unroll
  for (int i = 0; i < HP; ++i) hx[i] = pk[i];
  for (int k = 0; k < d.C; ++k) {
    const float z = (xr[k] - zs[2 * d.D + k]) / zs[2 * d.D + d.C + k];
#pragma unroll
    for (int i = 0; i < HP; ++i) hx[i] = fmaf((WxT + k * HP)[i], z, hx[i]);
  }
}

template <int HP>
__device__ __forceinline__ float nre_logit_from_x_part(const NreDims& d, const nre_cfloat* pk, const nre_cfloat* zs,
                                                       const float* tr, const float (&hx)[HP]) {
  const nre_cfloat* WtT = pk + HP + (int64_t)d.C * HP;
  float h[HP];
#pragma unroll
  for (int i = 0; i < HP; ++i) h[i] = hx[i];
  for (int k = 0; k < d.D; ++k) {
    const float z = (tr[k] - zs[k]) / zs[d.D + k];
#pragma unroll
    for (int i = 0; i < HP; ++i) h[i] = fmaf((WtT + k * HP)[i], z, h[i]);
  }
  for (int b = 0; b < d.NB; ++b) {
    const nre_cfloat* L0 = pk + nre_pk_blk<HP>(d, b, 0);
    const nre_cfloat* L1 = pk + nre_pk_blk<HP>(d, b, 1);
    float u[HP];
#pragma unroll
    for (int i = 0; i < HP; ++i) u[i] = L0[HP * HP + i];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const float a = h[j] > 0.f ? h[j] : 0.f;
#pragma unroll
      for (int i = 0; i < HP; ++i) u[i] = fmaf((L0 + j * HP)[i], a, u[i]);
    }
#pragma unroll
    for (int i = 0; i < HP; ++i) h[i] += L1[HP * HP + i];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const float c = u[j] > 0.f ? u[j] : 0.f;
#pragma unroll
      for (int i = 0; i < HP; ++i) h[i] = fmaf((L1 + j * HP)[i], c, h[i]);
    }
  }
  const nre_cfloat* F = pk + nre_pk_final<HP>(d);
  float lg = 0.f;
#pragma unroll
  for (int i = 0; i < HP; ++i) lg = fmaf(F[i], h[i], lg);
  return lg + F[HP];
}
