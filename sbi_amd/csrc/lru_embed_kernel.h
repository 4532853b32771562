// lru_embed_kernel.h -- the recurrent stack of LRUEmbedding on gfx950: plan, device functions, kernels (launchers:
// lru_embed.hip).  Contract: include/sbi_amd_lru.h.
//
// Execution model
//   * one launch per block.  A workgroup is 4 waves and owns whole sequences: b = group, group + G, ...  The block's
//     weights are staged once per workgroup in LDS, already in the form the GEMMs want: lambda (re, im), gamma B as a
//     real (2 S2, H) matrix with rows (re, im) of every state, C as a real (H, 2 S2) matrix with columns (re, -im), D,
//     the gate.  The sequence is walked in tiles of 16 time steps; the block-to-block maps (B, T, H) go through global
//     memory (they do not fit LDS for long T), everything else of a tile stays in LDS.
//   * every GEMM is lr_gemm on v_mfma_f32_16x16x4_f32: a wave owns 16 x 16 output tiles, operands are read from LDS with
//     guarded loads (an element outside M, N or K is an exact 0, never a stale value), so no buffer needs padding.
//   * the scan: lane s carries the complex state of s in registers across the tiles and runs one sequential fma chain
//     over the tile's steps.  The reversed-direction states of a bidirectional block are needed at the same t as the
//     forward ones: sweep 1 runs them first, in descending time, into the workspace; sweep 2 walks forward.
//   * backward (LR_BWD): sweep 2 also carries the gradient through gate, GELU and C to the states (DX), accumulates
//     dgate, dD and dC, and runs the reversed half's adjoint (it ascends); sweep 3 descends with the forward half's
//     adjoint.  Both add A^T u onto d(gamma B) and A (gamma B) onto the gradient of the block input, which replaces the
//     incoming gradient map in place.  In block 0 sweep 3 also forms the input layer's gradient.  Weight gradients
//     accumulate on the workgroup's own row of the partial buffer (read-modify-write by the one lane that owns the
//     element, L2 resident); lr_reduce_kernel adds the rows in workgroup order and lr_chain_kernel applies the chain
//     rules into log_nu, log_theta, log_gamma and B.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_lru.h"
#include "../../include/sbi_amd_nsf.h"

namespace {

#define LR_THREADS 256
#define LR_WAVES 4
#define LR_TT 16                    // time steps of a tile
#define LR_GROUPS 512               // most workgroups of a launch: sequences beyond walk the grid again
#define LR_LDS_BUDGET (160 * 1024)
#define LR_MAX_T 65535
#define LR_MAX_BLOCKS 8

typedef float lr_f4 __attribute__((ext_vector_type(4)));

struct LrPlan {
  int I, H, S, S2, W2, NB, bidir, agg;
  int P, PB, off_blk0;                               // flat parameters: all, one block, first block's offset
  int p_nu, p_th, p_B, p_C, p_D, p_lg, p_Wg, p_bg;   // offsets inside a block's parameters
  // LDS offsets (floats)
  int o_lam, o_gB, o_Cm, o_D, o_Wg, o_bg, o_U, o_X, o_Y0, o_Y1, o_SG, o_DX, o_GO, o_DZ, o_G, o_XI;
  long long fwd_floats, bwd_floats;
};

static int lr_plan_sizes(const sbi_amd_lru_config* cfg, LrPlan* out) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->input_dim < 1 || cfg->hidden_dim < 1 || cfg->state_dim < 1 || cfg->num_blocks < 1) return SBI_AMD_E_BADARG;
  if (cfg->bidirectional < 0 || cfg->bidirectional > 1) return SBI_AMD_E_BADARG;
  if (cfg->aggregation < 0 || cfg->aggregation > 1) return SBI_AMD_E_UNSUPPORTED;
  if (cfg->state_dim > 128) return SBI_AMD_E_UNSUPPORTED;
  const int S2 = cfg->state_dim * (cfg->bidirectional ? 2 : 1);
  if (cfg->input_dim > 64 || cfg->hidden_dim > 128 || S2 > 128 || cfg->num_blocks > LR_MAX_BLOCKS)
    return SBI_AMD_E_UNSUPPORTED;
  LrPlan p = {};
  p.I = cfg->input_dim; p.H = cfg->hidden_dim; p.S = cfg->state_dim; p.S2 = S2; p.W2 = 2 * S2;
  p.NB = cfg->num_blocks; p.bidir = cfg->bidirectional; p.agg = cfg->aggregation;
  const int H = p.H, W2 = p.W2;
  p.p_nu = 0; p.p_th = S2; p.p_B = 2 * S2; p.p_C = p.p_B + W2 * H; p.p_D = p.p_C + W2 * H; p.p_lg = p.p_D + H;
  p.p_Wg = p.p_lg + S2; p.p_bg = p.p_Wg + H * H; p.PB = p.p_bg + H;
  p.off_blk0 = H * p.I + H;
  p.P = p.off_blk0 + p.NB * p.PB;
  int o = 0;
  p.o_lam = o; o += W2;
  p.o_gB = o; o += W2 * H;
  p.o_Cm = o; o += W2 * H;
  p.o_D = o; o += H;
  p.o_Wg = o; o += H * H;
  p.o_bg = o; o += H;
  p.o_U = o; o += LR_TT * H;
  p.o_X = o; o += (LR_TT + 2) * W2;
  p.o_Y0 = o; o += LR_TT * H;
  p.o_Y1 = o; o += LR_TT * H;
  p.o_SG = o; o += LR_TT * H;
  p.fwd_floats = o;
  p.o_DX = o; o += LR_TT * W2;
  p.o_GO = o; o += LR_TT * H;
  p.o_DZ = o; o += LR_TT * H;
  p.o_G = o; o += LR_TT * H;
  p.o_XI = o; o += LR_TT * p.I;
  p.bwd_floats = o;
  *out = p;
  return 0;
}

static int lr_check_rows(int64_t B, int64_t T) {
  if (B < 1 || T < 1) return SBI_AMD_E_BADARG;
  if (T > LR_MAX_T || B > (((1ll << 31) - 64) / T) || B * T >= (1ll << 31) - 64) return SBI_AMD_E_UNSUPPORTED;
  return 0;
}

static int lr_build_plan(const sbi_amd_lru_config* cfg, LrPlan* out) {
  const int rc = lr_plan_sizes(cfg, out);
  if (rc) return rc;
  return out->bwd_floats * 4 <= LR_LDS_BUDGET ? 0 : SBI_AMD_E_LDS;
}

static int lr_groups(int64_t B) { return (int)(B < LR_GROUPS ? B : LR_GROUPS); }

struct LrArgs {
  const float* params;     // the flat image
  const float* x;          // (B, T, I)
  const float* in;         // this block's input map (B, T, H)
  float* out;              // the next block's input map (forward, not the last block)
  float* features;         // (B, H) (forward, last block)
  float* xs;               // (B, T, 2 S2) states
  float* dxs;              // (B, T, 2 S2) state gradients of the forward half (backward)
  float* gmap;             // (B, T, H) gradient of the block's output, replaced by that of its input (backward)
  const float* gfeat;      // (B, H) (backward, last block)
  float* partial;          // (G, P) (backward)
  int B, T, blk;
};

// C[m cm + n cn] (+)= sum_k A[m am + k ak] Bm[k bk + n bn] for m < M, n < N, k < K on 16x16x4 MFMA tiles; tile
// (mt, nt) belongs to wave (mt Nt + nt) mod 4, so every element has one owner lane whatever the call.
// MFMA operand layout: lane l gives A[m = l % 16][k = l / 16] and B[k = l / 16][n = l % 16]; D[4 (l / 16) + i][l % 16].
template <bool ACC>
__device__ __forceinline__ void lr_gemm(const float* A, int am, int ak, const float* Bm, int bk, int bn, float* C,
                                        int cm, int cn, int M, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int Nt = (N + 15) >> 4, tiles = ((M + 15) >> 4) * Nt;
  for (int tile = wave; tile < tiles; tile += LR_WAVES) {
    const int m0 = (tile / Nt) << 4, n0 = (tile % Nt) << 4;
    const int m = m0 + c, n = n0 + c;
    const bool m_ok = m < M, n_ok = n < N;
    const float* pa = A + m * am;
    const float* pb = Bm + n * bn;
    lr_f4 d = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + q;
      const bool k_ok = k < K;
      const float a = (m_ok && k_ok) ? pa[k * ak] : 0.f;
      const float b = (n_ok && k_ok) ? pb[k * bk] : 0.f;
      d = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d, 0, 0, 0);
    }
    if (n_ok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mm = m0 + 4 * q + i;
        if (mm < M) {
          float* pc = C + mm * cm + n * cn;
          if (ACC) *pc += d[i]; else *pc = d[i];
        }
      }
    }
  }
}

__device__ __forceinline__ float lr_gelu(float y) { return 0.5f * y * (1.f + erff(y * 0.70710678118654752440f)); }
__device__ __forceinline__ float lr_dgelu(float y) {
  return 0.5f * (1.f + erff(y * 0.70710678118654752440f)) + y * 0.39894228040143267794f * expf(-0.5f * y * y);
}
__device__ __forceinline__ float lr_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// h0 (rows, H) = x (rows, I) W^T + b: the input layer, one thread per output element
__global__ void __launch_bounds__(256)
lr_input_kernel(const float* __restrict__ params, const float* __restrict__ x, float* __restrict__ h0, long long rows,
                int I, int H) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * H) return;
  const long long row = e / H;
  const int h = (int)(e - row * H);
  const float* w = params + h * I;
  const float* xr = x + row * I;
  float acc = params[H * I + h];
  for (int i = 0; i < I; ++i) acc = fmaf(xr[i], w[i], acc);
  h0[e] = acc;
}

// stage the block's weights in the form the GEMMs want
__device__ __forceinline__ void lr_stage(const LrPlan& pl, float* lds, const float* bp, int tid) {
  const int H = pl.H, S2 = pl.S2, W2 = pl.W2;
  for (int s = tid; s < S2; s += LR_THREADS) {
    const float r = expf(-expf(bp[pl.p_nu + s]));
    float sn, cs;
    sincosf(expf(bp[pl.p_th + s]), &sn, &cs);
    lds[pl.o_lam + 2 * s] = r * cs;
    lds[pl.o_lam + 2 * s + 1] = r * sn;
  }
  for (int e = tid; e < W2 * H; e += LR_THREADS) {
    // gamma B: parameter (s, h, c) -> row 2 s + c, column h
    const int s = e / (2 * H), rem = e - s * 2 * H, h = rem >> 1, c = rem & 1;
    lds[pl.o_gB + (2 * s + c) * H + h] = expf(bp[pl.p_lg + s]) * bp[pl.p_B + e];
    // C: parameter (h, s, c) -> row h, column 2 s + c, the imaginary part negated (y = Re(C x))
    const float v = bp[pl.p_C + e];
    lds[pl.o_Cm + e] = (e & 1) ? -v : v;
  }
  for (int e = tid; e < H * H; e += LR_THREADS) lds[pl.o_Wg + e] = bp[pl.p_Wg + e];
  for (int h = tid; h < H; h += LR_THREADS) {
    lds[pl.o_D + h] = bp[pl.p_D + h];
    lds[pl.o_bg + h] = bp[pl.p_bg + h];
  }
}

// rows x cols of a global (.., ld) map -> a 16-row LDS tile of row stride lds_ld, rows beyond `rows` zeroed
__device__ __forceinline__ void lr_load_tile(float* dst, int lds_ld, const float* src, long long ld, int rows, int cols,
                                             int tid) {
  for (int e = tid; e < LR_TT * cols; e += LR_THREADS) {
    const int r = e / cols, c = e - r * cols;
    dst[r * lds_ld + c] = r < rows ? src[r * ld + c] : 0.f;
  }
}

template <bool BWD>
__global__ void __launch_bounds__(LR_THREADS) lr_block_kernel(LrPlan pl, LrArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int H = pl.H, S = pl.S, W2 = pl.W2, I = pl.I, T = a.T;
  const bool first = a.blk == 0, last = a.blk == pl.NB - 1, bidir = pl.bidir != 0;
  const float* bp = a.params + pl.off_blk0 + (long long)a.blk * pl.PB;
  lr_stage(pl, lds, bp, tid);
  const float* lam = lds + pl.o_lam;
  const float* gB = lds + pl.o_gB;
  const float* Cm = lds + pl.o_Cm;
  const float* Dv = lds + pl.o_D;
  const float* Wg = lds + pl.o_Wg;
  const float* bg = lds + pl.o_bg;
  float* U = lds + pl.o_U;
  float* X = lds + pl.o_X;              // row r + 1 holds step t0 + r; rows 0 and 17 are the halo steps
  float* Y0 = lds + pl.o_Y0;
  float* Y1 = lds + pl.o_Y1;
  float* SG = lds + pl.o_SG;
  float* DX = lds + pl.o_DX;
  float* GO = lds + pl.o_GO;
  float* DZ = lds + pl.o_DZ;
  float* Gt = lds + pl.o_G;
  float* XI = lds + pl.o_XI;
  const int nT = (T + LR_TT - 1) / LR_TT;
  const int RV = 2 * S;                 // first column of the reversed half
  const bool lane_s = tid < S;          // this thread carries state tid (and S + tid)
  float* pb = nullptr;                 // this workgroup's partial gradient of the block
  float* pin = nullptr;                 // ... of the input layer
  if (BWD) {
    pin = a.partial + (long long)blockIdx.x * pl.P;
    pb = pin + pl.off_blk0 + (long long)a.blk * pl.PB;
    for (int e = tid; e < pl.PB; e += LR_THREADS) pb[e] = 0.f;
    if (first)
      for (int e = tid; e < pl.off_blk0; e += LR_THREADS) pin[e] = 0.f;
  }
  __syncthreads();
  float lr_ = 0.f, li_ = 0.f, rr_ = 0.f, ri_ = 0.f;     // lambda of state tid and of state S + tid
  if (lane_s) {
    lr_ = lam[2 * tid]; li_ = lam[2 * tid + 1];
    if (bidir) { rr_ = lam[RV + 2 * tid]; ri_ = lam[RV + 2 * tid + 1]; }
  }

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const long long row0 = (long long)b * T;
    const float* in = a.in + row0 * H;
    float* xs = a.xs + row0 * W2;

    // ---- sweep 1: the reversed half, descending ----------------------------------------------------------------------
    if (bidir) {
      float xr = 0.f, xi = 0.f;
      for (int k = nT - 1; k >= 0; --k) {
        const int t0 = k * LR_TT, rows = min(LR_TT, T - t0);
        lr_load_tile(U, H, in + (long long)t0 * H, H, rows, H, tid);
        __syncthreads();
        lr_gemm<false>(U, H, 1, gB + RV * H, 1, H, X + W2 + RV, W2, 1, LR_TT, RV, H);
        __syncthreads();
        if (lane_s) {
          for (int r = rows - 1; r >= 0; --r) {
            const float* v = X + (r + 1) * W2 + RV + 2 * tid;
            const float nr = rr_ * xr - ri_ * xi + v[0], ni = rr_ * xi + ri_ * xr + v[1];
            xr = nr; xi = ni;
            float* o = xs + (long long)(t0 + r) * W2 + RV + 2 * tid;
            o[0] = xr; o[1] = xi;
          }
        }
        __syncthreads();
      }
    }

    // ---- sweep 2: ascending ------------------------------------------------------------------------------------------
    float xr = 0.f, xi = 0.f;           // forward state
    float ar = 0.f, ai = 0.f;           // adjoint of the reversed half (ascends)
    float dlr = 0.f, dli = 0.f;         // d lambda of the reversed half
    float agg = 0.f;                    // running sum over t of out[., tid]
    for (int k = 0; k < nT; ++k) {
      const int t0 = k * LR_TT, rows = min(LR_TT, T - t0);
      lr_load_tile(U, H, in + (long long)t0 * H, H, rows, H, tid);
      if (bidir) {
        // reversed states of steps t0 .. t0 + 16 (the last one is the halo the adjoint needs), 0 beyond T
        for (int e = tid; e < (LR_TT + 1) * RV; e += LR_THREADS) {
          const int r = e / RV, c = e - r * RV;
          X[(r + 1) * W2 + RV + c] = t0 + r < T ? xs[(long long)(t0 + r) * W2 + RV + c] : 0.f;
        }
      }
      if (BWD) {
        if (last) {
          for (int e = tid; e < LR_TT * H; e += LR_THREADS) {
            const int r = e / H, h = e - r * H;
            const float g = a.gfeat[(long long)b * H + h];
            GO[e] = r >= rows ? 0.f : pl.agg == 0 ? g / (float)T : (t0 + r == T - 1 ? g : 0.f);
          }
        } else {
          lr_load_tile(GO, H, a.gmap + (row0 + t0) * H, H, rows, H, tid);
        }
      }
      __syncthreads();
      lr_gemm<false>(U, H, 1, gB, 1, H, X + W2, W2, 1, LR_TT, RV, H);
      __syncthreads();
      if (lane_s) {
        for (int r = 0; r < rows; ++r) {
          float* v = X + (r + 1) * W2 + 2 * tid;
          const float nr = lr_ * xr - li_ * xi + v[0], ni = lr_ * xi + li_ * xr + v[1];
          xr = nr; xi = ni;
          v[0] = xr; v[1] = xi;
          if (BWD) {
            float* o = xs + (long long)(t0 + r) * W2 + 2 * tid;
            o[0] = xr; o[1] = xi;
          }
        }
      }
      __syncthreads();
      lr_gemm<false>(X + W2, W2, 1, Cm, 1, W2, Y0, H, 1, LR_TT, H, W2);
      __syncthreads();
      for (int e = tid; e < LR_TT * H; e += LR_THREADS) {
        const int h = e % H;
        const float y0 = Y0[e] + Dv[h] * U[e];
        Y0[e] = y0;
        Y1[e] = lr_gelu(y0);
      }
      __syncthreads();
      lr_gemm<false>(Y1, H, 1, Wg, 1, H, SG, H, 1, LR_TT, H, H);
      __syncthreads();
      if (!BWD) {
        for (int e = tid; e < LR_TT * H; e += LR_THREADS) {
          const int r = e / H, h = e - r * H;
          const float o = Y1[e] * lr_sigmoid(SG[e] + bg[h]) + U[e];
          if (last) Y0[e] = o;
          else if (r < rows) a.out[(row0 + t0 + r) * H + h] = o;
        }
        if (last) {
          __syncthreads();
          if (tid < H) {
            if (pl.agg == 0) {
              for (int r = 0; r < rows; ++r) agg += Y0[r * H + tid];
            } else if (k == nT - 1) {
              agg = Y0[(rows - 1) * H + tid];
            }
          }
        }
        __syncthreads();
        continue;
      }
      // ---- backward through the gate, GELU and C ----
      for (int e = tid; e < LR_TT * H; e += LR_THREADS) {
        const int h = e % H;
        const float s = lr_sigmoid(SG[e] + bg[h]);
        SG[e] = s;
        DZ[e] = GO[e] * Y1[e] * s * (1.f - s);
      }
      __syncthreads();
      lr_gemm<false>(DZ, H, 1, Wg, H, 1, Gt, H, 1, LR_TT, H, H);              // dz W
      lr_gemm<true>(DZ, 1, H, Y1, H, 1, pb + pl.p_Wg, H, 1, H, H, LR_TT);     // dW += dz^T a
      if (tid < H) {
        float acc = 0.f;
        for (int r = 0; r < LR_TT; ++r) acc += DZ[r * H + tid];
        pb[pl.p_bg + tid] += acc;
      }
      __syncthreads();
      for (int e = tid; e < LR_TT * H; e += LR_THREADS) {
        const int h = e % H;
        const float go = GO[e];
        const float g = (Gt[e] + go * SG[e]) * lr_dgelu(Y0[e]);
        Gt[e] = g;
        GO[e] = go + Dv[h] * g;                                                // the skip and D
      }
      __syncthreads();
      if (tid < H) {
        float acc = 0.f;
        for (int r = 0; r < LR_TT; ++r) acc += Gt[r * H + tid] * U[r * H + tid];
        pb[pl.p_D + tid] += acc;
      }
      lr_gemm<true>(Gt, 1, H, X + W2, W2, 1, pb + pl.p_C, W2, 1, H, W2, LR_TT);   // dC += g^T x
      lr_gemm<false>(Gt, H, 1, Cm, W2, 1, DX, W2, 1, LR_TT, W2, H);              // dx = g C
      __syncthreads();
      {
        float* dxs = a.dxs + (row0 + t0) * W2;
        for (int e = tid; e < rows * RV; e += LR_THREADS) {
          const int r = e / RV, c = e - r * RV;
          dxs[(long long)r * W2 + c] = DX[r * W2 + c];
        }
      }
      if (bidir) {
        if (lane_s) {
          for (int r = 0; r < rows; ++r) {
            float* d = DX + r * W2 + RV + 2 * tid;
            const float nr = d[0] + rr_ * ar + ri_ * ai, ni = d[1] + rr_ * ai - ri_ * ar;   // conj(lambda) a
            ar = nr; ai = ni;
            d[0] = ar; d[1] = ai;
            const float* xp = X + (r + 2) * W2 + RV + 2 * tid;                              // x of step t + 1
            dlr += ar * xp[0] + ai * xp[1];
            dli += ai * xp[0] - ar * xp[1];
          }
        }
        __syncthreads();
        lr_gemm<true>(DX + RV, 1, W2, U, H, 1, pb + pl.p_B + RV * H, H, 1, RV, H, LR_TT);   // d(gamma B) += a^T u
        lr_gemm<true>(DX + RV, W2, 1, gB + RV * H, H, 1, GO, H, 1, LR_TT, H, RV);           // du += a (gamma B)
      }
      __syncthreads();
      for (int e = tid; e < rows * H; e += LR_THREADS) a.gmap[(row0 + t0) * H + e] = GO[e];
      __syncthreads();
    }
    if (!BWD) {
      if (last && tid < H) a.features[(long long)b * H + tid] = pl.agg == 0 ? agg / (float)T : agg;
      continue;
    }
    if (bidir && lane_s) {
      pb[pl.p_nu + S + tid] += dlr;
      pb[pl.p_th + S + tid] += dli;
    }

    // ---- sweep 3: the forward half's adjoint, descending -------------------------------------------------------------
    ar = 0.f; ai = 0.f; dlr = 0.f; dli = 0.f;
    for (int k = nT - 1; k >= 0; --k) {
      const int t0 = k * LR_TT, rows = min(LR_TT, T - t0);
      lr_load_tile(U, H, in + (long long)t0 * H, H, rows, H, tid);
      lr_load_tile(GO, H, a.gmap + (row0 + t0) * H, H, rows, H, tid);
      if (first) lr_load_tile(XI, I, a.x + (row0 + t0) * I, I, rows, I, tid);
      for (int e = tid; e < LR_TT * RV; e += LR_THREADS) {
        const int r = e / RV, c = e - r * RV;
        DX[r * W2 + c] = r < rows ? a.dxs[(row0 + t0 + r) * W2 + c] : 0.f;
        const int tp = t0 + r - 1;                                             // X row r: the step before t0 + r
        X[r * W2 + c] = (tp >= 0 && r < rows) ? xs[(long long)tp * W2 + c] : 0.f;
      }
      __syncthreads();
      if (lane_s) {
        for (int r = rows - 1; r >= 0; --r) {
          float* d = DX + r * W2 + 2 * tid;
          const float nr = d[0] + lr_ * ar + li_ * ai, ni = d[1] + lr_ * ai - li_ * ar;
          ar = nr; ai = ni;
          d[0] = ar; d[1] = ai;
          const float* xp = X + r * W2 + 2 * tid;
          dlr += ar * xp[0] + ai * xp[1];
          dli += ai * xp[0] - ar * xp[1];
        }
      }
      __syncthreads();
      lr_gemm<true>(DX, 1, W2, U, H, 1, pb + pl.p_B, H, 1, RV, H, LR_TT);
      lr_gemm<true>(DX, W2, 1, gB, H, 1, GO, H, 1, LR_TT, H, RV);
      __syncthreads();
      if (first) {
        lr_gemm<true>(GO, 1, H, XI, I, 1, pin, I, 1, H, I, LR_TT);             // dW_in += g^T x
        if (tid < H) {
          float acc = 0.f;
          for (int r = 0; r < LR_TT; ++r) acc += GO[r * H + tid];
          pin[H * I + tid] += acc;
        }
      } else {
        for (int e = tid; e < rows * H; e += LR_THREADS) a.gmap[(row0 + t0) * H + e] = GO[e];
      }
      __syncthreads();
    }
    if (lane_s) {
      pb[pl.p_nu + tid] += dlr;
      pb[pl.p_th + tid] += dli;
    }
    __syncthreads();
  }
}

// raw[i] = sum over workgroups, in workgroup order
__global__ void __launch_bounds__(256)
lr_reduce_kernel(const float* __restrict__ partial, int groups, int P, float* __restrict__ raw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float acc = 0.f;
  for (int g = 0; g < groups; ++g) acc += partial[(long long)g * P + i];
  raw[i] = acc;
}

// raw holds d lambda (re in log_nu's slot, im in log_theta's), d(gamma B) as (2 S2, H) in B's slot, d(C re, -C im) in
// C's; the rest is final.  One thread per entry of grad_params.
__global__ void __launch_bounds__(256)
lr_chain_kernel(LrPlan pl, const float* __restrict__ params, const float* __restrict__ raw, float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= pl.P) return;
  if (i < pl.off_blk0) { grad[i] = raw[i]; return; }
  const int blk = (i - pl.off_blk0) / pl.PB, j = i - pl.off_blk0 - blk * pl.PB;
  const float* bp = params + pl.off_blk0 + blk * pl.PB;
  const float* br = raw + pl.off_blk0 + blk * pl.PB;
  const int H = pl.H, S2 = pl.S2;
  float out;
  if (j < pl.p_B) {
    // lambda = r (cos phi + i sin phi), r = exp(-nu), nu = exp(log_nu), phi = exp(log_theta)
    const int s = j < S2 ? j : j - S2;
    const float nu = expf(bp[pl.p_nu + s]), phi = expf(bp[pl.p_th + s]), r = expf(-nu);
    float sn, cs;
    sincosf(phi, &sn, &cs);
    const float dre = br[pl.p_nu + s], dim = br[pl.p_th + s];
    out = j < S2 ? -(dre * cs + dim * sn) * r * nu : (dim * cs - dre * sn) * r * phi;
  } else if (j < pl.p_C) {
    const int e = j - pl.p_B, s = e / (2 * H), rem = e - s * 2 * H, h = rem >> 1, c = rem & 1;
    out = expf(bp[pl.p_lg + s]) * br[pl.p_B + (2 * s + c) * H + h];
  } else if (j < pl.p_D) {
    out = (j - pl.p_C) & 1 ? -br[j] : br[j];
  } else if (j >= pl.p_lg && j < pl.p_Wg) {
    const int s = j - pl.p_lg;
    float acc = 0.f;
    for (int h = 0; h < H; ++h)
      for (int c = 0; c < 2; ++c) acc += br[pl.p_B + (2 * s + c) * H + h] * bp[pl.p_B + (s * H + h) * 2 + c];
    out = expf(bp[pl.p_lg + s]) * acc;
  } else {
    out = br[j];
  }
  grad[i] = out;
}

}  // namespace
