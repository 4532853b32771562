// lc2st_kernel.h -- the L-C2ST classifier ensemble on gfx950: plan, device functions, kernels (launchers: lc2st.hip).
//
// Reference behaviour: sbi/diagnostics/lc2st.py (train_lc2st / eval_lc2st over skorch's NeuralNetBinaryClassifier on
// MLPClassifierModule, sbi/utils/metrics.py); the contract is spelled out in include/sbi_amd_lc2st.h.
//
// Execution model
//   * one workgroup (8 waves) per member, for whole epochs.  The member's weights and biases live in LDS for the whole
//     launch (rows zero-padded to 16, row stride + 4 floats); Adam's moments live in global memory and are touched once
//     per step; the weight-gradient accumulators live in registers as MFMA D tiles, split over the waves by output tile.
//   * a batch is walked in chunks of LC_CR = 32 rows.  Per chunk the three hidden-layer GEMMs of the forward
//     (Z^T = W X^T, the transposed form of fmpe_kernel.h: M = output feature, N = row), of d/dactivation (W2^T dZ2^T)
//     and of d/dW (dZ^T A: M = output feature, N = input feature, K = row) all run on v_mfma_f32_16x16x4_f32; the
//     1-wide output layer, the loss and the bias gradients are a few hundred flops on the VALU.
//   * every sum over rows is ordered by (chunk, row in chunk) of the member's own epoch order: K steps of an MFMA chain,
//     or a sequential loop of one thread.  No atomics, no inter-workgroup traffic: a member's results do not depend on
//     which other members share the launch.
//   * at the corner F = 64, H = 128: weights 8704 + 16896 floats, vectors 512, chunk tiles X 2176 + A1 4224 + A2 4224,
//     scratch 768 = 150 KB of the 160 KB LDS.  A 64-row chunk would need 189 KB with the padded strides, so chunks are
//     32 rows at every shape: half the K depth of the d/dW chains per barrier, one code path.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_lc2st.h"
#include "../../include/sbi_amd_nsf.h"
#include "adam_math.h"
#include "philox.h"
#include "shuffle_prp.h"

namespace {

typedef float lc_f4 __attribute__((ext_vector_type(4)));
#define LC_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// wave (uniform, in an SGPR), lane, and the MFMA lane coordinates c (row / column in the tile) and g (K quarter).  The
// empty asm makes them opaque per call: without it the compiler hoists every tile's address arithmetic out of the epoch
// loop (lc_train_kernel: 256 VGPRs + 342 spilled); with it 157 VGPRs, none spilled, 188 SGPRs spilled to VGPR lanes,
// 8 bytes of scratch per lane for the one out-of-line call (2 waves per SIMD either way: the workgroup is 8 waves).
#define LC_LANE_IDS(tid)                                                  \
  int lc_tid_ = (tid);                                                    \
  asm volatile("" : "+v"(lc_tid_));                                       \
  const int wave = __builtin_amdgcn_readfirstlane(lc_tid_ >> 6);          \
  const int lane = lc_tid_ & 63, c = lane & 15, g = lane >> 4;            \
  (void)lane
#define LC_THREADS 512
#define LC_WAVES 8
#define LC_CR 32              // rows per chunk (two 16-row MFMA column tiles)
#define LC_LOSS_TID 448       // wave 7, lane 0: owns the scalar sums (loss, d/db3)
#define LC_EVAL_ROWS 512      // rows of theta per evaluation workgroup
#define LC_STREAM_TAG 0x4C433253u
// scratch region (floats): logit, dlogit, label, row loss, source row (int) per chunk row; scalars; eval accumulators
#define LC_M_LOGIT 0
#define LC_M_DLOG 32
#define LC_M_Y 64
#define LC_M_LOSS 96
#define LC_M_SRC 128
#define LC_M_B3 160
#define LC_M_BC1 161
#define LC_M_BC2 162
#define LC_M_BCAST 163
#define LC_M_PACC 256
#define LC_MISC_FLOATS (256 + LC_EVAL_ROWS)

struct LcPlan {
  int D, Dx, F, H, Fp, Hp, HB, FB, B, ld1, ld2;
  long long P;
  int off_b1, off_w2, off_b2, off_w3, off_b3;                                // flat parameter offsets
  int o_w1, o_w2, o_b1, o_b2, o_w3, o_b1e, o_x, o_a1, o_a2, o_misc, lds_floats;   // LDS offsets (floats)
  float lr, wd, beta1, beta2, eps, threshold;
  int patience, max_epochs;
};

static int lc_round_up(int a, int m) { return (a + m - 1) / m * m; }

static int lc_build_plan(const sbi_amd_lc2st_config* cfg, LcPlan* pl) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->D < 1 || cfg->Dx < 1 || cfg->H < 1 || cfg->B < 1 || cfg->max_epochs < 1 || cfg->patience < 1)
    return SBI_AMD_E_BADARG;
  if (cfg->D + cfg->Dx > 64 || cfg->H > 128) return SBI_AMD_E_UNSUPPORTED;
  if (cfg->B > (1 << 24) || cfg->max_epochs > (1 << 24)) return SBI_AMD_E_UNSUPPORTED;
  LcPlan p;
  p.D = cfg->D; p.Dx = cfg->Dx; p.F = cfg->D + cfg->Dx; p.H = cfg->H; p.B = cfg->B;
  p.Fp = lc_round_up(p.F, 16); p.Hp = lc_round_up(p.H, 16); p.HB = p.Hp / 16; p.FB = p.Fp / 16;
  p.ld1 = p.Fp + 4; p.ld2 = p.Hp + 4;
  p.off_b1 = p.H * p.F; p.off_w2 = p.off_b1 + p.H; p.off_b2 = p.off_w2 + p.H * p.H; p.off_w3 = p.off_b2 + p.H;
  p.off_b3 = p.off_w3 + p.H; p.P = p.off_b3 + 1;
  int o = 0;
  p.o_w1 = o; o += p.Hp * p.ld1;
  p.o_w2 = o; o += p.Hp * p.ld2;
  p.o_b1 = o; o += p.Hp;
  p.o_b2 = o; o += p.Hp;
  p.o_w3 = o; o += p.Hp;
  p.o_b1e = o; o += p.Hp;
  p.o_x = o; o += LC_CR * p.ld1;
  p.o_a1 = o; o += LC_CR * p.ld2;
  p.o_a2 = o; o += LC_CR * p.ld2;
  p.o_misc = o; o += LC_MISC_FLOATS;
  p.lds_floats = o;
  if ((long long)o * 4 > 160 * 1024) return SBI_AMD_E_LDS;
  p.lr = cfg->lr; p.wd = cfg->weight_decay; p.beta1 = cfg->beta1; p.beta2 = cfg->beta2; p.eps = cfg->eps;
  p.threshold = cfg->threshold; p.patience = cfg->patience; p.max_epochs = cfg->max_epochs;
  *pl = p;
  return 0;
}

// ---- parameters: flat (torch order) <-> LDS image ------------------------------------------------------------------
__device__ __forceinline__ void lc_load_params(const LcPlan& pl, float* __restrict__ lds, const float* __restrict__ p,
                                               int tid) {
  for (int i = tid; i < pl.o_x; i += LC_THREADS) lds[i] = 0.f;     // weights and vectors, pads included
  __syncthreads();
  for (int i = tid; i < pl.H * pl.F; i += LC_THREADS) {
    const int h = i / pl.F, f = i - h * pl.F;
    lds[pl.o_w1 + h * pl.ld1 + f] = p[i];
  }
  for (int i = tid; i < pl.H * pl.H; i += LC_THREADS) {
    const int h = i / pl.H, k = i - h * pl.H;
    lds[pl.o_w2 + h * pl.ld2 + k] = p[pl.off_w2 + i];
  }
  if (tid < pl.H) {
    lds[pl.o_b1 + tid] = p[pl.off_b1 + tid];
    lds[pl.o_b2 + tid] = p[pl.off_b2 + tid];
    lds[pl.o_w3 + tid] = p[pl.off_w3 + tid];
  }
  if (tid == 0) lds[pl.o_misc + LC_M_B3] = p[pl.off_b3];
  __syncthreads();
}

__device__ __forceinline__ void lc_store_params(const LcPlan& pl, const float* __restrict__ lds, float* __restrict__ p,
                                                int tid) {
  for (int i = tid; i < pl.H * pl.F; i += LC_THREADS) {
    const int h = i / pl.F, f = i - h * pl.F;
    p[i] = lds[pl.o_w1 + h * pl.ld1 + f];
  }
  for (int i = tid; i < pl.H * pl.H; i += LC_THREADS) {
    const int h = i / pl.H, k = i - h * pl.H;
    p[pl.off_w2 + i] = lds[pl.o_w2 + h * pl.ld2 + k];
  }
  if (tid < pl.H) {
    p[pl.off_b1 + tid] = lds[pl.o_b1 + tid];
    p[pl.off_b2 + tid] = lds[pl.o_b2 + tid];
    p[pl.off_w3 + tid] = lds[pl.o_w3 + tid];
  }
  if (tid == 0) p[pl.off_b3] = lds[pl.o_misc + LC_M_B3];
}

// ---- one chunk of rows into LDS: X[LC_CR][Fp] (zero beyond the row count and beyond F), labels -----------------------
// positions pos0 .. pos0 + cnt - 1 of the member's row list, through the epoch's permutation when `permute`
__device__ __forceinline__ void lc_gather(const LcPlan& pl, float* __restrict__ lds, const float* __restrict__ data,
                                          long long R, const int* __restrict__ rows_m,
                                          const float* __restrict__ labels_m, int pos0, int cnt, bool permute,
                                          unsigned n_perm, int hb, unsigned long long key, int tid) {
  float* misc = lds + pl.o_misc;
  int* src = reinterpret_cast<int*>(misc + LC_M_SRC);
  if (tid < LC_CR) {
    int s = -1;
    float y = 0.f;
    if (tid < cnt) {
      const unsigned i = (unsigned)(pos0 + tid);
      const unsigned p = permute ? shf_prp(i, n_perm, hb, key) : i;
      s = rows_m[p];
      y = labels_m[p];
      if (s < 0 || (long long)s >= R) s = -1;     // never out of bounds: such a row reads as zeros
    }
    src[tid] = s;
    misc[LC_M_Y + tid] = y;
  }
  __syncthreads();
  for (int e = tid; e < LC_CR * pl.Fp; e += LC_THREADS) {
    const int j = e / pl.Fp, f = e - j * pl.Fp;
    const int s = src[j];
    lds[pl.o_x + j * pl.ld1 + f] = (s >= 0 && f < pl.F) ? data[(long long)s * pl.F + f] : 0.f;
  }
  __syncthreads();
}

// ---- forward of one chunk: logits of the LC_CR rows -> misc[LC_M_LOGIT ..]; leaves a1, a2 in LDS --------------------
// K1 = width of the first contraction (a multiple of 16: Fp in training, round_up(D, 16) when x_o is folded into bias1)
__device__ __forceinline__ void lc_forward(const LcPlan& pl, float* __restrict__ lds, int K1,
                                           const float* __restrict__ bias1, int tid) {
  LC_LANE_IDS(tid);
  const float* W1 = lds + pl.o_w1;
  const float* W2 = lds + pl.o_w2;
  const float* X = lds + pl.o_x;
  float* A1 = lds + pl.o_a1;
  float* A2 = lds + pl.o_a2;
  const int ntile = pl.HB * (LC_CR / 16);
  for (int t = wave; t < ntile; t += LC_WAVES) {
    const int mb = t >> 1, nb = t & 1;
    const float* ap = W1 + (16 * mb + c) * pl.ld1 + 4 * g;
    const float* bp = X + (16 * nb + c) * pl.ld1 + 4 * g;
    lc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K1; k += 16) {
      const lc_f4 a = *reinterpret_cast<const lc_f4*>(ap + k);
      const lc_f4 b = *reinterpret_cast<const lc_f4*>(bp + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = LC_MFMA(a[r], b[r], acc);
    }
    const int h0 = 16 * mb + 4 * g;
    const lc_f4 bi = *reinterpret_cast<const lc_f4*>(bias1 + h0);
    lc_f4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = fmaxf(acc[r] + bi[r], 0.f);
    *reinterpret_cast<lc_f4*>(A1 + (16 * nb + c) * pl.ld2 + h0) = o;
  }
  __syncthreads();
  const float* b2 = lds + pl.o_b2;
  for (int t = wave; t < ntile; t += LC_WAVES) {
    const int mb = t >> 1, nb = t & 1;
    const float* ap = W2 + (16 * mb + c) * pl.ld2 + 4 * g;
    const float* bp = A1 + (16 * nb + c) * pl.ld2 + 4 * g;
    lc_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < pl.Hp; k += 16) {
      const lc_f4 a = *reinterpret_cast<const lc_f4*>(ap + k);
      const lc_f4 b = *reinterpret_cast<const lc_f4*>(bp + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = LC_MFMA(a[r], b[r], acc);
    }
    const int h0 = 16 * mb + 4 * g;
    const lc_f4 bi = *reinterpret_cast<const lc_f4*>(b2 + h0);
    lc_f4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = fmaxf(acc[r] + bi[r], 0.f);
    *reinterpret_cast<lc_f4*>(A2 + (16 * nb + c) * pl.ld2 + h0) = o;
  }
  __syncthreads();
  {   // logit[n] = w3 . a2[n] + b3: 16 lanes per row, strided partial sums, then a fixed xor tree
    const int n = tid >> 4, q = tid & 15;
    const float* w3 = lds + pl.o_w3;
    float s = 0.f;
    for (int h = q; h < pl.Hp; h += 16) s += w3[h] * A2[n * pl.ld2 + h];
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (q == 0) lds[pl.o_misc + LC_M_LOGIT + n] = s + lds[pl.o_misc + LC_M_B3];
  }
  __syncthreads();
}

__device__ __forceinline__ float lc_bce_with_logits(float z, float y) {
  return fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
}

// ---- gradient accumulators of one batch -----------------------------------------------------------------------------
struct LcGrad {
  lc_f4 w2[8];     // tile t = wave + 8 j of the HB x HB grid of dW2 (row = output feature, column = input feature)
  lc_f4 w1[4];     // tile t = wave + 8 j of the HB x FB grid of dW1
  float b1, b2, w3;   // thread h < Hp
  float b3, loss;     // thread LC_LOSS_TID: d/db3 and the sum of the row losses
};

__device__ __forceinline__ void lc_zero_grad(LcGrad& G) {
#pragma unroll
  for (int j = 0; j < 8; ++j) G.w2[j] = lc_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) G.w1[j] = lc_f4{0.f, 0.f, 0.f, 0.f};
  G.b1 = G.b2 = G.w3 = G.b3 = G.loss = 0.f;
}

// row losses of the chunk after lc_forward, summed into G.loss by LC_LOSS_TID (validation: no gradient)
__device__ __forceinline__ void lc_chunk_loss(const LcPlan& pl, float* __restrict__ lds, int cnt, float& loss, int tid) {
  float* misc = lds + pl.o_misc;
  if (tid < LC_CR)
    misc[LC_M_LOSS + tid] = tid < cnt ? lc_bce_with_logits(misc[LC_M_LOGIT + tid], misc[LC_M_Y + tid]) : 0.f;
  __syncthreads();
  if (tid == LC_LOSS_TID)
    for (int n = 0; n < LC_CR; ++n) loss += misc[LC_M_LOSS + n];
  __syncthreads();
}

// backward of one chunk after lc_forward; inv_n = 1 / (rows of the whole batch)
__device__ __forceinline__ void lc_backward(const LcPlan& pl, float* __restrict__ lds, int cnt, float inv_n, LcGrad& G,
                                            int tid) {
  LC_LANE_IDS(tid);
  float* misc = lds + pl.o_misc;
  const float* W2 = lds + pl.o_w2;
  const float* X = lds + pl.o_x;
  float* A1 = lds + pl.o_a1;
  float* A2 = lds + pl.o_a2;
  if (tid < LC_CR) {
    const float z = misc[LC_M_LOGIT + tid], y = misc[LC_M_Y + tid];
    const bool v = tid < cnt;
    const float sig = 1.f / (1.f + expf(-z));
    misc[LC_M_LOSS + tid] = v ? lc_bce_with_logits(z, y) : 0.f;
    misc[LC_M_DLOG + tid] = v ? (sig - y) * inv_n : 0.f;
  }
  __syncthreads();
  if (tid < pl.Hp) {     // column h of a2: d/dw3, dz2 = relu' * dlogit * w3 (in place), d/db2 -- rows in order
    const float w = lds[pl.o_w3 + tid];
    for (int n = 0; n < LC_CR; ++n) {
      const float a = A2[n * pl.ld2 + tid], dl = misc[LC_M_DLOG + n];
      G.w3 += dl * a;
      const float dz = a > 0.f ? dl * w : 0.f;
      G.b2 += dz;
      A2[n * pl.ld2 + tid] = dz;
    }
  }
  if (tid == LC_LOSS_TID) {
    for (int n = 0; n < LC_CR; ++n) {
      G.b3 += misc[LC_M_DLOG + n];
      G.loss += misc[LC_M_LOSS + n];
    }
  }
  __syncthreads();
  // dW2 += dZ2^T A1 (K = the chunk's rows)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int t = wave + LC_WAVES * j;
    if (t < pl.HB * pl.HB) {
      const int mb = t / pl.HB, nb = t - mb * pl.HB;
      const float* ap = A2 + 16 * mb + c;
      const float* bp = A1 + 16 * nb + c;
#pragma unroll
      for (int n = 0; n < LC_CR; n += 4) G.w2[j] = LC_MFMA(ap[(n + g) * pl.ld2], bp[(n + g) * pl.ld2], G.w2[j]);
    }
  }
  // dA1^T = W2^T dZ2^T, kept in registers until every wave is done reading a1
  lc_f4 da[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    da[j] = lc_f4{0.f, 0.f, 0.f, 0.f};
    const int t = wave + LC_WAVES * j;
    if (t < pl.HB * (LC_CR / 16)) {
      const int mb = t >> 1, nb = t & 1;
      const float* ap = W2 + (4 * g) * pl.ld2 + 16 * mb + c;
      const float* bp = A2 + (16 * nb + c) * pl.ld2 + 4 * g;
      for (int k = 0; k < pl.Hp; k += 16) {
        const lc_f4 b = *reinterpret_cast<const lc_f4*>(bp + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) da[j] = LC_MFMA(ap[(k + r) * pl.ld2], b[r], da[j]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {     // dz1 = relu' * da1, over a1 in place
    const int t = wave + LC_WAVES * j;
    if (t < pl.HB * (LC_CR / 16)) {
      const int mb = t >> 1, nb = t & 1;
      float* p = A1 + (16 * nb + c) * pl.ld2 + 16 * mb + 4 * g;
      const lc_f4 a1 = *reinterpret_cast<const lc_f4*>(p);
      lc_f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = a1[r] > 0.f ? da[j][r] : 0.f;
      *reinterpret_cast<lc_f4*>(p) = o;
    }
  }
  __syncthreads();
  // dW1 += dZ1^T X
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = wave + LC_WAVES * j;
    if (t < pl.HB * pl.FB) {
      const int mb = t / pl.FB, nb = t - mb * pl.FB;
      const float* ap = A1 + 16 * mb + c;
      const float* bp = X + 16 * nb + c;
#pragma unroll
      for (int n = 0; n < LC_CR; n += 4) G.w1[j] = LC_MFMA(ap[(n + g) * pl.ld2], bp[(n + g) * pl.ld1], G.w1[j]);
    }
  }
  if (tid < pl.Hp)
    for (int n = 0; n < LC_CR; ++n) G.b1 += A1[n * pl.ld2 + tid];
  __syncthreads();
}

// ---- g = dloss/dp + weight_decay p, then Adam (TRAIN) or store (batch_grad) ----------------------------------------
template <bool TRAIN>
__device__ __forceinline__ void lc_apply_one(const LcPlan& pl, float* __restrict__ lp, long long idx, float g,
                                             float* __restrict__ gm, float* __restrict__ gv, float* __restrict__ gout,
                                             const AdamK& k) {
  const float p = *lp;
  g = __builtin_fmaf(pl.wd, p, g);
  if (TRAIN) {
    float m = gm[idx], v = gv[idx];
    *lp = adam_apply_one(p, g, m, v, k);
    gm[idx] = m;
    gv[idx] = v;
  } else {
    gout[idx] = g;
  }
}

template <bool TRAIN>
__device__ __forceinline__ void lc_apply(const LcPlan& pl, float* __restrict__ lds, const LcGrad& G,
                                         float* __restrict__ gm, float* __restrict__ gv, float* __restrict__ gout,
                                         const AdamK& k, int tid) {
  LC_LANE_IDS(tid);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int t = wave + LC_WAVES * j;
    if (t < pl.HB * pl.HB) {
      const int mb = t / pl.HB, nb = t - mb * pl.HB;
      const int col = 16 * nb + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mb + 4 * g + r;
        if (row < pl.H && col < pl.H)
          lc_apply_one<TRAIN>(pl, lds + pl.o_w2 + row * pl.ld2 + col, pl.off_w2 + row * pl.H + col, G.w2[j][r], gm, gv,
                              gout, k);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = wave + LC_WAVES * j;
    if (t < pl.HB * pl.FB) {
      const int mb = t / pl.FB, nb = t - mb * pl.FB;
      const int col = 16 * nb + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mb + 4 * g + r;
        if (row < pl.H && col < pl.F)
          lc_apply_one<TRAIN>(pl, lds + pl.o_w1 + row * pl.ld1 + col, row * pl.F + col, G.w1[j][r], gm, gv, gout, k);
      }
    }
  }
  if (tid < pl.H) {
    lc_apply_one<TRAIN>(pl, lds + pl.o_b1 + tid, pl.off_b1 + tid, G.b1, gm, gv, gout, k);
    lc_apply_one<TRAIN>(pl, lds + pl.o_b2 + tid, pl.off_b2 + tid, G.b2, gm, gv, gout, k);
    lc_apply_one<TRAIN>(pl, lds + pl.o_w3 + tid, pl.off_w3 + tid, G.w3, gm, gv, gout, k);
  }
  if (tid == LC_LOSS_TID) lc_apply_one<TRAIN>(pl, lds + pl.o_misc + LC_M_B3, pl.off_b3, G.b3, gm, gv, gout, k);
  __syncthreads();
}

// adam.hip's host-side expressions for step `st`, evaluated on the device (out of line: double pow is long and runs
// once per step)
__device__ __noinline__ void lc_bias_corrections(float beta1, float beta2, int st, float* bc1, float* bc2_sqrt) {
  *bc1 = (float)(1.0 - pow((double)beta1, (double)st));
  *bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)st));
}

struct LcArgs {
  const float* data; long long R;
  const int* rows; const float* labels; long long row_stride;
  const int* n_train; const int* n_valid; const int* member_id;
  unsigned seed_lo, seed_hi;
  float* params; float* best_params; float* exp_avg; float* exp_avg_sq;
  int* step; float* best; int* misses; int* epoch; int* best_epoch; int* stopped; float* history;
  int epochs;
  // batch_grad
  const float* params_in; int which, g_epoch, g_batch; float* loss_out; float* grad_out;
};

__device__ __forceinline__ unsigned long long lc_epoch_key(const LcArgs& a, int e, int member) {
  unsigned o[4];
  philox4x32_10((unsigned)e, 0u, (unsigned)member, LC_STREAM_TAG, a.seed_lo, a.seed_hi, o);
  return (unsigned long long)o[0] | ((unsigned long long)o[1] << 32);
}

// gradient of one batch: positions [pos0, pos0 + cnt_b) of the member's list, chunk by chunk
__device__ __forceinline__ void lc_batch(const LcPlan& pl, float* __restrict__ lds, const LcArgs& a,
                                         const int* __restrict__ rows_m, const float* __restrict__ labels_m, int pos0,
                                         int cnt_b, bool permute, unsigned n_perm, int hb, unsigned long long key,
                                         LcGrad& G, int tid) {
  const float inv_n = 1.f / (float)cnt_b;
  for (int c0 = 0; c0 < cnt_b; c0 += LC_CR) {
    const int cnt = min(LC_CR, cnt_b - c0);
    lc_gather(pl, lds, a.data, a.R, rows_m, labels_m, pos0 + c0, cnt, permute, n_perm, hb, key, tid);
    lc_forward(pl, lds, pl.Fp, lds + pl.o_b1, tid);
    lc_backward(pl, lds, cnt, inv_n, G, tid);
  }
}

__global__ void __launch_bounds__(LC_THREADS) lc_train_kernel(LcPlan pl, LcArgs a) {
  extern __shared__ float lds[];
  const int m = blockIdx.x, tid = threadIdx.x;
  if (a.stopped[m]) return;
  const int nt = a.n_train[m], nv = a.n_valid[m], member = a.member_id[m];
  if (nt < 1 || nv < 1 || (long long)nt + nv > a.row_stride) {     // nothing to train or validate on, or a row list
    if (tid == 0) a.stopped[m] = 1;                                 // longer than its stride: a caller's mistake,
    return;                                                         // never a hang or a read past the list
  }
  const int* rows_m = a.rows + (long long)m * a.row_stride;
  const float* labels_m = a.labels + (long long)m * a.row_stride;
  float* gm = a.exp_avg + (long long)m * pl.P;
  float* gv = a.exp_avg_sq + (long long)m * pl.P;
  float* misc = lds + pl.o_misc;
  lc_load_params(pl, lds, a.params + (long long)m * pl.P, tid);
  int e = a.epoch[m], st = a.step[m], misses = a.misses[m], best_epoch = a.best_epoch[m], stopped = 0;
  float best = a.best[m];
  const int hb = shf_half_bits(nt);
  if (e >= pl.max_epochs) stopped = 1;     // (history has max_epochs rows)
  LcGrad G;
  for (int it = 0; it < a.epochs && !stopped; ++it) {
    const unsigned long long key = lc_epoch_key(a, e, member);
    float tsum = 0.f;
    for (int pos0 = 0; pos0 < nt; pos0 += pl.B) {
      const int cnt_b = min(pl.B, nt - pos0);
      st += 1;
      if (tid == 0) lc_bias_corrections(pl.beta1, pl.beta2, st, misc + LC_M_BC1, misc + LC_M_BC2);
      lc_zero_grad(G);
      lc_batch(pl, lds, a, rows_m, labels_m, pos0, cnt_b, true, (unsigned)nt, hb, key, G, tid);
      const AdamK k = {1.f, pl.beta1, pl.beta2, pl.eps, pl.lr / misc[LC_M_BC1], misc[LC_M_BC2]};
      if (tid == LC_LOSS_TID) tsum += (G.loss * (1.f / (float)cnt_b)) * (float)cnt_b;
      lc_apply<true>(pl, lds, G, gm, gv, nullptr, k, tid);
    }
    float vsum = 0.f;
    for (int c0 = 0; c0 < nv; c0 += LC_CR) {
      const int cnt = min(LC_CR, nv - c0);
      lc_gather(pl, lds, a.data, a.R, rows_m, labels_m, nt + c0, cnt, false, 0u, 0, 0ull, tid);
      lc_forward(pl, lds, pl.Fp, lds + pl.o_b1, tid);
      lc_chunk_loss(pl, lds, cnt, vsum, tid);
    }
    if (tid == LC_LOSS_TID) {
      const float valid = vsum / (float)nv;
      float* h = a.history + ((long long)m * pl.max_epochs + e) * 2;
      h[0] = tsum / (float)nt;
      h[1] = valid;
      misc[LC_M_BCAST] = valid;
    }
    __syncthreads();
    const float valid = misc[LC_M_BCAST];
    if (valid < best * (1.f - pl.threshold)) {
      best = valid;
      misses = 0;
      best_epoch = e;
      lc_store_params(pl, lds, a.best_params + (long long)m * pl.P, tid);
    } else {
      misses += 1;
    }
    e += 1;
    if (misses >= pl.patience || e >= pl.max_epochs) stopped = 1;
    __syncthreads();
  }
  lc_store_params(pl, lds, a.params + (long long)m * pl.P, tid);
  if (tid == 0) {
    a.epoch[m] = e; a.step[m] = st; a.misses[m] = misses; a.best_epoch[m] = best_epoch; a.best[m] = best;
    a.stopped[m] = stopped;
  }
}

__global__ void __launch_bounds__(LC_THREADS) lc_grad_kernel(LcPlan pl, LcArgs a) {
  extern __shared__ float lds[];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int nt = a.n_train[m], nv = a.n_valid[m];
  float* gout = a.grad_out + (long long)m * pl.P;
  int pos0, cnt_b;
  if (a.which == 0) {
    pos0 = a.g_batch * pl.B;
    cnt_b = min(pl.B, nt - pos0);
  } else {
    pos0 = nt;
    cnt_b = nv;
  }
  if (nt < 1 || nv < 0 || pos0 < 0 || cnt_b < 1 || (long long)nt + nv > a.row_stride) {
    for (long long i = tid; i < pl.P; i += LC_THREADS) gout[i] = 0.f;
    if (tid == 0) a.loss_out[m] = __builtin_nanf("");
    return;
  }
  const int* rows_m = a.rows + (long long)m * a.row_stride;
  const float* labels_m = a.labels + (long long)m * a.row_stride;
  lc_load_params(pl, lds, a.params_in + (long long)m * pl.P, tid);
  const unsigned long long key = lc_epoch_key(a, a.g_epoch, a.member_id[m]);
  LcGrad G;
  lc_zero_grad(G);
  lc_batch(pl, lds, a, rows_m, labels_m, pos0, cnt_b, a.which == 0, (unsigned)nt, shf_half_bits(nt), key, G, tid);
  const AdamK k = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  if (tid == LC_LOSS_TID) a.loss_out[m] = G.loss * (1.f / (float)cnt_b);
  lc_apply<false>(pl, lds, G, nullptr, nullptr, gout, k, tid);
}

// ---- evaluation at one x_o ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LC_THREADS)
lc_eval_kernel(LcPlan pl, const float* __restrict__ params, const float* __restrict__ theta,
               const float* __restrict__ x_o, long long n, int E, int theta_groups, float* __restrict__ proba_out) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, grp = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * LC_EVAL_ROWS;
  const int nrows = (int)min((long long)LC_EVAL_ROWS, n - row0);
  float* misc = lds + pl.o_misc;
  float* pacc = misc + LC_M_PACC;
  const float* th = theta + (theta_groups > 1 ? (long long)grp * n * pl.D : 0ll) + row0 * pl.D;
  const int K1 = (pl.D + 15) / 16 * 16;
  pacc[tid] = 0.f;
  for (int e = 0; e < E; ++e) {
    lc_load_params(pl, lds, params + ((long long)grp * E + e) * pl.P, tid);
    if (tid < pl.Hp) {     // the x_o term of the first layer, once per member: b1 + W1[:, D:] x_o
      float s = lds[pl.o_b1 + tid];
      if (tid < pl.H)
        for (int j = 0; j < pl.Dx; ++j) s += lds[pl.o_w1 + tid * pl.ld1 + pl.D + j] * x_o[j];
      lds[pl.o_b1e + tid] = s;
    }
    __syncthreads();
    for (int c0 = 0; c0 < nrows; c0 += LC_CR) {
      const int cnt = min(LC_CR, nrows - c0);
      for (int i = tid; i < LC_CR * pl.Fp; i += LC_THREADS) {
        const int j = i / pl.Fp, f = i - j * pl.Fp;
        lds[pl.o_x + j * pl.ld1 + f] = (j < cnt && f < pl.D) ? th[(long long)(c0 + j) * pl.D + f] : 0.f;
      }
      __syncthreads();
      lc_forward(pl, lds, K1, lds + pl.o_b1e, tid);
      if (tid < cnt) pacc[c0 + tid] += 1.f / (1.f + expf(misc[LC_M_LOGIT + tid]));     // 1 - sigmoid(z)
      __syncthreads();
    }
  }
  if (tid < nrows) proba_out[(long long)grp * n + row0 + tid] = pacc[tid] / (float)E;
}

// score[g] = mean_i (proba[g][i] - 1/2)^2: thread t sums i = t, t + 256, ...; then a fixed tree
__global__ void __launch_bounds__(256)
lc_score_kernel(const float* __restrict__ proba, long long n, float* __restrict__ score_out) {
  __shared__ float red[256];
  const float* p = proba + (long long)blockIdx.x * n;
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) {
    const float d = p[i] - 0.5f;
    s += d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) score_out[blockIdx.x] = red[0] / (float)n;
}

}  // namespace
