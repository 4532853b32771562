// resnet_embed_kernel.h -- kernels of the ResNetEmbedding1D trunk (include/sbi_amd_resnet.h): plan, weight streaming,
// forward, delta pass, weight gradients.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "../../include/sbi_amd_resnet.h"

#define RN_THREADS 256
#define RN_SA 132    // activation row stride in LDS: 16-byte aligned rows; C-layout stores of a wave fall on 32 banks
#define RN_NPS 144   // weight-panel row stride in LDS: = 16 mod 32, the B fragment's two k-rows of a 32-lane half land on
                     // disjoint banks
#define RN_GRID 256  // workgroups of the row-tile kernels: one per CU (the LDS image allows no second one)
#define RN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

typedef float rn_f4 __attribute__((ext_vector_type(4)));

struct RnPlan {
  int cin, ci, ch, nb;      // the config
  int CN, CI, CH;           // padded to multiples of 16
  int has_init;
  int64_t PI, PB, P;        // flat parameters: initial Linear, one block, all
  int64_t II, BI, IMG;      // image floats: initial Linear, one block, all
};

struct RnShape {
  int64_t rows, Rp;
  int RT, KP, lds_fwd, lds_bwd;
  int S;                    // row splits of the weight-gradient launches
  int64_t chunk;            // rows per split (a multiple of 64)
  int64_t PS;               // floats of one partial image
  int64_t ws_floats[2];     // inference, training
  int64_t o_stash, o_delta, o_dz, o_a, o_c, o_da, o_dc, o_part;
};

static inline int rn_pad16(int v) { return (v + 15) / 16 * 16; }

static inline int rn_plan_sizes(const sbi_amd_resnet_config* cfg, RnPlan* pl) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->c_in < 1 || cfg->c_internal < 1 || cfg->c_hidden < 1 || cfg->n_blocks < 1) return SBI_AMD_E_BADARG;
  if (cfg->c_in > SBI_AMD_RESNET_MAX_WIDTH || cfg->c_internal > SBI_AMD_RESNET_MAX_WIDTH ||
      cfg->c_hidden > SBI_AMD_RESNET_MAX_WIDTH || cfg->n_blocks > SBI_AMD_RESNET_MAX_BLOCKS)
    return SBI_AMD_E_UNSUPPORTED;
  pl->cin = cfg->c_in, pl->ci = cfg->c_internal, pl->ch = cfg->c_hidden, pl->nb = cfg->n_blocks;
  pl->CN = rn_pad16(pl->cin), pl->CI = rn_pad16(pl->ci), pl->CH = rn_pad16(pl->ch);
  pl->has_init = pl->cin != pl->ci;
  pl->PI = pl->has_init ? (int64_t)pl->ci * pl->cin + pl->ci : 0;
  pl->PB = 2 * (int64_t)pl->ch * pl->ci + (int64_t)pl->ch * pl->ch + 2 * pl->ch + pl->ci;
  pl->P = pl->PI + pl->nb * pl->PB;
  pl->II = pl->has_init ? (int64_t)pl->CN * pl->CI + pl->CI : 0;
  pl->BI = 4 * (int64_t)pl->CI * pl->CH + 2 * (int64_t)pl->CH * pl->CH + 2 * pl->CH + pl->CI;
  pl->IMG = pl->II + pl->nb * pl->BI;
  return 0;
}

static inline int rn_lds_bytes(int RT, int KP) { return (3 * RT * RN_SA + 2 * KP * RN_NPS) * 4; }

static inline int rn_plan_shape(const RnPlan& pl, int64_t rows, RnShape* sh) {
  if (rows < 1) return SBI_AMD_E_BADARG;
  if (rows >= 2147483648LL - 64) return SBI_AMD_E_UNSUPPORTED;
  sh->rows = rows;
  sh->Rp = (rows + 63) / 64 * 64;
  sh->RT = rows <= 16 * RN_GRID ? 16 : rows <= 64 * RN_GRID ? 32 : 64;
  sh->KP = sh->RT == 64 ? 32 : 64;
  sh->lds_fwd = sh->lds_bwd = rn_lds_bytes(sh->RT, sh->KP);
  if (sh->lds_fwd > 160 * 1024) return SBI_AMD_E_LDS;
  int64_t S = (sh->Rp + 1023) / 1024;
  if (S > SBI_AMD_RESNET_MAX_SPLITS) S = SBI_AMD_RESNET_MAX_SPLITS;
  sh->chunk = ((sh->Rp / 64 + S - 1) / S) * 64;
  sh->S = (int)((sh->Rp + sh->chunk - 1) / sh->chunk);
  sh->PS = pl.PB > pl.PI ? pl.PB : pl.PI;
  const int64_t rc = sh->Rp * pl.CI, rh = sh->Rp * pl.CH;
  int64_t o = pl.IMG;
  sh->ws_floats[0] = o;
  sh->o_stash = o, o += (pl.nb + 1) * rc;
  sh->o_delta = o, o += rc;
  sh->o_dz = o, o += rc;
  sh->o_a = o, o += rh;
  sh->o_c = o, o += rh;
  sh->o_da = o, o += rh;
  sh->o_dc = o, o += rh;
  sh->o_part = o, o += sh->S > 1 ? sh->S * sh->PS : 0;
  sh->ws_floats[1] = o;
  return 0;
}

// ---- pack: flat parameters -> staged image --------------------------------------------------------------------------
// element j of the (K, NP) transposed, padded image of W (N, K)
__device__ __forceinline__ float rn_pad_t(const float* W, int N, int K, int NP, int64_t j) {
  const int k = (int)(j / NP), n = (int)(j % NP);
  return (k < K && n < N) ? W[(int64_t)n * K + k] : 0.f;
}
// element j of the (NP, KPad) padded image of W (N, K) in its own orientation
__device__ __forceinline__ float rn_pad_n(const float* W, int N, int K, int KPad, int64_t j) {
  const int n = (int)(j / KPad), k = (int)(j % KPad);
  return (k < K && n < N) ? W[(int64_t)n * K + k] : 0.f;
}

__global__ void __launch_bounds__(RN_THREADS) rn_pack_kernel(RnPlan pl, const float* __restrict__ params,
                                                             float* __restrict__ img) {
  const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (i >= pl.IMG) return;
  float v;
  if (i < pl.II) {
    const int64_t m = (int64_t)pl.CN * pl.CI;
    if (i < m) v = rn_pad_t(params, pl.ci, pl.cin, pl.CI, i);
    else v = (i - m) < pl.ci ? params[(int64_t)pl.ci * pl.cin + (i - m)] : 0.f;
  } else {
    int64_t j = i - pl.II;
    const float* pb = params + pl.PI + (j / pl.BI) * pl.PB;
    j %= pl.BI;
    const int ci = pl.ci, ch = pl.ch, CI = pl.CI, CH = pl.CH;
    const float* w0 = pb;
    const float* b0 = w0 + (int64_t)ch * ci;
    const float* w2 = b0 + ch;
    const float* b2 = w2 + (int64_t)ch * ch;
    const float* w4 = b2 + ch;
    const float* b4 = w4 + (int64_t)ci * ch;
    const int64_t ic = (int64_t)CI * CH, hh = (int64_t)CH * CH;
    if (j < ic) v = rn_pad_t(w0, ch, ci, CH, j);
    else if ((j -= ic) < CH) v = j < ch ? b0[j] : 0.f;
    else if ((j -= CH) < hh) v = rn_pad_t(w2, ch, ch, CH, j);
    else if ((j -= hh) < CH) v = j < ch ? b2[j] : 0.f;
    else if ((j -= CH) < ic) v = rn_pad_t(w4, ci, ch, CI, j);
    else if ((j -= ic) < CI) v = j < ci ? b4[j] : 0.f;
    else if ((j -= CI) < ic) v = rn_pad_n(w0, ch, ci, CI, j);
    else if ((j -= ic) < hh) v = rn_pad_n(w2, ch, ch, CH, j);
    else v = rn_pad_n(w4, ci, ch, CH, j - hh);
  }
  img[i] = v;
}

// offsets inside one block's image
struct RnBlockImg {
  const float *w0t, *b0, *w2t, *b2, *w4t, *b4, *w0n, *w2n, *w4n;
};
__device__ __forceinline__ RnBlockImg rn_block_img(const RnPlan& pl, const float* img, int b) {
  RnBlockImg o;
  const int64_t ic = (int64_t)pl.CI * pl.CH, hh = (int64_t)pl.CH * pl.CH;
  o.w0t = img + pl.II + (int64_t)b * pl.BI;
  o.b0 = o.w0t + ic;
  o.w2t = o.b0 + pl.CH;
  o.b2 = o.w2t + hh;
  o.w4t = o.b2 + pl.CH;
  o.b4 = o.w4t + ic;
  o.w0n = o.b4 + pl.CI;
  o.w2n = o.w0n + ic;
  o.w4n = o.w2n + hh;
  return o;
}

// ---- weight streaming -------------------------------------------------------------------------------------------------
struct RnMat {
  const float* w;   // (Kp, Np) row-major in global memory, both multiples of 16; null: no matrix
  int Kp, Np;
};

template <int KP>
struct RnStream {
  static constexpr int Q = KP * 128 / 4 / RN_THREADS;   // 16-byte loads per thread for a full panel
  rn_f4 pre[Q];
  int buf;

  // the loads of panel `p` of `m` into registers (in flight until commit)
  __device__ __forceinline__ void issue(const RnMat& m, int p) {
    const int kp = min(KP, m.Kp - p * KP);
    const int n4 = kp * m.Np / 4;
    const rn_f4* src = reinterpret_cast<const rn_f4*>(m.w + (int64_t)p * KP * m.Np);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = threadIdx.x + q * RN_THREADS;
      if (i < n4) pre[q] = src[i];
    }
  }
  // registers -> LDS buffer `buf`
  __device__ __forceinline__ void commit(float* wbuf, const RnMat& m, int p) {
    const int kp = min(KP, m.Kp - p * KP);
    const int n4 = kp * m.Np / 4;
    float* dst = wbuf + buf * KP * RN_NPS;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = threadIdx.x + q * RN_THREADS;
      if (i < n4) {
        const int e = i * 4, r = e / m.Np, c = e - r * m.Np;
        *reinterpret_cast<rn_f4*>(dst + r * RN_NPS + c) = pre[q];
      }
    }
  }
};

// The wave's share of a row tile: RT / 16 row sub-tiles, the 8 column tiles dealt round-robin to the waves of one sub-tile.
template <int RT>
struct RnWave {
  static constexpr int RSUB = RT / 16, NG = 4 / RSUB, NTP = 8 / NG;
};

// acc[j] (column tile ng + NG j) = actIn (this wave's 16 rows, K = cur.Kp) x cur.  On entry the stream holds panel 0 of
// `cur` in registers; on exit panel 0 of `nxt` (when there is one).  One barrier per panel.
template <int RT, int KP>
__device__ __forceinline__ void rn_gemm(RnStream<KP>& st, float* wbuf, const RnMat cur, const RnMat nxt,
                                        const float* actIn, rn_f4 (&acc)[RnWave<RT>::NTP]) {
  using W = RnWave<RT>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rsub = wave % W::RSUB, ng = wave / W::RSUB;
  const int l16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int j = 0; j < W::NTP; ++j) acc[j] = rn_f4{0.f, 0.f, 0.f, 0.f};
  const int npan = (cur.Kp + KP - 1) / KP;
  const float* arow = actIn + (rsub * 16 + l16) * RN_SA + 4 * g;
  for (int p = 0; p < npan; ++p) {
    st.commit(wbuf, cur, p);
    __syncthreads();
    if (p + 1 < npan) st.issue(cur, p + 1);
    else if (nxt.w) st.issue(nxt, 0);
    const float* wb = wbuf + st.buf * KP * RN_NPS + l16;
    const int kp = min(KP, cur.Kp - p * KP);
    for (int kc = 0; kc < kp; kc += 16) {
      const rn_f4 a = *reinterpret_cast<const rn_f4*>(arow + p * KP + kc);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float* brow = wb + (kc + 4 * g + s) * RN_NPS;
#pragma unroll
        for (int j = 0; j < W::NTP; ++j) {
          const int nt = ng + W::NG * j;
          if (nt * 16 < cur.Np) acc[j] = RN_MFMA(a[s], brow[nt * 16], acc[j]);
        }
      }
    }
    st.buf ^= 1;
  }
}

// f(row in tile, column, value) for every accumulator element this lane holds
template <int RT, typename F>
__device__ __forceinline__ void rn_each(const rn_f4 (&acc)[RnWave<RT>::NTP], int Np, F f) {
  using W = RnWave<RT>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rsub = wave % W::RSUB, ng = wave / W::RSUB;
#pragma unroll
  for (int j = 0; j < W::NTP; ++j) {
    const int nt = ng + W::NG * j;
    if (nt * 16 < Np) {
#pragma unroll
      for (int r = 0; r < 4; ++r) f(rsub * 16 + 4 * (lane >> 4) + r, nt * 16 + (lane & 15), acc[j][r]);
    }
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------
struct RnFwdArgs {
  const float* img;
  const float* x;
  float* out;
  float* stash;   // (nb + 1, Rp, CI) or null
  int64_t rows, Rp;
  int64_t trows;   // rows the tiles cover: rows, or Rp with a stash (its padding rows are written too)
};

template <int RT, int KP>
__global__ void __launch_bounds__(RN_THREADS) rn_forward_kernel(RnPlan pl, RnFwdArgs a) {
  extern __shared__ float rn_lds[];
  float* A = rn_lds;
  float* B = A + RT * RN_SA;
  float* C = B + RT * RN_SA;
  float* wbuf = C + RT * RN_SA;
  RnStream<KP> st;
  st.buf = 0;
  rn_f4 acc[RnWave<RT>::NTP];
  const int CI = pl.CI, CH = pl.CH;
  const int64_t slab = a.Rp * CI;
  const int64_t ntiles = (a.trows + RT - 1) / RT;
  const RnMat none{nullptr, 0, 0};
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * RT;
    __syncthreads();   // the previous tile's last epilogue is done with A
    const RnBlockImg first = rn_block_img(pl, a.img, 0);
    const RnMat m_init{a.img, pl.CN, CI};
    const RnMat m_first{first.w0t, CI, CH};
    st.issue(pl.has_init ? m_init : m_first, 0);
    {
      const int Kin = pl.has_init ? pl.CN : CI;
      float* dst = pl.has_init ? C : A;
      for (int i = threadIdx.x; i < RT * Kin; i += RN_THREADS) {
        const int r = i / Kin, c = i - r * Kin;
        const int64_t gr = row0 + r;
        const float v = (gr < a.rows && c < pl.cin) ? a.x[gr * pl.cin + c] : 0.f;
        dst[r * RN_SA + c] = v;
        if (!pl.has_init && a.stash) a.stash[gr * CI + c] = v;
      }
    }
    if (pl.has_init) {
      rn_gemm<RT, KP>(st, wbuf, m_init, m_first, C, acc);
      const float* bias = a.img + (int64_t)pl.CN * CI;
      rn_each<RT>(acc, CI, [&](int r, int c, float v) {
        v += bias[c];
        A[r * RN_SA + c] = v;
        if (a.stash) a.stash[(row0 + r) * CI + c] = v;
      });
    }
    for (int b = 0; b < pl.nb; ++b) {
      const RnBlockImg bi = rn_block_img(pl, a.img, b);
      const RnMat m0{bi.w0t, CI, CH}, m2{bi.w2t, CH, CH}, m4{bi.w4t, CH, CI};
      const RnMat mn = b + 1 < pl.nb ? RnMat{rn_block_img(pl, a.img, b + 1).w0t, CI, CH} : none;
      rn_gemm<RT, KP>(st, wbuf, m0, m2, A, acc);
      rn_each<RT>(acc, CH, [&](int r, int c, float v) { B[r * RN_SA + c] = fmaxf(v + bi.b0[c], 0.f); });
      rn_gemm<RT, KP>(st, wbuf, m2, m4, B, acc);
      rn_each<RT>(acc, CH, [&](int r, int c, float v) { C[r * RN_SA + c] = fmaxf(v + bi.b2[c], 0.f); });
      rn_gemm<RT, KP>(st, wbuf, m4, mn, C, acc);
      const bool last = b + 1 == pl.nb;
      float* keep = a.stash ? a.stash + (b + 1) * slab : nullptr;
      rn_each<RT>(acc, CI, [&](int r, int c, float v) {
        v = fmaxf((v + bi.b4[c]) + A[r * RN_SA + c], 0.f);
        A[r * RN_SA + c] = v;
        const int64_t gr = row0 + r;
        if (keep) keep[gr * CI + c] = v;
        if (last && gr < a.rows && c < pl.ci) a.out[gr * pl.ci + c] = v;
      });
    }
  }
}

// ---- backward: the delta pass of one block -----------------------------------------------------------------------------
struct RnBwdArgs {
  const float* img;
  const float* xin;     // the block's input, (Rp, CI) slab of the stash
  const float* xout;    // the block's output, likewise
  const float* dsrc;    // delta at the block's output: (drows, dcols) with row stride dstride
  int64_t dstride, drows;
  int dcols;
  float* dout;          // delta at the block's input, (Rp, CI); may alias dsrc
  float *dz, *ha, *hc, *da, *dc;
  int64_t rows;       // Rp: the padding rows are walked too, their deltas are zero
  int block;
};

template <int RT, int KP>
__global__ void __launch_bounds__(RN_THREADS) rn_delta_kernel(RnPlan pl, RnBwdArgs a) {
  extern __shared__ float rn_lds[];
  float* A = rn_lds;
  float* B = A + RT * RN_SA;
  float* C = B + RT * RN_SA;
  float* wbuf = C + RT * RN_SA;
  RnStream<KP> st;
  st.buf = 0;
  rn_f4 acc[RnWave<RT>::NTP];
  const int CI = pl.CI, CH = pl.CH;
  const int64_t ntiles = (a.rows + RT - 1) / RT;
  const RnBlockImg bi = rn_block_img(pl, a.img, a.block);
  const RnMat m0{bi.w0t, CI, CH}, m2{bi.w2t, CH, CH}, n4{bi.w4n, CI, CH}, n2{bi.w2n, CH, CH}, n0{bi.w0n, CH, CI};
  const RnMat none{nullptr, 0, 0};
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * RT;
    __syncthreads();
    st.issue(m0, 0);
    for (int i = threadIdx.x; i < RT * CI; i += RN_THREADS) {
      const int r = i / CI, c = i - r * CI;
      A[r * RN_SA + c] = a.xin[(row0 + r) * CI + c];
    }
    rn_gemm<RT, KP>(st, wbuf, m0, m2, A, acc);
    rn_each<RT>(acc, CH, [&](int r, int c, float v) {
      v = fmaxf(v + bi.b0[c], 0.f);
      B[r * RN_SA + c] = v;
      a.ha[(row0 + r) * CH + c] = v;
    });
    rn_gemm<RT, KP>(st, wbuf, m2, n4, B, acc);
    rn_each<RT>(acc, CH, [&](int r, int c, float v) {
      v = fmaxf(v + bi.b2[c], 0.f);
      C[r * RN_SA + c] = v;
      a.hc[(row0 + r) * CH + c] = v;
    });
    // dZ = delta where the block's output is positive.  A was last read by the first GEMM, two barriers ago.
    for (int i = threadIdx.x; i < RT * CI; i += RN_THREADS) {
      const int r = i / CI, c = i - r * CI;
      const int64_t gr = row0 + r;
      const float d = (gr < a.drows && c < a.dcols) ? a.dsrc[gr * a.dstride + c] : 0.f;
      const float v = a.xout[gr * CI + c] > 0.f ? d : 0.f;
      A[r * RN_SA + c] = v;
      a.dz[gr * CI + c] = v;
    }
    rn_gemm<RT, KP>(st, wbuf, n4, n2, A, acc);
    rn_each<RT>(acc, CH, [&](int r, int c, float v) {
      v = C[r * RN_SA + c] > 0.f ? v : 0.f;
      C[r * RN_SA + c] = v;
      a.dc[(row0 + r) * CH + c] = v;
    });
    rn_gemm<RT, KP>(st, wbuf, n2, n0, C, acc);
    rn_each<RT>(acc, CH, [&](int r, int c, float v) {
      v = B[r * RN_SA + c] > 0.f ? v : 0.f;
      B[r * RN_SA + c] = v;
      a.da[(row0 + r) * CH + c] = v;
    });
    rn_gemm<RT, KP>(st, wbuf, n0, none, B, acc);
    rn_each<RT>(acc, CI, [&](int r, int c, float v) { a.dout[(row0 + r) * CI + c] = v + A[r * RN_SA + c]; });
  }
}

// ---- backward: weight gradients ---------------------------------------------------------------------------------------
// dW (N, K) = D^T A over the rows of split blockIdx.y, db (N) = the column sums of D.  One workgroup per 16-row strip of
// dW (blockIdx.x) and matrix (blockIdx.z); wave w takes quarter w of the split's rows, the quarters are added in wave
// order.
struct RnWgMat {
  const float* D;     // (Rp, NP) padded, rows past the batch are zero
  const float* A;     // (arows, K) with row stride astride: guarded
  int64_t astride, arows;
  int N, NP, K;
  int64_t ow, ob;     // offsets of dW / db in the output image
};
struct RnWgArgs {
  RnWgMat m[3];
  float* out;         // grad_params region (splits == 1) or the partial images
  int64_t out_stride; // floats between two splits' images
  int64_t Rp, chunk;
};

__global__ void __launch_bounds__(RN_THREADS) rn_wgrad_kernel(RnWgArgs a) {
  __shared__ float red[3][8][4][64];
  __shared__ float redb[3][64];
  const RnWgMat m = a.m[blockIdx.z];
  const int n0 = blockIdx.x * 16;
  if (n0 >= m.NP) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, g = lane >> 4;
  const int64_t s0 = (int64_t)blockIdx.y * a.chunk;
  const int64_t s1 = min(s0 + a.chunk, a.Rp);
  const int64_t quarter = (s1 - s0) / 4;      // chunk and Rp are multiples of 64
  const int64_t r_begin = s0 + wave * quarter, r_end = r_begin + quarter;
  const int nkt = (m.K + 15) / 16;
  rn_f4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = rn_f4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int64_t r = r_begin + g; r < r_end; r += 4) {
    const float d = m.D[r * m.NP + n0 + l16];
    bsum += d;
    const bool rv = r < m.arows;
    const float* ar = m.A + r * m.astride;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < nkt) {
        const int k = j * 16 + l16;
        const float v = (rv && k < m.K) ? ar[k] : 0.f;
        acc[j] = RN_MFMA(d, v, acc[j]);
      }
    }
  }
  bsum += __shfl_xor(bsum, 16);
  bsum += __shfl_xor(bsum, 32);
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[wave - 1][j][q][lane] = acc[j][q];
    if (g == 0) redb[wave - 1][l16] = bsum;
  }
  __syncthreads();
  if (wave > 0) return;
  float* out = a.out + (int64_t)blockIdx.y * a.out_stride;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < nkt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = acc[j][q];
        v += red[0][j][q][lane];
        v += red[1][j][q][lane];
        v += red[2][j][q][lane];
        const int n = n0 + 4 * g + q, k = j * 16 + l16;
        if (n < m.N && k < m.K) out[m.ow + (int64_t)n * m.K + k] = v;
      }
    }
  }
  if (g == 0 && n0 + l16 < m.N) out[m.ob + n0 + l16] = ((bsum + redb[0][l16]) + redb[1][l16]) + redb[2][l16];
}

// grad[i] = the partial images' element i added in split order
__global__ void __launch_bounds__(RN_THREADS) rn_reduce_kernel(const float* __restrict__ part, int S, int64_t stride,
                                                               int64_t n, float* __restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (i >= n) return;
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[s * stride + i];
  grad[i] = v;
}
