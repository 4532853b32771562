// embed_kernel.h -- FCEmbedding / PermutationInvariantEmbedding on gfx950: plan, device functions, kernels (launchers:
// embed.hip).  Contract: include/sbi_amd_embed.h.  Nearest relative: lc2st_kernel.h (same GEMM forms and LDS image).
//
// Execution model
//   * a workgroup is 8 waves.  The net's weights and biases are staged once per workgroup in LDS (rows zero-padded to
//     16, row stride + 4 floats) and the rows are walked in chunks of 32 (16 for the widest nets, whose image would not
//     fit next to 32-row tiles: a property of the configuration, never of the batch).  Per chunk every layer's GEMM runs on
//     v_mfma_f32_16x16x4_f32 in the transposed form Z^T = W A^T (M = output feature, N = row); bias and ReLU on the VALU.
//     All activations a_0 .. a_L of the chunk stay in LDS; nothing of size (rows, hidden) goes to global memory.
//   * rows are flat: for the permutation-invariant net row = b T + t, so a chunk packs trials of several batch elements
//     when T is small and no tile row is wasted.  A trial's embedding is one MFMA column: it depends on that row alone.
//   * pooling (forward): a workgroup owns whole batch elements.  After each chunk one thread per (element, feature) adds
//     the chunk's trials of that element in the order t = lo, lo + 1, ... onto a carry that travels from chunk to
//     chunk: the sum of an element is ONE sequential chain over t = 0 .. T - 1.  Masked trials add +0 (a select, never a
//     multiplication).  The association therefore depends on the trial index alone.
//   * backward: the chunk's forward is recomputed, then per layer dW += dZ^T A (K = rows of the chunk) accumulates in
//     MFMA D tiles that live in registers for the whole launch; d/da = W^T dZ^T on the MFMA; relu' on the VALU, in place.
//     Each workgroup writes its partial gradient to the workspace; a second kernel adds the partials in workgroup order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_embed.h"
#include "../../include/sbi_amd_nsf.h"

namespace {

typedef float em_f4 __attribute__((ext_vector_type(4)));
#define EM_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// wave (uniform), lane, MFMA lane coordinates c (row / column in the tile) and g (K quarter); opaque per call so that
// tile address arithmetic is not hoisted out of the chunk loop (see lc2st_kernel.h)
#define EM_LANE_IDS(tid)                                                  \
  int em_tid_ = (tid);                                                    \
  asm volatile("" : "+v"(em_tid_));                                       \
  const int wave = __builtin_amdgcn_readfirstlane(em_tid_ >> 6);          \
  const int lane = em_tid_ & 63, c = lane & 15, g = lane >> 4;            \
  (void)lane
#define EM_THREADS 512
#define EM_WAVES 8
#define EM_CR 32               // rows per chunk (two 16-row MFMA column tiles); 16 when 32 would not fit the LDS
#define EM_MAXL 4
#define EM_CW 80               // carry width: trial out_dim + 1 (the count column) <= 65
#define EM_M_VALID 0           // misc region: validity of the chunk's rows
#define EM_M_CARRY 32          // [2][EM_CW] pooled carry, double-buffered by chunk parity
#define EM_M_CCNT (32 + 2 * EM_CW)     // [2][EM_CW] count carry
#define EM_MISC_FLOATS (32 + 4 * EM_CW)
#define EM_MAX_ROWS (0x7fffffffll - 64)
#define EM_FWD_GROUPS 1024
#define EM_BWD_GROUPS 512
#define EM_BWD_WS_FLOATS (1ll << 22)

struct EmPlan {
  int L;
  int dim[EM_MAXL + 1], dimp[EM_MAXL + 1], ld[EM_MAXL + 1];    // widths of a_0 .. a_L, padded to 16, LDS row stride
  int off_w[EM_MAXL], off_b[EM_MAXL];                          // flat parameter offsets
  int o_w[EM_MAXL], o_b[EM_MAXL], o_a[EM_MAXL + 1], o_misc;    // LDS offsets (floats)
  int o_act, lds_floats, P;
  int CR, sh;                                                  // rows per chunk (32 or 16) and log2(CR / 16)
};

static int em_round_up(int a, int m) { return (a + m - 1) / m * m; }

// sizes: widths, flat parameter offsets and P, the weight image.  Valid for every shape inside the per-field limits.
static int em_plan_sizes(const sbi_amd_fc_embed_config* cfg, EmPlan* pl) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->in_dim < 1 || cfg->hidden < 1 || cfg->out_dim < 1 || cfg->num_layers < 1) return SBI_AMD_E_BADARG;
  if (cfg->in_dim > 64 || cfg->hidden > 128 || cfg->out_dim > 64 || cfg->num_layers < 2 || cfg->num_layers > EM_MAXL)
    return SBI_AMD_E_UNSUPPORTED;
  EmPlan p = {};
  p.L = cfg->num_layers;
  for (int l = 0; l <= p.L; ++l) {
    p.dim[l] = l == 0 ? cfg->in_dim : (l == p.L ? cfg->out_dim : cfg->hidden);
    p.dimp[l] = em_round_up(p.dim[l], 16);
    p.ld[l] = p.dimp[l] + 4;
  }
  int off = 0, o = 0;
  for (int l = 0; l < p.L; ++l) {
    p.off_w[l] = off; off += p.dim[l + 1] * p.dim[l];
    p.off_b[l] = off; off += p.dim[l + 1];
    p.o_w[l] = o; o += p.dimp[l + 1] * p.ld[l];
    p.o_b[l] = o; o += p.dimp[l + 1];
  }
  p.P = off;
  p.o_act = o;
  *pl = p;
  return 0;
}

// sizes plus the row tiles: SBI_AMD_E_LDS when the image and the tiles do not fit one workgroup's LDS
static int em_build_plan(const sbi_amd_fc_embed_config* cfg, EmPlan* pl) {
  EmPlan p;
  const int rc = em_plan_sizes(cfg, &p);
  if (rc) return rc;
  int o;
  for (p.CR = EM_CR; p.CR >= 16; p.CR /= 2) {     // the widest nets walk their rows in half chunks
    o = p.o_act;
    for (int l = 0; l <= p.L; ++l) { p.o_a[l] = o; o += p.CR * p.ld[l]; }
    p.o_misc = o; o += EM_MISC_FLOATS;
    p.lds_floats = o;
    if ((long long)o * 4 <= 160 * 1024) break;
  }
  if (p.CR < 16) return SBI_AMD_E_LDS;
  p.sh = p.CR / 32;
  *pl = p;
  return 0;
}

// workgroups of a backward launch over `rows` rows: a host-side function of the shape alone
static int em_bwd_groups(const EmPlan& pl, long long rows) {
  long long n = (rows + pl.CR - 1) / pl.CR;
  if (n > EM_BWD_GROUPS) n = EM_BWD_GROUPS;
  const long long cap = EM_BWD_WS_FLOATS / pl.P;
  if (n > cap) n = cap;
  return n < 1 ? 1 : (int)n;
}

// ---- flat parameters (state_dict order) -> LDS image ----------------------------------------------------------------
__device__ __forceinline__ void em_load_params(const EmPlan& pl, float* __restrict__ lds, const float* __restrict__ p,
                                               int tid) {
  for (int i = tid; i < pl.o_act; i += EM_THREADS) lds[i] = 0.f;     // weights and biases, pads included
  __syncthreads();
  for (int l = 0; l < pl.L; ++l) {
    const int K = pl.dim[l], M = pl.dim[l + 1];
    for (int i = tid; i < M * K; i += EM_THREADS) {
      const int h = i / K, f = i - h * K;
      lds[pl.o_w[l] + h * pl.ld[l] + f] = p[pl.off_w[l] + i];
    }
    if (tid < M) lds[pl.o_b[l] + tid] = p[pl.off_b[l] + tid];
  }
  __syncthreads();
}

// ---- rows [r0, r0 + CR) into a_0 (zero beyond r_end and beyond in_dim); MASK: NaN -> 0, all-NaN row -> invalid ----
template <bool MASK>
__device__ __forceinline__ void em_load_rows(const EmPlan& pl, float* __restrict__ lds, const float* __restrict__ x,
                                             long long r0, long long r_end, int tid) {
  const int F = pl.dim[0], Fp = pl.dimp[0];
  float* X = lds + pl.o_a[0];
  for (int e = tid; e < pl.CR * Fp; e += EM_THREADS) {
    const int j = e / Fp, f = e - j * Fp;
    float v = 0.f;
    if (r0 + j < r_end && f < F) {
      v = x[(r0 + j) * F + f];
      if (MASK && v != v) v = 0.f;
    }
    X[j * pl.ld[0] + f] = v;
  }
  if (tid < pl.CR) {
    float ok = 0.f;
    if (r0 + tid < r_end) {
      ok = 1.f;
      if (MASK) {
        bool all_nan = true;
        for (int f = 0; f < F; ++f) {
          const float v = x[(r0 + tid) * F + f];
          all_nan = all_nan && (v != v);
        }
        if (all_nan) ok = 0.f;
      }
    }
    lds[pl.o_misc + EM_M_VALID + tid] = ok;
  }
  __syncthreads();
}

// ---- a_{l+1} = relu(W_l a_l + b_l) for the chunk ---------------------------------------------------------------------
__device__ __forceinline__ void em_layer_forward(const EmPlan& pl, float* __restrict__ lds, int l, int tid) {
  EM_LANE_IDS(tid);
  const int ldi = pl.ld[l], ldo = pl.ld[l + 1], Kp = pl.dimp[l];
  const float* W = lds + pl.o_w[l];
  const float* bias = lds + pl.o_b[l];
  const float* In = lds + pl.o_a[l];
  float* Out = lds + pl.o_a[l + 1];
  const int ntile = (pl.dimp[l + 1] / 16) << pl.sh;
  for (int t = wave; t < ntile; t += EM_WAVES) {
    const int mb = t >> pl.sh, nb = t & pl.sh;
    const float* ap = W + (16 * mb + c) * ldi + 4 * g;
    const float* bp = In + (16 * nb + c) * ldi + 4 * g;
    em_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Kp; k += 16) {
      const em_f4 a = *reinterpret_cast<const em_f4*>(ap + k);
      const em_f4 b = *reinterpret_cast<const em_f4*>(bp + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = EM_MFMA(a[r], b[r], acc);
    }
    const int h0 = 16 * mb + 4 * g;
    const em_f4 bi = *reinterpret_cast<const em_f4*>(bias + h0);
    em_f4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {     // relu that hands a NaN on, as torch.relu does (fmaxf would answer 0)
      const float z = acc[r] + bi[r];
      o[r] = z < 0.f ? 0.f : z;
    }
    *reinterpret_cast<em_f4*>(Out + (16 * nb + c) * ldo + h0) = o;
  }
  __syncthreads();
}

__device__ __forceinline__ void em_chunk_forward(const EmPlan& pl, float* __restrict__ lds, int tid) {
  for (int l = 0; l < pl.L; ++l) em_layer_forward(pl, lds, l, tid);
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// POOL == false: out (N, out_dim); chunks are dealt round-robin to the workgroups.
// POOL == true: x (B, T, in_dim); workgroup w owns elements [w b_per, min(B, (w + 1) b_per)); head_in (B, E + 1).
struct EmFwdArgs {
  const float* params; const float* x; float* out;
  long long N;          // rows (B T when pooling)
  int B, T, b_per, mean;
};

template <bool POOL>
__global__ void __launch_bounds__(EM_THREADS) em_forward_kernel(EmPlan pl, EmFwdArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  em_load_params(pl, lds, a.params, tid);
  const int E = pl.dim[pl.L];
  const float* AL = lds + pl.o_a[pl.L];
  const int ldL = pl.ld[pl.L];
  if (!POOL) {
    const long long nchunk = (a.N + pl.CR - 1) / pl.CR;
    for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
      const long long r0 = ch * pl.CR;
      em_load_rows<false>(pl, lds, a.x, r0, a.N, tid);
      em_chunk_forward(pl, lds, tid);
      for (int e = tid; e < pl.CR * E; e += EM_THREADS) {
        const int j = e / E, h = e - j * E;
        if (r0 + j < a.N) a.out[(r0 + j) * E + h] = AL[j * ldL + h];
      }
      __syncthreads();
    }
  } else {
    float* misc = lds + pl.o_misc;
    const int b0 = blockIdx.x * a.b_per;
    const int b1 = min(a.B, b0 + a.b_per);
    const long long T = a.T;
    const long long row_a = (long long)b0 * T, row_b = (long long)b1 * T;
    const int CW = E + 1;
    int par = 0;
    for (long long r0 = row_a; r0 < row_b; r0 += pl.CR, par ^= 1) {
      em_load_rows<true>(pl, lds, a.x, r0, row_b, tid);
      em_chunk_forward(pl, lds, tid);
      const long long r1 = r0 + pl.CR;
      const long long b_first = r0 / T;
      for (int idx = tid; idx < pl.CR * CW; idx += EM_THREADS) {
        const int j = idx / CW, e = idx - j * CW;
        const long long b = b_first + j;
        const long long s = b * T;                      // the element's first row
        if (b >= b1 || s >= r1) continue;
        const bool cont_in = s < r0, cont_out = s + T > r1;
        const int lo = (int)(max(s, r0) - r0), hi = (int)(min(s + T, r1) - r0);
        float acc = cont_in ? misc[EM_M_CARRY + par * EM_CW + e] : 0.f;
        float cnt = cont_in ? misc[EM_M_CCNT + par * EM_CW + e] : 0.f;
        for (int n = lo; n < hi; ++n) {
          const float v = misc[EM_M_VALID + n];
          const float y = e < E ? (v != 0.f ? AL[n * ldL + e] : 0.f) : v;
          acc += y;
          cnt += v;
        }
        if (cont_out) {
          misc[EM_M_CARRY + (par ^ 1) * EM_CW + e] = acc;
          misc[EM_M_CCNT + (par ^ 1) * EM_CW + e] = cnt;
        } else {
          a.out[b * CW + e] = (e < E && a.mean) ? acc / cnt : acc;
        }
      }
      __syncthreads();
    }
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// POOL == false: grad_out (N, out_dim).  POOL == true: the gradient of row b T + t is grad_head_in[b][:E] (divided by
// count[b] under mean) when the trial is valid and 0 when it is masked; count[b] = head_in[b][E].
struct EmBwdArgs {
  const float* params; const float* x; const float* grad_out; const float* head_in;
  float* grad_x;        // may be null
  float* partial;       // (gridDim.x, P)
  long long N;
  int T, mean;
};

// Weight-gradient tiles live in registers: layer l's tiles are dealt round-robin to the waves, and a wave keeps its
// share in fixed slots of GW by the layer's role: first layer slots 0..3 (<= 8 x 4 tiles), last layer 4..7 (<= 4 x 8),
// hidden layer l (1 or 2) slots 8 l .. 8 l + 7 (<= 8 x 8).
#define EM_GT 24

// dW_l += dz_{l+1}^T a_l over the chunk's rows (K = CR), slots JB .. JB + NS - 1
template <int JB, int NS>
__device__ __forceinline__ void em_dw(const EmPlan& pl, const float* __restrict__ lds, int l, em_f4 (&GW)[EM_GT],
                                      int tid) {
  EM_LANE_IDS(tid);
  const int ldi = pl.ld[l], ldo = pl.ld[l + 1], KB = pl.dimp[l] / 16;
  const int ntile = (pl.dimp[l + 1] / 16) * KB;
  const float* A = lds + pl.o_a[l];
  const float* DZ = lds + pl.o_a[l + 1];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int t = wave + EM_WAVES * j;
    if (t < ntile) {
      const int mb = t / KB, nb = t - mb * KB;
      const float* ap = DZ + 16 * mb + c;
      const float* bp = A + 16 * nb + c;
      for (int n = 0; n < pl.CR; n += 16) {
#pragma unroll
        for (int q = 0; q < 16; q += 4)
          GW[JB + j] = EM_MFMA(ap[(n + q + g) * ldo], bp[(n + q + g) * ldi], GW[JB + j]);
      }
    }
  }
}

template <int JB, int NS>
__device__ __forceinline__ void em_dw_store(const EmPlan& pl, int l, const em_f4 (&GW)[EM_GT], float* __restrict__ part,
                                            int tid) {
  EM_LANE_IDS(tid);
  const int KB = pl.dimp[l] / 16, K = pl.dim[l], M = pl.dim[l + 1];
  const int ntile = (pl.dimp[l + 1] / 16) * KB;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int t = wave + EM_WAVES * j;
    if (t < ntile) {
      const int mb = t / KB, nb = t - mb * KB;
      const int col = 16 * nb + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mb + 4 * g + r;
        if (row < M && col < K) part[pl.off_w[l] + row * K + col] = GW[JB + j][r];
      }
    }
  }
}

// d/da_l^T = W_l^T dz_{l+1}^T, then dz_l = relu'(a_l) * d/da_l over a_l in place (RELU == false: layer 0, d/dx)
template <bool RELU>
__device__ __forceinline__ void em_da(const EmPlan& pl, float* __restrict__ lds, int l, int tid) {
  EM_LANE_IDS(tid);
  const int ldi = pl.ld[l], ldo = pl.ld[l + 1], KB = pl.dimp[l] / 16, Mp = pl.dimp[l + 1];
  const float* W = lds + pl.o_w[l];
  float* A = lds + pl.o_a[l];
  const float* DZ = lds + pl.o_a[l + 1];
  em_f4 da[2];     // kept in registers until every wave is done reading a_l
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    da[j] = em_f4{0.f, 0.f, 0.f, 0.f};
    const int t = wave + EM_WAVES * j;
    if (t < (KB << pl.sh)) {
      const int mb = t >> pl.sh, nb = t & pl.sh;
      const float* ap = W + (4 * g) * ldi + 16 * mb + c;
      const float* bp = DZ + (16 * nb + c) * ldo + 4 * g;
      for (int k = 0; k < Mp; k += 16) {
        const em_f4 b = *reinterpret_cast<const em_f4*>(bp + k);
#pragma unroll
        for (int r = 0; r < 4; ++r) da[j] = EM_MFMA(ap[(k + r) * ldi], b[r], da[j]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int t = wave + EM_WAVES * j;
    if (t < (KB << pl.sh)) {
      const int mb = t >> pl.sh, nb = t & pl.sh;
      float* p = A + (16 * nb + c) * ldi + 16 * mb + 4 * g;
      const em_f4 al = *reinterpret_cast<const em_f4*>(p);
      em_f4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (!RELU || al[r] > 0.f) ? da[j][r] : 0.f;
      *reinterpret_cast<em_f4*>(p) = o;
    }
  }
}

template <bool POOL>
__global__ void __launch_bounds__(EM_THREADS) em_backward_kernel(EmPlan pl, EmBwdArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  em_load_params(pl, lds, a.params, tid);
  const float* misc = lds + pl.o_misc;
  const int E = pl.dim[pl.L];
  em_f4 GW[EM_GT];
  float GB[EM_MAXL];
#pragma unroll
  for (int j = 0; j < EM_GT; ++j) GW[j] = em_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < EM_MAXL; ++l) GB[l] = 0.f;

  const long long nchunk = (a.N + pl.CR - 1) / pl.CR;
  for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const long long r0 = ch * pl.CR;
    em_load_rows<POOL>(pl, lds, a.x, r0, a.N, tid);
    em_chunk_forward(pl, lds, tid);
    {   // dz_L = relu'(a_L) * d/da_L, over a_L in place (pad columns and rows beyond N: 0)
      float* AL = lds + pl.o_a[pl.L];
      const int ldL = pl.ld[pl.L], Ep = pl.dimp[pl.L];
      for (int e = tid; e < pl.CR * Ep; e += EM_THREADS) {
        const int j = e / Ep, h = e - j * Ep;
        float d = 0.f;
        if (h < E && misc[EM_M_VALID + j] != 0.f) {
          if (POOL) {
            const long long b = (r0 + j) / a.T;
            const float gg = a.grad_out[b * (E + 1) + h];
            d = a.mean ? gg / a.head_in[b * (E + 1) + E] : gg;
          } else {
            d = a.grad_out[(r0 + j) * E + h];
          }
        }
        const float act = AL[j * ldL + h];
        AL[j * ldL + h] = act > 0.f ? d : 0.f;
      }
      __syncthreads();
    }
#pragma unroll
    for (int l = EM_MAXL - 1; l >= 0; --l) {
      if (l < pl.L) {
        if (l == 0) em_dw<0, 4>(pl, lds, l, GW, tid);
        else if (l == pl.L - 1) em_dw<4, 4>(pl, lds, l, GW, tid);
        else if (l == 1) em_dw<8, 8>(pl, lds, l, GW, tid);
        else em_dw<16, 8>(pl, lds, l, GW, tid);
        if (tid < pl.dimp[l + 1]) {
          const float* DZ = lds + pl.o_a[l + 1];
          for (int n = 0; n < pl.CR; ++n) GB[l] += DZ[n * pl.ld[l + 1] + tid];
        }
        if (l > 0) em_da<true>(pl, lds, l, tid);
        else if (a.grad_x != nullptr) em_da<false>(pl, lds, l, tid);
        __syncthreads();
      }
    }
    if (a.grad_x != nullptr) {
      const int F = pl.dim[0];
      const float* X = lds + pl.o_a[0];
      for (int e = tid; e < pl.CR * F; e += EM_THREADS) {
        const int j = e / F, f = e - j * F;
        if (r0 + j < a.N) a.grad_x[(r0 + j) * F + f] = X[j * pl.ld[0] + f];
      }
      __syncthreads();
    }
  }

  // this workgroup's partial gradient
  float* part = a.partial + (long long)blockIdx.x * pl.P;
#pragma unroll
  for (int l = 0; l < EM_MAXL; ++l) {
    if (l < pl.L) {
      if (l == 0) em_dw_store<0, 4>(pl, l, GW, part, tid);
      else if (l == pl.L - 1) em_dw_store<4, 4>(pl, l, GW, part, tid);
      else if (l == 1) em_dw_store<8, 8>(pl, l, GW, part, tid);
      else em_dw_store<16, 8>(pl, l, GW, part, tid);
      if (tid < pl.dim[l + 1]) part[pl.off_b[l] + tid] = GB[l];
    }
  }
}

// grad[i] = sum over workgroups, in workgroup order
__global__ void __launch_bounds__(256)
em_reduce_kernel(const float* __restrict__ partial, int groups, int P, float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float s = 0.f;
  for (int w = 0; w < groups; ++w) s += partial[(long long)w * P + i];
  grad[i] = s;
}

}  // namespace
