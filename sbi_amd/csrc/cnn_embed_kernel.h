// cnn_embed_kernel.h -- the convolution stack of CNNEmbedding on gfx950: plan, device functions, kernels (launchers:
// cnn_embed.hip).  Contract: include/sbi_amd_cnn.h.
//
// Execution model
//   * a workgroup is 16 waves and owns whole samples: b = group, group + G, ...  The flat parameters are staged once
//     per workgroup in LDS; the sample's input map of EVERY layer lives in LDS with a zero border (the padding), written
//     once per launch: a sample only overwrites the interiors.  Nothing of a map's size goes to global memory.
//   * direct VALU convolution.  With 6 / 12 output channels a 16-row MFMA tile is mostly padding and the f32-input
//     MFMA runs at the VALU rate anyway.  One thread owns one POOLED output (co, py, px): it runs the PH x PW conv
//     outputs of its window as PH x PW independent fma chains (bias first, then ci, ky, kx), reading each weight once
//     (a broadcast: the lanes of a wave share co except at a channel boundary), then ReLU and the max in row-major
//     window order.  The last layer's pooled outputs go straight to `features`, coalesced.
//   * a map's row stride is its padded width rounded up to odd, so rows and channels never line up on one LDS bank.
//     Neighbouring lanes read addresses PW apart (the pool stride): a PW-way conflict on the 32-bank b32 reads of the
//     input; the weight read of every tap is a broadcast.  Not removed: see DESIGN.md section 7r.
//   * backward: the forward is recomputed and keeps, per pooled output, the offset of the selected conv output (-1: the
//     ReLU is off).  Then per layer, last to first: the gated gradient G of the pooled outputs; one thread per weight /
//     bias walks the pooled positions in order and adds G x (input at the selected window's tap) onto its own LDS
//     accumulator (no two threads share one: no atomics); for l >= 1 the gradient is scattered to a dense conv-output
//     map (one element per pool window, windows are disjoint) and gathered back through the weights to the layer's
//     input, which is the next G.  Each workgroup writes its accumulators to the workspace; a second kernel adds the
//     partials in workgroup order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_cnn.h"
#include "../../include/sbi_amd_nsf.h"

namespace {

#define CN_THREADS 1024
#define CN_MAXL 4
#define CN_GROUPS 512               // most workgroups of a launch: samples beyond walk the grid again
#define CN_MAX_BATCH 1024           // larger batches measured slower than eager torch (README, CNN embedding): refused
#define CN_LDS_BUDGET (160 * 1024)
#define CN_MAX_EXTENT (1 << 20)

struct CnLayer {
  int cin, cout;
  int H, W;                // input extents (H = 1 in 1-D)
  int RS, CS;              // input map in LDS: row stride, channel stride (floats)
  int HC, WC, HP, WP;      // conv and pool output extents
  int off_w, off_b;        // flat parameter offsets
  int o_a, o_sel;          // LDS offsets (floats): input map; selections (relative to the plan's o_sel)
};

struct CnPlan {
  int L, k, KH, PH, PW, pad_y;     // KH = PH = 1, pad_y = 0 in 1-D
  CnLayer ly[CN_MAXL];
  int P, F, in_floats;             // parameters, features per sample, floats of one sample of x
  int o_maps, maps_floats;         // LDS (floats): all input maps, behind the P weights at 0
  int o_acc, o_sel, o_G, o_D;      // backward only
  long long fwd_floats, bwd_floats, F64;   // F64: F before it is narrowed (host-side answers)
};

static int cn_odd(int n) { return n | 1; }

// Everything but the LDS verdict.  long long throughout: an extent of 2^20 must not wrap before it is refused.
static int cn_plan_sizes(const sbi_amd_cnn_config* cfg, CnPlan* out) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->ndim < 1 || cfg->ndim > 2 || cfg->in_channels < 1 || cfg->num_conv_layers < 1 || cfg->kernel_size < 1 ||
      cfg->pool_kernel_size < 1 || cfg->spatial[0] < 1 || (cfg->ndim == 2 && cfg->spatial[1] < 1))
    return SBI_AMD_E_BADARG;
  if (cfg->num_conv_layers > CN_MAXL) return SBI_AMD_E_UNSUPPORTED;
  for (int l = 0; l < cfg->num_conv_layers; ++l)
    if (cfg->out_channels[l] < 1) return SBI_AMD_E_BADARG;
  if (cfg->in_channels > 8 || cfg->kernel_size > 7 || cfg->pool_kernel_size < 2 || cfg->pool_kernel_size > 4 ||
      cfg->spatial[0] > CN_MAX_EXTENT || (cfg->ndim == 2 && cfg->spatial[1] > CN_MAX_EXTENT))
    return SBI_AMD_E_UNSUPPORTED;
  for (int l = 0; l < cfg->num_conv_layers; ++l)
    if (cfg->out_channels[l] > 32) return SBI_AMD_E_UNSUPPORTED;
  CnPlan p = {};
  const bool two = cfg->ndim == 2;
  p.L = cfg->num_conv_layers;
  p.k = cfg->kernel_size;
  p.KH = two ? p.k : 1;
  p.PW = cfg->pool_kernel_size;
  p.PH = two ? p.PW : 1;
  p.pad_y = two ? 1 : 0;
  long long off = 0, maps = 0, sel = 0, gmax = 0, dmax = 0;
  int H = two ? cfg->spatial[0] : 1, W = two ? cfg->spatial[1] : cfg->spatial[0], C = cfg->in_channels;
  p.in_floats = 0;
  for (int l = 0; l < p.L; ++l) {
    CnLayer& y = p.ly[l];
    y.cin = C; y.cout = cfg->out_channels[l];
    y.H = H; y.W = W;
    y.RS = cn_odd(W + 2);
    const long long cs = (long long)(H + 2 * p.pad_y) * y.RS;
    y.HC = H + 2 * p.pad_y - p.KH + 1; y.WC = W + 3 - p.k;
    if (y.HC < 1 || y.WC < 1) return SBI_AMD_E_BADARG;
    y.HP = y.HC / p.PH; y.WP = y.WC / p.PW;
    if (y.HP < 1 || y.WP < 1) return SBI_AMD_E_BADARG;
    const long long pooled = (long long)y.cout * y.HP * y.WP, conv = (long long)y.cout * y.HC * y.WC;
    // an image this large is refused below; the int fields only have to hold what can be resident
    if (cs * C > (1ll << 28) || pooled > (1ll << 28) || conv > (1ll << 28)) {
      maps = sel = 1ll << 40;
    }
    y.CS = (int)(cs > (1ll << 28) ? (1ll << 28) : cs);
    y.off_w = (int)off; off += (long long)y.cout * y.cin * p.KH * p.k;
    y.off_b = (int)off; off += y.cout;
    y.o_a = (int)(maps < (1ll << 30) ? maps : 0); maps += cs * C;
    y.o_sel = (int)(sel < (1ll << 30) ? sel : 0); sel += pooled;
    if (pooled > gmax) gmax = pooled;
    if (l >= 1 && conv > dmax) dmax = conv;
    if (l == 0) p.in_floats = (int)((long long)C * H * W < (1ll << 30) ? (long long)C * H * W : 0);
    C = y.cout; H = y.HP; W = y.WP;
  }
  p.P = (int)off;
  p.F64 = (long long)C * H * W;
  p.F = (int)((long long)C * H * W < (1ll << 30) ? (long long)C * H * W : 0);
  p.fwd_floats = off + maps;
  p.bwd_floats = p.fwd_floats + off + sel + gmax + dmax;
  if (p.bwd_floats * 4 <= CN_LDS_BUDGET) {
    p.o_maps = p.P;
    p.maps_floats = (int)maps;
    for (int l = 0; l < p.L; ++l) p.ly[l].o_a += p.o_maps;
    p.o_acc = p.o_maps + p.maps_floats;
    p.o_sel = p.o_acc + p.P;
    p.o_G = p.o_sel + (int)sel;
    p.o_D = p.o_G + (int)gmax;
  }
  *out = p;
  return 0;
}

static int cn_build_plan(const sbi_amd_cnn_config* cfg, CnPlan* pl) {
  const int rc = cn_plan_sizes(cfg, pl);
  if (rc) return rc;
  return pl->bwd_floats * 4 <= CN_LDS_BUDGET ? 0 : SBI_AMD_E_LDS;
}

static int cn_groups(long long B) { return (int)(B < CN_GROUPS ? B : CN_GROUPS); }

struct CnArgs {
  const float* params;
  const float* x;
  const float* grad_features;
  float* features;
  float* partial;
  long long B;
};

// x[b] -> the interior of layer 0's map
__device__ __forceinline__ void cn_load_x(const CnPlan& pl, const float* __restrict__ xb, float* lds) {
  const CnLayer& y = pl.ly[0];
  float* a = lds + y.o_a;
  const int hw = y.H * y.W;
  for (int i = threadIdx.x; i < pl.in_floats; i += CN_THREADS) {
    const int c = i / hw, r = i - c * hw, yy = r / y.W, xx = r - yy * y.W;
    a[c * y.CS + (yy + pl.pad_y) * y.RS + xx + 1] = xb[i];
  }
}

// layer l: conv + ReLU + max-pool of the sample in LDS.  `next`: the next layer's map (LDS) or null; `gout`: this
// sample's feature row (global) or null; `sel`: selections (LDS) or null.
template <int PH, int PW>
__device__ __forceinline__ void cn_stage(const CnPlan& pl, int l, const float* lds, float* next, float* gout, int* sel) {
  const CnLayer& y = pl.ly[l];
  const int npool = y.HP * y.WP, items = y.cout * npool, KH = pl.KH, k = pl.k, RS = y.RS;
  const float* in = lds + y.o_a;
  for (int idx = threadIdx.x; idx < items; idx += CN_THREADS) {
    const int co = idx / npool, rem = idx - co * npool, py = rem / y.WP, px = rem - py * y.WP;
    const float* w = lds + y.off_w + co * y.cin * KH * k;
    const float bias = lds[y.off_b + co];
    float acc[PH * PW];
#pragma unroll
    for (int e = 0; e < PH * PW; ++e) acc[e] = bias;
    const float* base = in + py * PH * RS + px * PW;
    for (int ci = 0; ci < y.cin; ++ci)
      for (int ky = 0; ky < KH; ++ky) {
        const float* row = base + ci * y.CS + ky * RS;
        for (int kx = 0; kx < k; ++kx) {
          const float wv = *w++;
#pragma unroll
          for (int wy = 0; wy < PH; ++wy)
#pragma unroll
            for (int wx = 0; wx < PW; ++wx) acc[wy * PW + wx] = fmaf(wv, row[wy * RS + wx + kx], acc[wy * PW + wx]);
        }
      }
    float m = 0.f;
    int am = 0;
#pragma unroll
    for (int e = 0; e < PH * PW; ++e) {
      float r = acc[e];
      r = r > 0.f ? r : (r != r ? r : 0.f);
      if (e == 0 || r > m || r != r) { m = r; am = e; }
    }
    if (next) {
      const CnLayer& n = pl.ly[l + 1];
      next[co * n.CS + (py + pl.pad_y) * n.RS + px + 1] = m;
    }
    if (gout) gout[idx] = m;
    if (sel) sel[idx] = m > 0.f ? (py * PH + am / PW) * RS + px * PW + am % PW : -1;
  }
}

// stage the parameters, zero everything else of the image (the maps' borders stay zero for the whole launch)
__device__ __forceinline__ void cn_prologue(const CnPlan& pl, const float* __restrict__ params, float* lds, int floats) {
  for (int i = threadIdx.x; i < pl.P; i += CN_THREADS) lds[i] = params[i];
  for (int i = pl.P + threadIdx.x; i < floats; i += CN_THREADS) lds[i] = 0.f;
  __syncthreads();
}

template <int PH, int PW>
__global__ __launch_bounds__(CN_THREADS) void cn_forward_kernel(CnPlan pl, CnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  cn_prologue(pl, a.params, lds, pl.o_maps + pl.maps_floats);
  for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
    cn_load_x(pl, a.x + b * pl.in_floats, lds);
    __syncthreads();
    for (int l = 0; l < pl.L; ++l) {
      const bool last = l == pl.L - 1;
      cn_stage<PH, PW>(pl, l, lds, last ? nullptr : lds + pl.ly[l + 1].o_a, last ? a.features + b * pl.F : nullptr,
                       nullptr);
      __syncthreads();
    }
  }
}

template <int PH, int PW>
__global__ __launch_bounds__(CN_THREADS) void cn_backward_kernel(CnPlan pl, CnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  cn_prologue(pl, a.params, lds, (int)pl.bwd_floats);
  float* acc = lds + pl.o_acc;
  float* G = lds + pl.o_G;
  float* D = lds + pl.o_D;
  const int KH = pl.KH, k = pl.k;
  for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {
    cn_load_x(pl, a.x + b * pl.in_floats, lds);
    __syncthreads();
    for (int l = 0; l < pl.L; ++l) {
      cn_stage<PH, PW>(pl, l, lds, l == pl.L - 1 ? nullptr : lds + pl.ly[l + 1].o_a, nullptr,
                       (int*)(lds + pl.o_sel) + pl.ly[l].o_sel);
      __syncthreads();
    }
    {   // the gated gradient of the last layer's pooled outputs
      const int* sel = (const int*)(lds + pl.o_sel) + pl.ly[pl.L - 1].o_sel;
      const float* gf = a.grad_features + b * pl.F;
      for (int i = threadIdx.x; i < pl.F; i += CN_THREADS) G[i] = sel[i] >= 0 ? gf[i] : 0.f;
    }
    __syncthreads();
    for (int l = pl.L - 1; l >= 0; --l) {
      const CnLayer& y = pl.ly[l];
      const int* sel = (const int*)(lds + pl.o_sel) + y.o_sel;
      const float* in = lds + y.o_a;
      const int npool = y.HP * y.WP, taps = y.cin * KH * k, nw = y.cout * taps;
      // weights and biases: one thread per element, pooled positions in order
      for (int e = threadIdx.x; e < nw + y.cout; e += CN_THREADS) {
        float s = 0.f;
        if (e < nw) {
          const int co = e / taps, r = e - co * taps, ci = r / (KH * k), r2 = r - ci * KH * k, ky = r2 / k,
                    kx = r2 - ky * k;
          const float* tap = in + ci * y.CS + ky * y.RS + kx;
          const float* g = G + co * npool;
          const int* sl = sel + co * npool;
#pragma unroll 4
          for (int p = 0; p < npool; ++p) {
            const int o = sl[p];
            s = fmaf(g[p], tap[o < 0 ? 0 : o], s);
          }
        } else {
          const float* g = G + (e - nw) * npool;
#pragma unroll 4
          for (int p = 0; p < npool; ++p) s += g[p];
        }
        acc[y.off_w + e] += s;
      }
      if (l == 0) break;     // uniform: no d/dx
      const int conv = y.HC * y.WC;
      for (int i = threadIdx.x; i < y.cout * conv; i += CN_THREADS) D[i] = 0.f;
      __syncthreads();
      for (int i = threadIdx.x; i < y.cout * npool; i += CN_THREADS) {
        const int o = sel[i];
        if (o >= 0) {
          const int oy = o / y.RS, ox = o - oy * y.RS;
          D[(i / npool) * conv + oy * y.WC + ox] = G[i];
        }
      }
      __syncthreads();
      // d/d(input of layer l), gated by layer l - 1's selections: the next G
      const int* selb = (const int*)(lds + pl.o_sel) + pl.ly[l - 1].o_sel;
      const float* wl = lds + y.off_w;
      const int hw = y.H * y.W;
      for (int i = threadIdx.x; i < y.cin * hw; i += CN_THREADS) {
        const int ci = i / hw, r = i - ci * hw, iy = r / y.W, ix = r - iy * y.W;
        float s = 0.f;
        for (int co = 0; co < y.cout; ++co)
          for (int ky = 0; ky < KH; ++ky) {
            const int oy = iy + pl.pad_y - ky;
            if (oy < 0 || oy >= y.HC) continue;
            const float* d = D + co * conv + oy * y.WC;
            const float* w = wl + ((co * y.cin + ci) * KH + ky) * k;
            for (int kx = 0; kx < k; ++kx) {
              const int ox = ix + 1 - kx;
              if (ox >= 0 && ox < y.WC) s = fmaf(d[ox], w[kx], s);
            }
          }
        G[i] = selb[i] >= 0 ? s : 0.f;
      }
      __syncthreads();
    }
    __syncthreads();
  }
  float* part = a.partial + (long long)blockIdx.x * pl.P;
  for (int i = threadIdx.x; i < pl.P; i += CN_THREADS) part[i] = acc[i];
}

// grad[i] = sum over workgroups, in workgroup order
__global__ __launch_bounds__(256) void cn_reduce_kernel(const float* __restrict__ partial, int groups, int P,
                                                        float* __restrict__ grad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float s = 0.f;
  for (int g = 0; g < groups; ++g) s += partial[(long long)g * P + i];
  grad[i] = s;
}

}  // namespace
