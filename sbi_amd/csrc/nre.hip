// nre.hip -- neural ratio estimation on the ResNet ratio classifier, C ABI sbi_amd_nre_* (include/sbi_amd_nsf.h, NRE
// section).  Device side of the per-pair passes: nre_kernel.h.  Here: the pack, the deterministic weight-gradient
// reduction, the four trainers' loss-weight launches and the trials sum.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/sbi_amd_nsf.h"
#include "nre_kernel.h"

namespace {

constexpr int kRS = 16;      // rows per LDS sub-chunk of the weight-gradient reduction
constexpr int kAMax = 196;   // >= D + C + 1 rounded up to 4 (D <= 64, C <= 128)
constexpr int kMaxTiles = 4; // 4x4 output tiles per thread: 16 * ceil(197 / 4) = 784 <= 4 * 256

// one thread per pair: a launch covers fewer than 2^32 threads
constexpr int64_t kMaxRows = (1ll << 32) - 256;

int check_cfg(const sbi_amd_nre_config* cfg, NreDims* d) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->D < 1 || cfg->C < 1 || cfg->H < 1 || cfg->NB < 1) return SBI_AMD_E_BADARG;
  if (cfg->D > 64 || cfg->C > 128 || cfg->H > 64 || cfg->NB > 4) return SBI_AMD_E_UNSUPPORTED;
  *d = NreDims{cfg->D, cfg->C, cfg->H, cfg->NB, 0};
  d->HS = d->H > 48 && d->H <= 56 ? 56 : (d->H + 15) / 16 * 16;
  return 0;
}

int hp_of(const NreDims& d) { return d.HS; }   // H rounded up to 16 (sbi's default 50: 56)

// flat (nflows) parameter offsets
__host__ __device__ inline int64_t fl_init_b(const NreDims& d) { return (int64_t)d.H * (d.D + d.C); }
__host__ __device__ inline int64_t fl_blk(const NreDims& d, int b, int lin) {
  return fl_init_b(d) + d.H + (int64_t)(2 * b + lin) * ((int64_t)d.H * d.H + d.H);
}
__host__ __device__ inline int64_t fl_final(const NreDims& d) { return fl_blk(d, d.NB, 0); }
__host__ __device__ inline int64_t fl_count(const NreDims& d) { return fl_final(d) + d.H + 1; }

int64_t packed_floats(const NreDims& d) {
  const int hp = hp_of(d);
  return (int64_t)hp * (1 + d.C + d.D) + (int64_t)2 * d.NB * (hp * hp + hp) + hp + 4;
}

__global__ void __launch_bounds__(256)
nre_pack_kernel(NreDims d, int HP, const float* __restrict__ p, float* __restrict__ pk, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int H = d.H, DC = d.D + d.C;
  const int64_t blk0 = (int64_t)HP * (1 + d.C + d.D);
  const int64_t fin = blk0 + (int64_t)2 * d.NB * (HP * HP + HP);
  float v = 0.f;
  if (e < HP) {
    if (e < H) v = p[fl_init_b(d) + e];
  } else if (e < blk0) {
    const int64_t q = e - HP;
    const int k = (int)(q / HP), i = (int)(q % HP);
    const int col = k < d.C ? d.D + k : k - d.C;     // x columns first in the image, theta columns after
    if (i < H) v = p[(int64_t)i * DC + col];
  } else if (e < fin) {
    const int64_t q = e - blk0;
    const int bl = (int)(q / (HP * HP + HP));
    const int rem = (int)(q % (HP * HP + HP));
    const int64_t base = fl_blk(d, bl >> 1, bl & 1);
    if (rem < HP * HP) {
      const int j = rem / HP, i = rem % HP;
      if (i < H && j < H) v = p[base + (int64_t)i * H + j];
    } else if (rem - HP * HP < H) {
      v = p[base + (int64_t)H * H + (rem - HP * HP)];
    }
  } else if (e < fin + HP) {
    if (e - fin < H) v = p[fl_final(d) + (e - fin)];
  } else if (e == fin + HP) {
    v = p[fl_final(d) + H];
  }
  pk[e] = v;
}

// Weight gradients of one linear layer over one chunk of rows: dW[i][j] = sum_r G[i][r] A[j][r] and db[i] = sum_r G[i][r]
// (the bias as a column of ones next to A), summed over the chunk's rows in ascending order and written -- not added --
// to the chunk's own flat gradient.  Layer L: 0 initial, 1 + 2 b + lin the block linears, 1 + 2 NB the final layer.
__global__ void __launch_bounds__(256)
nre_dw_kernel(NreDims d, int64_t n, int64_t chunk, const float* __restrict__ w, const float* __restrict__ ws,
              float* __restrict__ partials, int64_t P) {
  __shared__ __attribute__((aligned(16))) float As[kRS][kAMax];
  __shared__ __attribute__((aligned(16))) float Gs[kRS][64];
  const int L = blockIdx.y, tid = threadIdx.x;
  const int64_t c = blockIdx.x, r0 = c * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
  int in, out;
  bool relu;
  int64_t arow, grow;      // stash features of A and G (grow < 0: G is the upstream weight w, the final layer)
  int64_t woff, boff;
  if (L == 0) {
    in = d.D + d.C, out = d.H, relu = false, arow = 0, grow = nre_st_g0(d), woff = 0, boff = fl_init_b(d);
  } else if (L <= 2 * d.NB) {
    const int b = (L - 1) >> 1, lin = (L - 1) & 1;
    in = d.H, out = d.H, relu = true;
    arow = lin ? nre_st_u(d, b) : nre_st_h(d, b);
    grow = nre_st_gl(d, b, lin);
    woff = fl_blk(d, b, lin), boff = woff + (int64_t)d.H * d.H;
  } else {
    in = d.H, out = 1, relu = false, arow = nre_st_h(d, d.NB), grow = -1, woff = fl_final(d), boff = woff + d.H;
  }
  const int ntj = (in + 1 + 3) >> 2, nti = (out + 3) >> 2, ntiles = nti * ntj;
  float acc[kMaxTiles][16];
#pragma unroll
  for (int t = 0; t < kMaxTiles; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  for (int64_t rs = r0; rs < r1; rs += kRS) {
    for (int e = tid; e < kRS * 4 * ntj; e += 256) {
      const int k = e / kRS, rr = e % kRS;
      const int64_t row = rs + rr;
      float v = 0.f;
      if (row < r1) {
        if (k < in) {
          v = ws[nre_st_base(d, row) + (arow + k) * 256];
          if (relu) v = v > 0.f ? v : 0.f;
        } else if (k == in) {
          v = 1.f;
        }
      }
      As[rr][k] = v;
    }
    for (int e = tid; e < kRS * 4 * nti; e += 256) {
      const int i = e / kRS, rr = e % kRS;
      const int64_t row = rs + rr;
      Gs[rr][i] = (row < r1 && i < out) ? (grow < 0 ? w[row] : ws[nre_st_base(d, row) + (grow + i) * 256]) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t) {
      const int tile = tid + t * 256;
      if (tile < ntiles) {
        const int ti = tile / ntj, tj = tile % ntj;
        for (int rr = 0; rr < kRS; ++rr) {
          const float4 g4 = *reinterpret_cast<const float4*>(&Gs[rr][4 * ti]);
          const float4 a4 = *reinterpret_cast<const float4*>(&As[rr][4 * tj]);
          const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
          for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[t][ii * 4 + jj] = fmaf(gv[ii], av[jj], acc[t][ii * 4 + jj]);
        }
      }
    }
    __syncthreads();
  }
  float* dst = partials + c * P;
#pragma unroll
  for (int t = 0; t < kMaxTiles; ++t) {
    const int tile = tid + t * 256;
    if (tile >= ntiles) continue;
    const int ti = tile / ntj, tj = tile % ntj;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int i = 4 * ti + ii, j = 4 * tj + jj;
        if (i >= out) continue;
        if (j < in) dst[woff + (int64_t)i * in + j] = acc[t][ii * 4 + jj];
        else if (j == in) dst[boff + i] = acc[t][ii * 4 + jj];
      }
  }
}

// grad[p] = sum over chunks in ascending order: a fixed order, no atomics, bit-identical repeat calls
__global__ void __launch_bounds__(256)
nre_reduce_kernel(const float* __restrict__ partials, int64_t nchunks, int64_t P, float* __restrict__ grad) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  float s = 0.f;
  for (int64_t c = 0; c < nchunks; ++c) s += partials[c * P + p];
  grad[p] = s;
}

// one wave per theta, fp64 lanes + fixed butterfly: the order depends on the trial index alone
__global__ void __launch_bounds__(256)
nre_trials_sum_kernel(const float* __restrict__ rows, int64_t num_trials, int64_t num_theta, float* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= num_theta) return;
  const float* r = rows + c * num_trials;
  double acc = 0.0;
  for (int64_t i = lane; i < num_trials; i += 64) acc += (double)r[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) out[c] = (float)acc;
}

__device__ inline float sigm(float l) { return 1.f / (1.f + expf(-l)); }

// nn.BCELoss on sigmoid(l) for one pair: loss with the log clamped at -100, and d loss / d l the way torch's
// binary_cross_entropy backward and sigmoid backward compose it
__device__ inline void bce_pair(float l, float y, float* loss, float* dl, float* s_out) {
  const float s = sigm(l);
  const float lp = fmaxf(logf(s), -100.f), lq = fmaxf(logf(1.f - s), -100.f);
  *loss = -(y * lp + (1.f - y) * lq);
  const float gp = (s - y) / fmaxf((1.f - s) * s, 1e-12f);
  *dl = gp * ((1.f - s) * s);
  *s_out = s;
}

// BNRE's balancing term couples the batch: per-workgroup sums of sigmoid(l_joint) + sigmoid(l_marginal) - 1 (fixed tree)
__global__ void __launch_bounds__(256)
nre_bnre_parts_kernel(const float* __restrict__ logits, int B, float* __restrict__ parts) {
  __shared__ float red[256];
  const int b = blockIdx.x * 256 + threadIdx.x;
  red[threadIdx.x] = b < B ? sigm(logits[b]) + sigm(logits[B + b]) - 1.f : 0.f;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) parts[blockIdx.x] = red[0];
}

// torch.logsumexp over {add + v[a * stride], a < m} and, when has_extra, the value `extra` (an infinite maximum is
// replaced by 0 before the shift, as torch does)
__device__ inline float lse(const float* v, int m, int64_t stride, float add, bool has_extra, float extra) {
  float mx = has_extra ? extra : -INFINITY;
  for (int a = 0; a < m; ++a) mx = fmaxf(mx, add + v[a * stride]);
  if (!(fabsf(mx) < INFINITY)) mx = 0.f;
  float s = has_extra ? expf(extra - mx) : 0.f;
  for (int a = 0; a < m; ++a) s += expf((add + v[a * stride]) - mx);
  return logf(s) + mx;
}

// one thread per row b; logits atoms-major (atom a of row b at a * B + b)
__global__ void __launch_bounds__(256)
nre_loss_kernel(int mode, const float* __restrict__ logits, int B, int A, float gamma, float lam, float scale,
                float* __restrict__ loss_out, float* __restrict__ w_out, const float* __restrict__ parts, int nparts) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  if (mode == 0 || mode == 3) {
    float l0, l1, d0, d1, s0, s1;
    bce_pair(logits[b], 1.f, &l0, &d0, &s0);
    bce_pair(logits[B + b], 0.f, &l1, &d1, &s1);
    float loss = 0.5f * (l0 + l1);
    d0 *= 0.5f, d1 *= 0.5f;
    if (mode == 3) {
      float sum = 0.f;
      for (int p = 0; p < nparts; ++p) sum += parts[p];
      const float m = sum / (float)B;
      loss += lam * (m * m);
      d0 += lam * 2.f * m * (s0 * (1.f - s0));
      d1 += lam * 2.f * m * (s1 * (1.f - s1));
    }
    loss_out[b] = loss;
    if (w_out) w_out[b] = scale * d0, w_out[B + b] = scale * d1;
    return;
  }
  if (mode == 1) {
    const float* lb = logits + b;
    const float z = lse(lb, A, B, 0.f, false, 0.f);
    loss_out[b] = -(lb[0] - z);
    if (w_out)
      for (int a = 0; a < A; ++a) w_out[(int64_t)a * B + b] = scale * (expf(lb[(int64_t)a * B] - z) - (a == 0 ? 1.f : 0.f));
    return;
  }
  // mode 2, NRE_C: marginal set (K + 1 atoms, atom 0 dropped) then the joint set (K atoms); each denominator is
  // [log gamma + logits ; log K]
  const int K = A - 1;
  const float lg = logf(gamma), lK = logf((float)K);
  const float pj = gamma / (1.f + gamma), pm = 1.f / (1.f + gamma);
  const float* lm = logits + (int64_t)B + b;                  // atoms 1 .. K of the marginal set
  const float* lj = logits + (int64_t)(K + 1) * B + b;
  const float zm = lse(lm, K, B, lg, true, lK);
  const float lpm = lK - zm;
  const float zj = lse(lj, K, B, lg, true, lK);
  const float lpj = lg + lj[0] - zj;
  if (w_out) {
    w_out[b] = 0.f;
    for (int a = 0; a < K; ++a) w_out[(int64_t)(a + 1) * B + b] = scale * pm * expf((lg + lm[(int64_t)a * B]) - zm);
    float* wj = w_out + (int64_t)(K + 1) * B;
    for (int a = 0; a < K; ++a)
      wj[(int64_t)a * B + b] = scale * pj * (expf((lg + lj[(int64_t)a * B]) - zj) - (a == 0 ? 1.f : 0.f));
  }
  loss_out[b] = -(pm * lpm + pj * lpj);
}

template <int HP>
int launch_forward(const NreDims& d, bool train, const float* pk, const float* zs, const float* theta, const float* x,
                   int64_t n, int64_t x_rows, int64_t theta_div, float* out, float* ws, hipStream_t st) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (train)
    hipLaunchKernelGGL((nre_forward_kernel<HP, true, false>), grid, block, 0, st, d, pk, zs, theta, x, n, x_rows,
                       theta_div, out, ws);
  else if (x_rows == 1)
    hipLaunchKernelGGL((nre_forward_kernel<HP, false, true>), grid, block, 0, st, d, pk, zs, theta, x, n, x_rows,
                       theta_div, out, ws);
  else
    hipLaunchKernelGGL((nre_forward_kernel<HP, false, false>), grid, block, 0, st, d, pk, zs, theta, x, n, x_rows,
                       theta_div, out, ws);
  return (int)hipGetLastError();
}

int forward(const NreDims& d, bool train, const float* pk, const float* zs, const float* theta, const float* x,
            int64_t n, int64_t x_rows, int64_t theta_div, float* out, float* ws, hipStream_t st) {
  switch (hp_of(d)) {
    case 16: return launch_forward<16>(d, train, pk, zs, theta, x, n, x_rows, theta_div, out, ws, st);
    case 32: return launch_forward<32>(d, train, pk, zs, theta, x, n, x_rows, theta_div, out, ws, st);
    case 48: return launch_forward<48>(d, train, pk, zs, theta, x, n, x_rows, theta_div, out, ws, st);
    case 56: return launch_forward<56>(d, train, pk, zs, theta, x, n, x_rows, theta_div, out, ws, st);
    default: return launch_forward<64>(d, train, pk, zs, theta, x, n, x_rows, theta_div, out, ws, st);
  }
}

// rows per weight-gradient chunk: about 2 048 workgroups over the layers at large batches, >= 64 rows per chunk
void chunk_plan(const NreDims& d, int64_t n, int64_t* chunk, int64_t* nchunks) {
  const int64_t layers = 2 + 2 * d.NB, target = 2048 / layers;
  int64_t c = (n + target - 1) / target;
  c = (c + kRS - 1) / kRS * kRS;
  if (c < 64) c = 64;
  *chunk = c;
  *nchunks = n > 0 ? (n + c - 1) / c : 0;
}

}  // namespace

extern "C" int64_t sbi_amd_nre_param_count(const sbi_amd_nre_config* cfg) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  return rc ? rc : fl_count(d);
}

extern "C" int64_t sbi_amd_nre_param_offset(const sbi_amd_nre_config* cfg, int32_t layer, int32_t bias) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (layer < 0 || layer > 2 * d.NB + 1 || bias < 0 || bias > 1) return SBI_AMD_E_BADARG;
  if (layer == 0) return bias ? fl_init_b(d) : 0;
  if (layer == 2 * d.NB + 1) return fl_final(d) + (bias ? d.H : 0);
  const int64_t w = fl_blk(d, (layer - 1) >> 1, (layer - 1) & 1);
  return bias ? w + (int64_t)d.H * d.H : w;
}

extern "C" int64_t sbi_amd_nre_packed_floats(const sbi_amd_nre_config* cfg) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  return rc ? rc : packed_floats(d);
}

extern "C" int sbi_amd_nre_pack(const sbi_amd_nre_config* cfg, const float* params, float* packed, void* stream) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (!params || !packed) return SBI_AMD_E_BADARG;
  const int64_t total = packed_floats(d);
  hipLaunchKernelGGL(nre_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d,
                     hp_of(d), params, packed, total);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_nre_log_ratio(const sbi_amd_nre_config* cfg, const float* packed, const float* zstats,
                                     const float* theta, const float* x, int64_t n, int64_t x_rows, float* logit_out,
                                     void* stream) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (n < 0 || x_rows < 1) return SBI_AMD_E_BADARG;
  if (n > kMaxRows) return SBI_AMD_E_UNSUPPORTED;
  if (n == 0) return 0;
  if (!packed || !zstats || !theta || !x || !logit_out) return SBI_AMD_E_BADARG;
  return forward(d, false, packed, zstats, theta, x, n, x_rows, 1, logit_out, nullptr, (hipStream_t)stream);
}

extern "C" int64_t sbi_amd_nre_log_ratio_trials_workspace_floats(const sbi_amd_nre_config* cfg, int64_t num_trials,
                                                                 int64_t num_theta) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (num_trials < 1 || num_theta < 0 || (num_theta > 0 && num_trials > INT64_MAX / num_theta)) return SBI_AMD_E_BADARG;
  if (num_trials * num_theta > kMaxRows) return SBI_AMD_E_UNSUPPORTED;
  return num_trials * num_theta;
}

extern "C" int sbi_amd_nre_log_ratio_trials(const sbi_amd_nre_config* cfg, const float* packed, const float* zstats,
                                            const float* x_trials, int64_t num_trials, const float* theta,
                                            int64_t num_theta, float* sum_out, float* row_out, float* workspace,
                                            void* stream) {
  const int64_t n = sbi_amd_nre_log_ratio_trials_workspace_floats(cfg, num_trials, num_theta);
  if (n < 0) return (int)n;
  if (n == 0) return 0;
  if (!packed || !zstats || !x_trials || !theta || !sum_out || (!row_out && !workspace)) return SBI_AMD_E_BADARG;
  NreDims d;
  check_cfg(cfg, &d);
  float* rows = row_out ? row_out : workspace;
  hipStream_t st = (hipStream_t)stream;
  const int rc = forward(d, false, packed, zstats, theta, x_trials, n, num_trials, num_trials, rows, nullptr, st);
  if (rc) return rc;
  hipLaunchKernelGGL(nre_trials_sum_kernel, dim3((unsigned)((num_theta + 3) / 4)), dim3(256), 0, st,
                     (const float*)rows, num_trials, num_theta, sum_out);
  return (int)hipGetLastError();
}

extern "C" int64_t sbi_amd_nre_train_workspace_floats(const sbi_amd_nre_config* cfg, int64_t n) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (n < 1) return SBI_AMD_E_BADARG;
  if (n > kMaxRows) return SBI_AMD_E_UNSUPPORTED;
  int64_t chunk, nchunks;
  chunk_plan(d, n, &chunk, &nchunks);
  return nre_st_floats(d, n) + nchunks * fl_count(d);
}

extern "C" int sbi_amd_nre_train_forward(const sbi_amd_nre_config* cfg, const float* packed, const float* zstats,
                                         const float* theta, const float* x, int64_t n, int64_t x_rows,
                                         float* logit_out, float* workspace, void* stream) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (n < 1 || x_rows < 1) return SBI_AMD_E_BADARG;
  if (n > kMaxRows) return SBI_AMD_E_UNSUPPORTED;
  if (!packed || !zstats || !theta || !x || !logit_out || !workspace) return SBI_AMD_E_BADARG;
  return forward(d, true, packed, zstats, theta, x, n, x_rows, 1, logit_out, workspace, (hipStream_t)stream);
}

extern "C" int sbi_amd_nre_train_backward(const sbi_amd_nre_config* cfg, const float* packed, const float* zstats,
                                          int64_t n, const float* weights, float* grad_out, float* grad_theta_out,
                                          float* workspace, void* stream) {
  NreDims d;
  const int rc = check_cfg(cfg, &d);
  if (rc) return rc;
  if (n < 1) return SBI_AMD_E_BADARG;
  if (n > kMaxRows) return SBI_AMD_E_UNSUPPORTED;
  if (!packed || !zstats || !weights || !grad_out || !workspace) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  switch (hp_of(d)) {
    case 16: hipLaunchKernelGGL(nre_backward_kernel<16>, grid, block, 0, st, d, packed, zstats, n, weights, grad_theta_out, workspace); break;
    case 32: hipLaunchKernelGGL(nre_backward_kernel<32>, grid, block, 0, st, d, packed, zstats, n, weights, grad_theta_out, workspace); break;
    case 48: hipLaunchKernelGGL(nre_backward_kernel<48>, grid, block, 0, st, d, packed, zstats, n, weights, grad_theta_out, workspace); break;
    case 56: hipLaunchKernelGGL(nre_backward_kernel<56>, grid, block, 0, st, d, packed, zstats, n, weights, grad_theta_out, workspace); break;
    default: hipLaunchKernelGGL(nre_backward_kernel<64>, grid, block, 0, st, d, packed, zstats, n, weights, grad_theta_out, workspace); break;
  }
  int64_t chunk, nchunks;
  chunk_plan(d, n, &chunk, &nchunks);
  const int64_t P = fl_count(d);
  float* partials = workspace + nre_st_floats(d, n);
  hipLaunchKernelGGL(nre_dw_kernel, dim3((unsigned)nchunks, (unsigned)(2 + 2 * d.NB)), dim3(256), 0, st, d, n, chunk,
                     weights, (const float*)workspace, partials, P);
  hipLaunchKernelGGL(nre_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (const float*)partials,
                     nchunks, P, grad_out);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_nre_loss_weights(int32_t mode, const float* logits, int32_t batch, int32_t num_atoms,
                                        float gamma, float reg_strength, float scale, float* loss_out,
                                        float* weights_out, float* scratch, void* stream) {
  if (mode < 0 || mode > 3 || batch < 1 || !logits || !loss_out) return SBI_AMD_E_BADARG;
  if ((int64_t)batch * num_atoms > kMaxRows) return SBI_AMD_E_UNSUPPORTED;
  if ((mode == 0 || mode == 3) && num_atoms != 2) return SBI_AMD_E_BADARG;
  if (mode == 1 && (num_atoms < 1 || num_atoms > 1024)) return SBI_AMD_E_UNSUPPORTED;
  if (mode == 2 && (num_atoms < 2 || num_atoms > 1024 || !(gamma > 0.f))) return num_atoms > 1024 ? SBI_AMD_E_UNSUPPORTED
                                                                                                    : SBI_AMD_E_BADARG;
  if (mode == 3 && !scratch) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((batch + 255) / 256);
  if (mode == 3) hipLaunchKernelGGL(nre_bnre_parts_kernel, dim3(blocks), dim3(256), 0, st, logits, batch, scratch);
  hipLaunchKernelGGL(nre_loss_kernel, dim3(blocks), dim3(256), 0, st, (int)mode, logits, batch, num_atoms, gamma,
                     reg_strength, scale, loss_out, weights_out, (const float*)scratch, (int)blocks);
  return (int)hipGetLastError();
}
