// Micro-benchmark: v_mfma_f32_4x4x1_16b_f32 (__builtin_amdgcn_mfma_f32_4x4x1f32) on gfx950, the candidate instruction
// for the thin remainder tiles of the 50-wide hidden layers (features 48, 49 of a 64-wide padding).
//   1. Lane maps, probed one lane at a time (A or B = 1 in lane p only, the other operand all ones), then checked on
//      random data against a host evaluation.  Hypothesis: 16 blocks of 4x4x1; lane l supplies A[m = l & 3] and
//      B[n = l & 3] of block b = l >> 2; D[m][n] of block b is lane 4 b + n, register m.
//   2. Rounding: a 16x16x4 f32 MFMA against a chain of fmaf over its k-slots 0..3 (C first), a 4x4x1 one against one
//      fmaf -- bit for bit, on random operands spanning 12 binades (what makes a 4x4x1 path bit-identical to a 16x16x4 one).
//   3. Issue cost: back-to-back MFMAs on 4 independent accumulators and on one dependent accumulator, at 1 and 2
//      waves per SIMD (every CU busy), against v_mfma_f32_16x16x4_f32 under the same loop.  Cycles from
//      s_memtime per wave (shader clock), reported per instruction and per SIMD.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o mfma_4x4 mfma_4x4.hip ; run: ./mfma_4x4
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                               \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) {                                                                    \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
      exit(1);                                                                                 \
    }                                                                                          \
  } while (0)

// one MFMA of one wave: out[lane][r] = D register r of lane `lane` for A = a[lane], B = b[lane], C = 0
__global__ void one4x4(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out) {
  const int l = threadIdx.x;
  f4 d = {0.f, 0.f, 0.f, 0.f};
  d = __builtin_amdgcn_mfma_f32_4x4x1f32(a[l], b[l], d, 0, 0, 0);
  for (int r = 0; r < 4; ++r) out[l * 4 + r] = d[r];
}

// OP 0: 4x4x1_16b, OP 1: 16x16x4.  DEP: one accumulator (dependent chain) instead of four.
template <int OP, bool DEP>
__global__ void __launch_bounds__(512) issue(float a0, float b0, float* __restrict__ sink, long long* __restrict__ cyc,
                                             int iters) {
  const int l = threadIdx.x & 63;
  float a = a0 + 1e-7f * l, b = b0 - 1e-7f * l;
  f4 acc[4];
  for (int i = 0; i < 4; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = DEP ? 0 : (u & 3);
      if (OP == 0) acc[i] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, acc[i], 0, 0, 0);
      else acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
    }
  }
  const long long t1 = __builtin_readcyclecounter();
  float s = 0.f;
  for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  sink[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (l == 0) cyc[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
}

static bool probe_maps() {
  float *da, *db, *dout;
  CHECK(hipMalloc(&da, 64 * 4));
  CHECK(hipMalloc(&db, 64 * 4));
  CHECK(hipMalloc(&dout, 256 * 4));
  std::vector<float> a(64), b(64), out(256);
  bool okA = true, okB = true;
  for (int side = 0; side < 2; ++side)
    for (int p = 0; p < 64; ++p) {
      for (int l = 0; l < 64; ++l) {
        a[l] = side == 0 ? (l == p ? 1.f : 0.f) : 1.f;
        b[l] = side == 1 ? (l == p ? 1.f : 0.f) : 1.f;
      }
      CHECK(hipMemcpy(da, a.data(), 256, hipMemcpyHostToDevice));
      CHECK(hipMemcpy(db, b.data(), 256, hipMemcpyHostToDevice));
      one4x4<<<1, 64>>>(da, db, dout);
      CHECK(hipMemcpy(out.data(), dout, 1024, hipMemcpyDeviceToHost));
      // expected: A from lane p feeds D[m = p & 3][n] of block p >> 2 = lanes 4 (p >> 2) + n, register p & 3;
      //           B from lane p feeds D[m][n = p & 3] of block p >> 2 = lane p, every register
      for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) {
          const bool want = side == 0 ? ((l >> 2) == (p >> 2) && r == (p & 3)) : (l == p);
          if ((out[l * 4 + r] != 0.f) != want) (side == 0 ? okA : okB) = false;
        }
    }
  // random data against the host evaluation of the hypothesised map
  srand(7);
  for (int l = 0; l < 64; ++l) {
    a[l] = (float)rand() / (float)RAND_MAX - 0.5f;
    b[l] = (float)rand() / (float)RAND_MAX - 0.5f;
  }
  CHECK(hipMemcpy(da, a.data(), 256, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, b.data(), 256, hipMemcpyHostToDevice));
  one4x4<<<1, 64>>>(da, db, dout);
  CHECK(hipMemcpy(out.data(), dout, 1024, hipMemcpyDeviceToHost));
  double err = 0.0;
  for (int blk = 0; blk < 16; ++blk)
    for (int m = 0; m < 4; ++m)
      for (int n = 0; n < 4; ++n)
        err = std::max(err, std::fabs((double)out[(4 * blk + n) * 4 + m] - (double)a[4 * blk + m] * b[4 * blk + n]));
  printf("lane maps (16 blocks of 4x4x1):\n");
  printf("  A: lane l -> A[m = l & 3] of block l >> 2 ...................... %s\n", okA ? "confirmed" : "MISMATCH");
  printf("  B: lane l -> B[n = l & 3] of block l >> 2 ...................... %s\n", okB ? "confirmed" : "MISMATCH");
  printf("  D: D[m][n] of block b -> lane 4 b + n, register m, random data: max |err| = %.3g %s\n", err,
         err < 1e-6 ? "(exact)" : "MISMATCH");
  CHECK(hipFree(da));
  CHECK(hipFree(db));
  CHECK(hipFree(dout));
  return okA && okB && err < 1e-6;
}

__global__ void one16x16(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                         float* __restrict__ out, int four) {
  const int l = threadIdx.x, o = blockIdx.x * 64 + l;
  f4 d = {c[o * 4], c[o * 4 + 1], c[o * 4 + 2], c[o * 4 + 3]};
  d = four ? __builtin_amdgcn_mfma_f32_4x4x1f32(a[o], b[o], d, 0, 0, 0)
           : __builtin_amdgcn_mfma_f32_16x16x4f32(a[o], b[o], d, 0, 0, 0);
  for (int r = 0; r < 4; ++r) out[o * 4 + r] = d[r];
}
static bool probe_rounding() {
  const int NB = 2048, n = NB * 64;
  std::vector<float> a(n), b(n), c(n * 4), d(n * 4);
  srand(3);
  auto rnd = [] { return ((float)rand() / (float)RAND_MAX - 0.5f) * std::ldexp(1.f, rand() % 12 - 6); };
  for (auto& v : a) v = rnd();
  for (auto& v : b) v = rnd();
  for (auto& v : c) v = rnd();
  float *da, *db, *dc, *dd;
  CHECK(hipMalloc(&da, n * 4));
  CHECK(hipMalloc(&db, n * 4));
  CHECK(hipMalloc(&dc, n * 16));
  CHECK(hipMalloc(&dd, n * 16));
  CHECK(hipMemcpy(da, a.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, b.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dc, c.data(), n * 16, hipMemcpyHostToDevice));
  long bad16 = 0, bad4 = 0;
  one16x16<<<NB, 64>>>(da, db, dc, dd, 0);
  CHECK(hipMemcpy(d.data(), dd, n * 16, hipMemcpyDeviceToHost));
  for (int o = 0; o < n; ++o)      // lane (n = l & 15, k = l >> 4) supplies A[m = l & 15][k], B[k][n]; D reg r: m = 4 (l >> 4) + r
    for (int r = 0; r < 4; ++r) {
      const int base = o & ~63, l = o & 63, nn = l & 15, mm = 4 * (l >> 4) + r;
      float s = c[o * 4 + r];
      for (int k = 0; k < 4; ++k) s = std::fmaf(a[base + 16 * k + mm], b[base + 16 * k + nn], s);
      bad16 += (s != d[o * 4 + r]);
    }
  one16x16<<<NB, 64>>>(da, db, dc, dd, 1);
  CHECK(hipMemcpy(d.data(), dd, n * 16, hipMemcpyDeviceToHost));
  for (int o = 0; o < n; ++o)
    for (int m = 0; m < 4; ++m) {
      const int base = o & ~63, l = o & 63, blk = l >> 2, nn = l & 3;
      bad4 += (std::fmaf(a[base + 4 * blk + m], b[base + 4 * blk + nn], c[o * 4 + m]) != d[o * 4 + m]);
    }
  printf("\nrounding (%d outputs each, operands over 12 binades):\n", n * 4);
  printf("  16x16x4 f32 == fmaf chain over k = 0, 1, 2, 3 starting from C: %ld mismatches\n", bad16);
  printf("  4x4x1_16b  == fmaf(A, B, C):                                   %ld mismatches\n", bad4);
  CHECK(hipFree(da));
  CHECK(hipFree(db));
  CHECK(hipFree(dc));
  CHECK(hipFree(dd));
  return bad16 == 0 && bad4 == 0;
}

template <int OP, bool DEP>
static double time_issue(int waves_per_simd, int iters) {
  const int nblocks = 256, threads = 256 * waves_per_simd, nw = threads / 64;
  float* sink;
  long long* cyc;
  CHECK(hipMalloc(&sink, (size_t)nblocks * threads * 4));
  CHECK(hipMalloc(&cyc, (size_t)nblocks * nw * 8));
  issue<OP, DEP><<<nblocks, threads>>>(0.5f, 0.25f, sink, cyc, iters);   // warm-up
  issue<OP, DEP><<<nblocks, threads>>>(0.5f, 0.25f, sink, cyc, iters);
  CHECK(hipDeviceSynchronize());
  std::vector<long long> c((size_t)nblocks * nw);
  CHECK(hipMemcpy(c.data(), cyc, c.size() * 8, hipMemcpyDeviceToHost));
  std::sort(c.begin(), c.end());
  CHECK(hipFree(sink));
  CHECK(hipFree(cyc));
  return (double)c[c.size() / 2] / (16.0 * iters);   // median cycles per MFMA of one wave
}

int main() {
  const bool maps = probe_maps();
  const bool rounding = probe_rounding();
  const int iters = 4096;
  printf("\nback-to-back issue, 256 workgroups (every CU), cycles per MFMA (median wave; s_memtime):\n");
  printf("  %-28s %-14s %12s %12s %14s\n", "instruction", "accumulators", "waves/SIMD", "per wave", "per SIMD");
  for (int w = 1; w <= 2; ++w) {
    const double c4i = time_issue<0, false>(w, iters), c4d = time_issue<0, true>(w, iters);
    const double c16i = time_issue<1, false>(w, iters), c16d = time_issue<1, true>(w, iters);
    printf("  %-28s %-14s %12d %12.2f %14.2f\n", "v_mfma_f32_4x4x1_16b_f32", "4 independent", w, c4i, c4i / w);
    printf("  %-28s %-14s %12d %12.2f %14.2f\n", "v_mfma_f32_4x4x1_16b_f32", "1 dependent", w, c4d, c4d / w);
    printf("  %-28s %-14s %12d %12.2f %14.2f\n", "v_mfma_f32_16x16x4_f32", "4 independent", w, c16i, c16i / w);
    printf("  %-28s %-14s %12d %12.2f %14.2f\n", "v_mfma_f32_16x16x4_f32", "1 dependent", w, c16d, c16d / w);
  }
  printf("\n(FLOPs per instruction: 4x4x1_16b 512, 16x16x4 2048)\n");
  return maps && rounding ? 0 : 1;
}
