/* sbi_amd_resnet.h -- C ABI of the MI355X-native trunk of ResNetEmbedding1D (sbi/neural_nets/embedding_nets/resnet.py):
 * the initial Linear plus every residual block, x (rows, c_in) -> trunk (rows, c_internal).  The head (`final`) is not
 * here: it stays ordinary torch in both routes.
 *
 *   h_0      = x Wi^T + bi                       (or x itself when c_in == c_internal: no initial Linear)
 *   per block: a = relu(h W0^T + b0);  c = relu(a W2^T + b2);  h' = relu(c W4^T + b4 + h)
 *   trunk    = h_{n_blocks}
 *
 * Flat fp32 parameters in state_dict order: initial.weight (c_internal, c_in), initial.bias (c_internal) when
 * c_in != c_internal; then per block f.0.weight (c_hidden, c_internal), f.0.bias, f.2.weight (c_hidden, c_hidden),
 * f.2.bias, f.4.weight (c_internal, c_hidden), f.4.bias.  6 n_blocks (+ 2) entries.
 *
 * Mapping.  Every GEMM runs on v_mfma_f32_16x16x4_f32 (M = row, N = output feature, K = input feature).
 *   - Pack: one launch writes the staged weight image into the workspace: every matrix transposed to (K, N) and
 *     zero-padded to multiples of 16, its bias behind it, and (used by the backward) every block matrix once more in
 *     its own (N, K) orientation.  Widths that are no multiple of 16 are padded here, never refused.
 *   - Forward: ONE launch.  A workgroup (256 threads, 4 waves) owns row tiles of RT rows (16, 32 or 64 by `rows`);
 *     the tile's residual stream and both hidden activations live in LDS for all 3 n_blocks (+ 1) GEMMs.  Weights
 *     stream through LDS as K-panels of KP rows (64 for RT 16 / 32, 32 for RT 64), double-buffered: the next panel's
 *     global loads are issued before the current panel's MFMAs and land in LDS after them, one barrier per panel,
 *     across matrix boundaries too.
 *   - Backward: per block, last to first, a row-parallel delta launch (rebuilds both hidden activations from the
 *     stashed block input, walks the delta back through the three matrices, leaves the five operands of the weight
 *     gradients in the workspace) and a weight-gradient launch (dW = D^T A over the rows as the K dimension: each wave
 *     one 16-row strip of dW over a quarter of the split's rows, the four waves joined in wave order through LDS).
 *     With more than one row split (splits = ceil(Rp / 1024), at most 64) the splits write partial images and a third
 *     launch adds them in split order.  No float atomics.
 *
 * Semantics.  A row's trunk output is one fixed chain of operations: K ascends in steps of 16, the MFMA of step s
 * takes k = 16 c + 4 g + s (g = 0..3), whatever RT is.  It is bitwise the same alone, anywhere in a batch and at any
 * batch size.  Two backward calls give identical bits.  No d/dx.
 *
 * Envelope: 1 <= c_in, c_internal, c_hidden <= 128; 1 <= n_blocks <= 64; 1 <= rows < 2^31 - 64.  Outside it
 * SBI_AMD_E_UNSUPPORTED; zero or negative sizes and null pointers SBI_AMD_E_BADARG (nothing is launched).
 *
 * Workspace in floats, with P(v) = 16 ceil(v / 16), CI = P(c_internal), CH = P(c_hidden), CN = P(c_in),
 * Rp = 64 ceil(rows / 64), BI = 4 CI CH + 2 CH CH + 2 CH + CI (one block's image), II = CN CI + CI (0 without the
 * initial Linear), PB = one block's parameters, PI = the initial Linear's:
 *     inference  II + n_blocks BI
 *     training   + (n_blocks + 1) Rp CI      the stash: every block's input and the trunk output; the two hidden
 *                                            activations are recomputed
 *                + 2 Rp CI + 4 Rp CH         delta stream, dZ; a, c, dA, dC of the block in flight
 *                + splits max(PB, PI)        weight-gradient partials (0 when splits == 1)
 * The forward of a call that needs gradients runs with training = 1 on the workspace the backward is given.
 *
 * Every pointer is a DEVICE pointer unless noted; `stream` is a hipStream_t.  Return value: 0 = launched; < 0 =
 * SBI_AMD_E_* (sbi_amd_nsf.h); > 0 = hipError_t.
 */
#ifndef SBI_AMD_RESNET_H
#define SBI_AMD_RESNET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBI_AMD_RESNET_MAX_WIDTH 128
#define SBI_AMD_RESNET_MAX_BLOCKS 64
#define SBI_AMD_RESNET_MAX_SPLITS 64

typedef struct sbi_amd_resnet_config {
  int32_t c_in;
  int32_t c_internal;
  int32_t c_hidden;
  int32_t n_blocks;
} sbi_amd_resnet_config;

/* Host only.  Number of flat parameters, or SBI_AMD_E_*.  `offsets` (HOST pointer, may be null) receives
 * 6 n_blocks (+ 2 with the initial Linear) entries, the offset of every state_dict entry in order. */
int64_t sbi_amd_resnet_param_count(const sbi_amd_resnet_config* cfg, int64_t* offsets);

/* Host only.  0 or SBI_AMD_E_*.  row_tile: RT.  lds_bytes (2 entries): forward, delta kernel.  splits: row splits of the
 * weight-gradient launches.  Each HOST pointer may be null. */
int sbi_amd_resnet_plan(const sbi_amd_resnet_config* cfg, int64_t rows, int32_t* row_tile, int32_t* lds_bytes,
                        int32_t* splits);

/* Host only.  Bytes of workspace (see above), or SBI_AMD_E_*. */
int64_t sbi_amd_resnet_workspace_bytes(const sbi_amd_resnet_config* cfg, int64_t rows, int32_t training);

/* x (rows, c_in) contiguous; out (rows, c_internal).  training = 1 keeps the stash in `workspace`. */
int sbi_amd_resnet_forward(const sbi_amd_resnet_config* cfg, const float* params, const float* x, int64_t rows,
                           float* out, void* workspace, int32_t training, void* stream);

/* grad_params = d/dparams of sum(out * grad_out), grad_out (rows, c_internal) contiguous, on the workspace a training
 * forward with the same arguments filled. */
int sbi_amd_resnet_backward(const sbi_amd_resnet_config* cfg, const float* params, const float* x, int64_t rows,
                            const float* grad_out, float* grad_params, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
