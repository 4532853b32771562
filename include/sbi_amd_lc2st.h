/* sbi_amd_lc2st.h -- C ABI of the MI355X-native L-C2ST classifier ensemble (sbi/diagnostics/lc2st.py).
 *
 * One local classifier two-sample test trains (1 + num_trials_null) x num_folds x num_ensemble small binary MLPs
 * ("members") on one shared data matrix; a null trial differs from the observed classifier only in its labels.  The
 * members are independent, and one member's weights fit one workgroup's LDS, so one persistent workgroup per member
 * runs whole epochs -- forward, backward, Adam, validation, early stopping -- with no host in the loop and no
 * synchronisation between workgroups.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless noted;
 * `stream` is a hipStream_t.  Return value: 0 = launched; < 0 = SBI_AMD_E_* (sbi_amd_nsf.h; nothing launched);
 * > 0 = hipError_t.
 *
 * Network of a member (the reference's MLPClassifierModule, sbi/utils/metrics.py): Linear(F, H), ReLU, Linear(H, H),
 * ReLU, Linear(H, 1) on rows [theta, x], F = D + Dx.  Flat parameters per member in torch's order under the
 * reference's key names: sequential.0.weight (H, F), sequential.0.bias (H), sequential.2.weight (H, H),
 * sequential.2.bias (H), sequential.4.weight (1, H), sequential.4.bias (1): P = H F + H H + 3 H + 1 floats.
 * Envelope: 1 <= D, 1 <= Dx, F <= 64, 1 <= H <= 128, two hidden layers of equal width; anything else is
 * SBI_AMD_E_UNSUPPORTED.  Inside the kernels H and F are zero-padded to multiples of 16 (F needs a multiple of 4 for the
 * MFMA's K step; 16 makes the weight-gradient tiles whole); pad entries are zeros that no update touches.
 *
 * Data: `data` (R x F, fp32, shared).  Member m owns the row list rows[m * row_stride + i] (int32 indices into data;
 * an index outside [0, R) reads as a row of zeros, never out of bounds) with the aligned labels[m * row_stride + i]
 * (0 / 1 floats): the first n_train[m] entries are its training rows, the next n_valid[m] (>= 1) its validation rows;
 * n_train[m] + n_valid[m] <= row_stride is required (a member that violates it is marked stopped untrained, and
 * batch_grad answers NaN / 0 for it: no list is read past its stride).
 *
 * Epoch e of member m: position i of the epoch is entry pi(i) of the row list, pi = the keyed Feistel permutation of
 * csrc/shuffle_prp.h on [0, n_train), 64-bit key = words 0 (low) and 1 (high) of Philox4x32-10 with counter
 * (e, 0, member_id[m], 0x4C433253) and key (seed low, seed high): a member's stream depends on its id, not its slot.
 * Batch b covers positions [b B, min((b + 1) B, n_train)); the last batch may be short and is kept (drop_last=False).
 * One step: loss = mean over the batch of BCE-with-logits; g = dloss/dp + weight_decay p (torch Adam's coupled L2);
 * p <- adam_apply_one(p, g, ...) of csrc/adam_math.h with coef = 1 and, for the member's own step counter t,
 * step_size = lr / (float)(1 - beta1^t), bc2_sqrt = (float)sqrt(1 - beta2^t): the same expressions as adam.hip's host
 * side, in double, but evaluated by the device's pow and sqrt (not guaranteed bit-equal to the host's libm).
 * Every sum over rows has an order fixed by the member's own data: results do not depend on M, the grid or the slot.
 *
 * After each epoch: history[m][e][0] = sum_b loss_b n_b / n_train, history[m][e][1] = valid = mean BCE over the
 * validation rows.  Early stopping restates skorch's EarlyStopping as the reference configures it (monitor valid_loss,
 * patience, threshold 1e-4 with threshold_mode "rel", lower_is_better, load_best=True).  skorch is not installable where
 * this was written, so these rules are RECALLED from skorch's documentation, not pinned against its code:
 *   improved iff valid < best * (1 - threshold)  (fp32);  improved: best = valid, misses = 0, best_epoch = e,
 *   best_params = params;  otherwise misses += 1;  then epoch = e + 1 and the member stops when misses == patience or
 *   epoch == max_epochs.  The trained classifier is best_params.
 * Per-member state the caller initialises before the first launch: params (initial weights), exp_avg = exp_avg_sq = 0,
 * step = 0, best = +inf, misses = 0, epoch = 0, best_epoch = -1, stopped = 0, history = NaN.
 */
#ifndef SBI_AMD_LC2ST_H
#define SBI_AMD_LC2ST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sbi_amd_lc2st_config {
  int32_t D, Dx, H;    /* theta-dim, x-dim, hidden width (reference default 10 D) */
  int32_t B;           /* minibatch rows (reference: 200) */
  float lr;            /* skorch's default 0.01 */
  float weight_decay;  /* reference: 1e-4 */
  float beta1, beta2, eps; /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 */
  int32_t patience;    /* reference: 50 */
  float threshold;     /* skorch's default 1e-4 (relative) */
  int32_t max_epochs;  /* reference: 1000 */
} sbi_amd_lc2st_config;

/* P, or SBI_AMD_E_* for a shape outside the envelope (a host-side answer). */
int64_t sbi_amd_lc2st_param_count(const sbi_amd_lc2st_config* cfg);

/* Up to `epochs_this_launch` (>= 1) epochs of every member that has not stopped: grid = M workgroups, a stopped member's
 * workgroup returns at once.  A bounded piece of work: the host loops over launches and reads `stopped` once per launch.
 * params, best_params, exp_avg, exp_avg_sq: (M, P);  step, misses, epoch, best_epoch, stopped: int32 (M);  best: (M);
 * history: (M, max_epochs, 2). */
int sbi_amd_lc2st_train_epochs(const sbi_amd_lc2st_config* cfg, const float* data, int64_t R, const int32_t* rows,
                               const float* labels, int64_t row_stride, const int32_t* n_train, const int32_t* n_valid,
                               const int32_t* member_id, int64_t M, uint64_t seed, float* params, float* best_params,
                               float* exp_avg, float* exp_avg_sq, int32_t* step, float* best, int32_t* misses,
                               int32_t* epoch, int32_t* best_epoch, int32_t* stopped, float* history,
                               int32_t epochs_this_launch, void* stream);

/* loss_out[m] and grad_out[m][P] = g (weight-decay term included) of every member at `params`, through the trainer's
 * own device functions, without an update.  which == 0: batch `batch` of epoch `epoch`; which == 1: the validation rows
 * as one batch (epoch and batch are ignored).  A batch index past the member's last batch gives loss NaN and g = 0. */
int sbi_amd_lc2st_batch_grad(const sbi_amd_lc2st_config* cfg, const float* data, int64_t R, const int32_t* rows,
                             const float* labels, int64_t row_stride, const int32_t* n_train, const int32_t* n_valid,
                             const int32_t* member_id, int64_t M, uint64_t seed, const float* params, int32_t which,
                             int32_t epoch, int32_t batch, float* loss_out, float* grad_out, void* stream);

/* The test statistic at one observation x_o[Dx].  The M members form M / group_size groups of consecutive members (an
 * ensemble); proba_out[g][i] = mean over the group's members of 1 - sigmoid(logit([theta_i, x_o])) -- the probability
 * of class 0, averaged over the ensemble before the score -- and score_out[g] = mean_i (proba - 1/2)^2, summed in a
 * fixed order.  theta: (theta_groups, n, D) with theta_groups == 1 (shared) or M / group_size (one block per group).
 * The first layer's x_o term W_x x_o + b is folded once per workgroup and member. */
int sbi_amd_lc2st_eval(const sbi_amd_lc2st_config* cfg, const float* params, const float* theta, const float* x_o,
                       int64_t n, int64_t M, int32_t group_size, int32_t theta_groups, float* proba_out,
                       float* score_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
