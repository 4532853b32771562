"""L-C2ST, the local classifier two-sample test (Linhart et al. 2023), behind the interface of
``sbi/diagnostics/lc2st.py`` (``LC2ST``, ``LC2ST_NF``) with every classifier trained and evaluated on the device.

The reference trains ``(1 + num_trials_null) x num_folds x num_ensemble`` small binary MLPs one after the other
(skorch, a dozen launches per minibatch).  Here they are the *members* of one trainer run: one persistent workgroup per
member runs whole epochs -- forward, backward, Adam, validation, early stopping -- on one shared data matrix
(csrc/lc2st_kernel.h, include/sbi_amd_lc2st.h).  The host builds the members (row lists, labels, validation split,
initial weights), loops over bounded launches until every member has stopped, and evaluates all classifiers of a call in
one launch.

What differs from the reference, on purpose:
  * only the MLP classifier exists (``classifier="mlp"`` or sklearn's ``MLPClassifier`` class, which means the same
    here); anything else raises ``NotImplementedError``.  There is no CPU path: without a ROCm device training and
    evaluation raise ``RuntimeError``.
  * the minibatch orders come from the device-side keyed permutation, the validation split (10 % of a member's rows,
    not stratified) and the ``nn.Linear``-default initial weights from host generators seeded per member: a run is a
    pure function of ``seed``, but not the reference's stream.
  * early stopping restates skorch's ``EarlyStopping`` from its documentation (see the header).
"""

from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from enum import Enum, auto
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from sbi_amd.utils.sbiutils import handle_invalid_x

HIDDEN_WIDTH_PER_THETA_DIM = 10      # the reference's default classifier: two hidden layers of 10 x theta-dim
MAX_EPOCHS, PATIENCE = 1000, 50      # its epoch limit and early-stopping patience
VALID_FRACTION = 0.1                 # share of a member's rows held out for validation
# Epochs per launch, from tools/bench_lc2st.py (profiles/lc2st_bench.json): at the reference's
# default sizes (D = Dx = 10, N = 10 000, 101 members) an epoch of all members is 10.3 ms on the device whether a launch
# holds 1 epoch (10.49 ms), 4 (10.34 ms) or 16 (10.33 ms), so the launch itself costs ~1 %; 4 keeps one launch a bounded ~40 ms piece
# of work, takes that 1 % back, and makes the host's one read of `stopped` per launch < 0.2 % of the run.
DEFAULT_EPOCHS_PER_LAUNCH = 4

_ACCEPTED_KWARGS = ("module__hidden_layer_sizes", "max_epochs", "batch_size", "lr", "optimizer__weight_decay", "patience")


class LC2STState(Enum):
    """INITIALIZED -> OBSERVED_TRAINED / NULL_TRAINED -> READY, as the training methods are called (either order)."""

    INITIALIZED = auto()
    OBSERVED_TRAINED = auto()
    NULL_TRAINED = auto()
    READY = auto()


@dataclass
class LC2STScores:
    """scores: (num_folds,) per call on observed data, (num_trials_null,) under the null; probabilities as the reference."""

    scores: np.ndarray
    probabilities: Optional[np.ndarray] = None


@dataclass(frozen=True)
class LC2STHyper:
    """Hyper-parameters of one trainer run (mirror of ``struct sbi_amd_lc2st_config``)."""

    D: int
    Dx: int
    H: int
    batch_size: int = 200
    lr: float = 0.01
    weight_decay: float = 1e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    patience: int = PATIENCE
    threshold: float = 1e-4
    max_epochs: int = MAX_EPOCHS

    @property
    def F(self) -> int:
        return self.D + self.Dx

    def param_count(self) -> int:
        return self.H * self.F + self.H * self.H + 3 * self.H + 1

    def param_shapes(self) -> List[Tuple[str, Tuple[int, ...]]]:
        H, F = self.H, self.F
        return [("sequential.0.weight", (H, F)), ("sequential.0.bias", (H,)), ("sequential.2.weight", (H, H)),
                ("sequential.2.bias", (H,)), ("sequential.4.weight", (1, H)), ("sequential.4.bias", (1,))]

    def c_config(self):
        from sbi_amd import _lib

        return _lib.LC2STConfigC(self.D, self.Dx, self.H, self.batch_size, self.lr, self.weight_decay, self.beta1,
                                 self.beta2, self.eps, self.patience, self.threshold, self.max_epochs)


@dataclass
class Members:
    """The members of one trainer run over a shared data matrix (host arrays; see include/sbi_amd_lc2st.h)."""

    rows: np.ndarray        # (M, stride) int32 indices into the data matrix: n_train training rows, then n_valid
    labels: np.ndarray      # (M, stride) float32, aligned with rows
    n_train: np.ndarray     # (M,) int32
    n_valid: np.ndarray     # (M,) int32
    member_id: np.ndarray   # (M,) int32
    init_seed: np.ndarray   # (M,) int64: seed of the member's initial weights


@dataclass
class TrainedClassifier:
    """One entry of ``trained_clfs``: the ensemble of one cross-validation fold (``best_params`` of its members)."""

    hyper: LC2STHyper
    params: Tensor                 # (num_ensemble, P), on the device
    history: np.ndarray            # (num_ensemble, max_epochs, 2): train / valid loss, NaN beyond the last epoch
    best_epoch: np.ndarray         # (num_ensemble,)
    epochs: np.ndarray             # (num_ensemble,)


def _null_permutation(n: int, seed: int) -> np.ndarray:
    """The order in which null trial `seed` re-deals the 2 n joint rows to the two classes: torch's `randperm` right after
    `manual_seed(seed)` on the global generator, which is what the reference's null trials use."""
    torch.manual_seed(seed)
    return torch.randperm(2 * n).numpy()


def permute_data(theta_p: Tensor, theta_q: Tensor, seed: int = 1) -> Tuple[Tensor, Tensor]:
    """Null samples from two equally sized sample sets: pool them, re-deal the pooled rows in the order
    `_null_permutation(n, seed)`, hand the first n back as P and the rest as Q (the same as permuting the labels)."""
    n = len(theta_p)
    if len(theta_q) != n:
        raise ValueError(f"permute_data needs two sample sets of one size, got {n} and {len(theta_q)}.")
    order = torch.from_numpy(_null_permutation(n, seed))
    pooled = torch.cat([theta_p, theta_q], dim=0)
    return pooled[order[:n]], pooled[order[n:]]


def kfold_train_indices(n: int, num_folds: int, seed: int) -> List[np.ndarray]:
    """Training indices of ``KFold(n_splits=num_folds, shuffle=True, random_state=seed).split(range(n))``: the shuffled
    indices are cut into folds of n // k (+ 1 for the first n % k) and a fold's training set is the sorted rest."""
    if num_folds <= 1:
        return [np.arange(n)]
    idx = np.arange(n)
    np.random.RandomState(seed).shuffle(idx)
    sizes = np.full(num_folds, n // num_folds, dtype=int)
    sizes[: n % num_folds] += 1
    out, start = [], 0
    for s in sizes:
        mask = np.ones(n, dtype=bool)
        mask[idx[start:start + s]] = False
        out.append(np.nonzero(mask)[0])
        start += s
    return out


def resolve_hyper(classifier: Any, classifier_kwargs: Optional[Dict[str, Any]], D: int, Dx: int) -> LC2STHyper:
    """The reference's ``_resolve_classifier`` + ``_get_classifier_kwargs`` for the one classifier that exists here."""
    if isinstance(classifier, str):
        name = classifier.lower()
        if name == "random_forest":
            raise NotImplementedError('classifier "random_forest" is not implemented on the device; use "mlp".')
        if name != "mlp":
            raise ValueError(f'Invalid classifier: "{classifier}". Expected "mlp", "random_forest", '
                             "or a valid scikit-learn classifier class.")
    elif isinstance(classifier, type) and any(
            b.__name__ == "BaseEstimator" and b.__module__.startswith("sklearn.") for b in classifier.__mro__):
        if classifier.__name__ != "MLPClassifier" or not classifier.__module__.startswith("sklearn.neural_network"):
            raise NotImplementedError(f"classifier class {classifier.__name__} is not implemented on the device; "
                                      'only the MLP classifier ("mlp" / sklearn\'s MLPClassifier) is.')
    else:
        raise TypeError(f"classifier must be a string or a subclass of BaseEstimator, got {type(classifier).__name__}.")
    kw = dict(classifier_kwargs or {})
    for k in kw:
        if k not in _ACCEPTED_KWARGS:
            raise NotImplementedError(f"classifier_kwargs[{k!r}] is not supported by the device classifier "
                                      f"(accepted: {', '.join(_ACCEPTED_KWARGS)}).")
    hidden = kw.get("module__hidden_layer_sizes", (HIDDEN_WIDTH_PER_THETA_DIM * D,) * 2)
    hidden = tuple(int(h) for h in hidden)
    if len(hidden) != 2 or hidden[0] != hidden[1]:
        raise NotImplementedError(f"module__hidden_layer_sizes={hidden}: the device classifier has two hidden layers of "
                                  "equal width.")
    H = hidden[0]
    if D < 1 or Dx < 1 or D + Dx > 64:
        raise NotImplementedError(f"theta-dim {D} + x-dim {Dx} = {D + Dx} inputs: the device classifier takes 2 ... 64.")
    if not 1 <= H <= 128:
        raise NotImplementedError(f"hidden width {H}: the device classifier takes 1 ... 128 "
                                  "(pass classifier_kwargs={'module__hidden_layer_sizes': (128, 128)} at most).")
    hyper = LC2STHyper(D=D, Dx=Dx, H=H, batch_size=int(kw.get("batch_size", 200)), lr=float(kw.get("lr", 0.01)),
                       weight_decay=float(kw.get("optimizer__weight_decay", 1e-4)),
                       patience=int(kw.get("patience", PATIENCE)),
                       max_epochs=int(kw.get("max_epochs", MAX_EPOCHS)))
    if hyper.batch_size < 1 or hyper.max_epochs < 1 or hyper.patience < 1:
        raise ValueError("batch_size, max_epochs and patience must be >= 1.")
    return hyper


def build_members(n: int, num_folds: int, num_ensemble: int, seed: int, trials: List[Tuple[int, Optional[np.ndarray], int]],
                  fold_seed: Optional[int] = None) -> Members:
    """Members of the trials ``(trial_index, perm, row_offset)`` over joint data laid out [P rows; Q rows] (n each) from
    ``row_offset``.  ``perm`` (2 n,) re-assigns the joint rows to the halves -- position j < n is a P row (label 0),
    position n + j a Q row (label 1) -- or is None for the identity.  Folds are cut on the halves after the permutation;
    each member holds out ceil(10 %) of its rows for validation, split drawn from (seed, member id).  The folds follow
    ``fold_seed`` (default: ``seed``)."""
    folds = kfold_train_indices(n, num_folds, seed if fold_seed is None else fold_seed)
    stride = 2 * max(len(f) for f in folds)
    M = len(trials) * num_folds * num_ensemble
    rows = np.zeros((M, stride), dtype=np.int32)
    labels = np.zeros((M, stride), dtype=np.float32)
    n_train = np.zeros(M, dtype=np.int32)
    n_valid = np.zeros(M, dtype=np.int32)
    member_id = np.zeros(M, dtype=np.int32)
    init_seed = np.zeros(M, dtype=np.int64)
    m = 0
    for trial, perm, offset in trials:
        for f, tr in enumerate(folds):
            pos = np.concatenate([tr, n + tr])
            src = (pos if perm is None else perm[pos]) + offset
            lab = np.concatenate([np.zeros(len(tr), np.float32), np.ones(len(tr), np.float32)])
            for e in range(num_ensemble):
                mid = (trial * num_folds + f) * num_ensemble + e
                order = np.random.RandomState([(seed + e) % (2**32), mid]).permutation(len(pos))
                nv = max(1, int(math.ceil(VALID_FRACTION * len(pos))))
                order = np.concatenate([order[nv:], order[:nv]])      # training rows first, then the validation rows
                rows[m, : len(pos)] = src[order]
                labels[m, : len(pos)] = lab[order]
                n_train[m], n_valid[m], member_id[m] = len(pos) - nv, nv, mid
                init_seed[m] = (seed + e) * 1_000_003 + mid
                m += 1
    return Members(rows, labels, n_train, n_valid, member_id, init_seed)


def init_params(hyper: LC2STHyper, init_seed: int) -> Tensor:
    """torch's ``nn.Linear`` default for the three layers (weight and bias U(+-1 / sqrt(fan_in))), flat, from a host
    generator: the oracle loads the same numbers."""
    g = torch.Generator().manual_seed(int(init_seed))
    out = []
    for name, shape in hyper.param_shapes():
        fan_in = {"0": hyper.F, "2": hyper.H, "4": hyper.H}[name.split(".")[1]]
        bound = 1.0 / math.sqrt(fan_in)
        out.append(((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound).float().reshape(-1))
    return torch.cat(out)


def early_stopping_replay(valid: np.ndarray, patience: int, max_epochs: int, threshold: float = 1e-4
                          ) -> Tuple[bool, int, int]:
    """The early-stopping rule of the trainer over a sequence of validation losses, in fp32 as the kernel:
    -> (stopped, epochs run, best epoch)."""
    best, misses, best_epoch = np.float32(np.inf), 0, -1
    scale = np.float32(1.0) - np.float32(threshold)
    e = 0
    for e0, v in enumerate(np.asarray(valid, dtype=np.float32)):
        if v < best * scale:
            best, misses, best_epoch = v, 0, e0
        else:
            misses += 1
        e = e0 + 1
        if misses >= patience or e >= max_epochs:
            return True, e, best_epoch
    return False, e, best_epoch


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("sbi_amd: the L-C2ST classifiers train and evaluate only on a ROCm device (MI355X) and none "
                           "is visible. There is deliberately no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


class TrainerRun:
    """Device state of one trainer run (include/sbi_amd_lc2st.h); ``run()`` loops over bounded launches."""

    def __init__(self, hyper: LC2STHyper, data: Tensor, members: Members, seed: int, params0: Optional[Tensor] = None):
        from sbi_amd import _lib

        self._lib = _lib
        self.hyper, self.seed = hyper, int(seed) & (2**64 - 1)
        dev = self.dev = _device()
        self.data = data.to(dev, torch.float32).contiguous()
        if self.data.dim() != 2 or self.data.shape[1] != hyper.F:
            raise ValueError(f"data must be (rows, {hyper.F}), got {tuple(self.data.shape)}")
        M = self.M = len(members.n_train)
        P = hyper.param_count()
        tot = members.n_train.astype(np.int64) + members.n_valid
        if (members.n_train < 1).any() or (members.n_valid < 1).any() or (tot > members.rows.shape[1]).any():
            raise ValueError("every member needs >= 1 training and >= 1 validation row within its row list")
        if members.rows.min() < 0 or members.rows.max() >= self.data.shape[0]:
            raise ValueError("row index outside the data matrix")
        self.rows = torch.from_numpy(np.ascontiguousarray(members.rows, dtype=np.int32)).to(dev)
        self.labels = torch.from_numpy(np.ascontiguousarray(members.labels, dtype=np.float32)).to(dev)
        self.n_train = torch.from_numpy(members.n_train.astype(np.int32)).to(dev)
        self.n_valid = torch.from_numpy(members.n_valid.astype(np.int32)).to(dev)
        self.member_id = torch.from_numpy(members.member_id.astype(np.int32)).to(dev)
        if params0 is None:
            params0 = torch.stack([init_params(hyper, s) for s in members.init_seed])
        self.params = params0.to(dev, torch.float32).contiguous().clone()
        assert self.params.shape == (M, P)
        self.best_params = self.params.clone()
        self.exp_avg = torch.zeros(M, P, device=dev)
        self.exp_avg_sq = torch.zeros(M, P, device=dev)
        self.step = torch.zeros(M, dtype=torch.int32, device=dev)
        self.best = torch.full((M,), float("inf"), device=dev)
        self.misses = torch.zeros(M, dtype=torch.int32, device=dev)
        self.epoch = torch.zeros(M, dtype=torch.int32, device=dev)
        self.best_epoch = torch.full((M,), -1, dtype=torch.int32, device=dev)
        self.stopped = torch.zeros(M, dtype=torch.int32, device=dev)
        self.history = torch.full((M, hyper.max_epochs, 2), float("nan"), device=dev)
        self._cfg = hyper.c_config()

    def launch(self, epochs_this_launch: int) -> None:
        lib, p = self._lib, self._lib.ptr
        with torch.cuda.device(self.dev):
            rc = lib.load().sbi_amd_lc2st_train_epochs(
                self._cfg, p(self.data), self.data.shape[0], p(self.rows), p(self.labels), self.rows.shape[1],
                p(self.n_train), p(self.n_valid), p(self.member_id), self.M, self.seed, p(self.params),
                p(self.best_params), p(self.exp_avg), p(self.exp_avg_sq), p(self.step), p(self.best), p(self.misses),
                p(self.epoch), p(self.best_epoch), p(self.stopped), p(self.history), int(epochs_this_launch),
                lib.current_stream(self.dev))
        lib.check(rc, "lc2st_train_epochs")

    def run(self, epochs_per_launch: int = DEFAULT_EPOCHS_PER_LAUNCH) -> "TrainerRun":
        for _ in range(-(-self.hyper.max_epochs // epochs_per_launch) + 1):
            self.launch(epochs_per_launch)
            if bool(self.stopped.all()):      # the one host read per launch
                return self
        raise RuntimeError("sbi_amd: L-C2ST trainer did not stop within max_epochs (internal error)")

    def batch_grad(self, params: Tensor, which: int = 0, epoch: int = 0, batch: int = 0) -> Tuple[Tensor, Tensor]:
        lib, p = self._lib, self._lib.ptr
        params = params.to(self.dev, torch.float32).contiguous()
        loss = torch.empty(self.M, device=self.dev)
        grad = torch.empty(self.M, self.hyper.param_count(), device=self.dev)
        with torch.cuda.device(self.dev):
            rc = lib.load().sbi_amd_lc2st_batch_grad(
                self._cfg, p(self.data), self.data.shape[0], p(self.rows), p(self.labels), self.rows.shape[1],
                p(self.n_train), p(self.n_valid), p(self.member_id), self.M, self.seed, p(params), int(which),
                int(epoch), int(batch), p(loss), p(grad), lib.current_stream(self.dev))
        lib.check(rc, "lc2st_batch_grad")
        return loss, grad


def lc2st_eval(hyper: LC2STHyper, params: Tensor, theta: Tensor, x_o: Tensor, group_size: int = 1
               ) -> Tuple[Tensor, Tensor]:
    """-> proba (groups, n), score (groups,) on the device.  params (M, P); theta (n, D) shared or (groups, n, D)."""
    from sbi_amd import _lib

    dev = _device()
    params = params.to(dev, torch.float32).contiguous()
    theta = theta.to(dev, torch.float32).contiguous()
    x_o = x_o.to(dev, torch.float32).reshape(-1).contiguous()
    M = params.shape[0]
    if M % group_size:
        raise ValueError("the number of members must be a multiple of group_size")
    groups = M // group_size
    theta_groups = 1 if theta.dim() == 2 else theta.shape[0]
    n = theta.shape[-2]
    if theta.shape[-1] != hyper.D or x_o.numel() != hyper.Dx or theta_groups not in (1, groups):
        raise ValueError(f"theta {tuple(theta.shape)} / x_o {tuple(x_o.shape)} do not fit D={hyper.D}, Dx={hyper.Dx}, "
                         f"{groups} groups")
    proba = torch.empty(groups, n, device=dev)
    score = torch.empty(groups, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().sbi_amd_lc2st_eval(hyper.c_config(), _lib.ptr(params), _lib.ptr(theta), _lib.ptr(x_o), n, M,
                                            group_size, theta_groups, _lib.ptr(proba), _lib.ptr(score),
                                            _lib.current_stream(dev))
    _lib.check(rc, "lc2st_eval")
    return proba, score


# ---- front end ----------------------------------------------------------------------------------------------------
_SAMPLE_ARGS = ("prior_samples", "xs", "posterior_samples")
_DEPRECATED_THETAS = ("Parameter 'thetas' is deprecated and will be removed in a future version. "
                      "Use 'prior_samples' instead.")
_DEPRECATED_RETURN_PROBS = ("The 'return_probs' parameter is deprecated and will be removed in a future release. It "
                            "returns a (probs, scores) tuple; use LC2STScores.probabilities and LC2STScores.scores from "
                            "the default return value instead.")
_NULL_ALREADY_TRAINED = ("Classifiers under the null hypothesis are already trained. To retrain, create a new instance "
                         "or reset `trained_clfs_null` explicitly. Note that for LC2ST_NF the null classifiers are "
                         "data-independent and can be reused with new estimators.")
# what each training event makes of each state, and what a p-value still lacks in each state
_NEXT_STATE = {
    "observed": {LC2STState.INITIALIZED: LC2STState.OBSERVED_TRAINED, LC2STState.OBSERVED_TRAINED: LC2STState.OBSERVED_TRAINED,
                 LC2STState.NULL_TRAINED: LC2STState.READY, LC2STState.READY: LC2STState.READY},
    "null": {LC2STState.INITIALIZED: LC2STState.NULL_TRAINED, LC2STState.NULL_TRAINED: LC2STState.NULL_TRAINED,
             LC2STState.OBSERVED_TRAINED: LC2STState.READY, LC2STState.READY: LC2STState.READY},
}
_STILL_TO_CALL = {
    LC2STState.INITIALIZED: "train_on_observed_data() and train_under_null_hypothesis()",
    LC2STState.NULL_TRAINED: "train_on_observed_data()",
    LC2STState.OBSERVED_TRAINED: "train_under_null_hypothesis()",
}


def _take_samples(prior_samples, xs, posterior_samples, thetas) -> Dict[str, Any]:
    """The three sample arguments by name, with the deprecated alias `thetas` folded into `prior_samples`."""
    if thetas is not None:
        warnings.warn(_DEPRECATED_THETAS, FutureWarning, stacklevel=3)
        if prior_samples is not None:
            raise ValueError("Cannot specify both 'thetas' and 'prior_samples'. Use 'prior_samples' only.")
    given = dict(zip(_SAMPLE_ARGS, (thetas if prior_samples is None else prior_samples, xs, posterior_samples)))
    for name, value in given.items():
        if value is None:
            raise ValueError(f"{name} is required.")
    return given


def _check_samples(given: Dict[str, Any], num_folds: int, seed: Any) -> None:
    """Types, emptiness, matching sizes and dimensions of the sample tensors; the fold count; the seed's type."""
    for name, value in given.items():
        if not isinstance(value, Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(value)}.")
    for name, value in given.items():
        if len(value) == 0:
            raise ValueError(f"{name} cannot be empty.")
    n_prior, n_x, n_post = (len(given[name]) for name in _SAMPLE_ARGS)
    if len({n_prior, n_x, n_post}) != 1:
        raise ValueError(f"Sample size mismatch: prior_samples has {n_prior}, xs has {n_x}, posterior_samples has "
                         f"{n_post}. All must have the same number of samples.")
    d_prior, d_post = given["prior_samples"].shape[-1], given["posterior_samples"].shape[-1]
    if d_prior != d_post:
        raise ValueError(f"Dimension mismatch: prior_samples has dimension {d_prior}, but posterior_samples has "
                         f"dimension {d_post}.")
    if num_folds < 1:
        raise ValueError(f"num_folds must be >= 1, got {num_folds}.")
    if num_folds > n_prior:
        raise ValueError(f"num_folds ({num_folds}) cannot exceed sample size ({n_prior}).")
    if not isinstance(seed, int):
        raise TypeError(f"seed must be an integer, got {type(seed)}.")


def _drop_invalid_rows(given: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """Rows whose x holds a NaN or an Inf leave all three tensors (with a warning that counts them)."""
    keep, n_nan, n_inf = handle_invalid_x(given["xs"], exclude_invalid_x=True)
    if n_nan + n_inf > 0:
        warnings.warn(f"Found {n_nan} NaNs and {n_inf} Infs in xs. These rows will be removed from all input tensors. "
                      f"Only {keep.sum()} / {len(given['xs'])} samples remain.", stacklevel=3)
    return {name: value[keep] for name, value in given.items()}


def _column_stats(samples: Tensor) -> Tuple[Tensor, Tensor]:
    """(mean, std) per column; a constant column gets std 1, so that z-scoring only centres it."""
    std = samples.std(dim=0)
    return samples.mean(dim=0), torch.where(std == 0, torch.ones_like(std), std)


class LC2ST:
    r"""L-C2ST: tests :math:`H_0(x_o): q(\theta \mid x_o) = p(\theta \mid x_o)` at one observation.

    A classifier is trained to tell the joint samples :math:`[\theta_p, x]` (posterior, class 0) from
    :math:`[\theta_q, x]` (prior, class 1); the statistic at :math:`x_o` is the mean squared distance of its class-0
    probability from 1/2 over posterior samples at :math:`x_o`.  The same is done ``num_trials_null`` times under the
    null (permuted labels, or samples of a known null distribution), and the p-value is the share of null statistics
    above the observed one.  Arguments, states and messages are those of ``sbi.diagnostics.lc2st.LC2ST``.

    Example:
        >>> lc2st = LC2ST(prior_samples, xs, posterior_samples, num_folds=5)
        >>> lc2st.train_on_observed_data().train_under_null_hypothesis()
        >>> p_value = lc2st.p_value(theta_o=theta_obs, x_o=x_obs)
    """

    def __init__(self, prior_samples: Optional[Tensor] = None, xs: Optional[Tensor] = None,
                 posterior_samples: Optional[Tensor] = None, seed: int = 1, num_folds: int = 1, num_ensemble: int = 1,
                 classifier: Any = "mlp", z_score: bool = False, classifier_kwargs: Optional[Dict[str, Any]] = None,
                 num_trials_null: int = 100, permutation: bool = True, device: str = "cpu", *,
                 thetas: Optional[Tensor] = None) -> None:
        given = _take_samples(prior_samples, xs, posterior_samples, thetas)
        _check_samples(given, num_folds, seed)          # before indexing with the mask of valid rows ...
        given = _drop_invalid_rows({name: value.detach().cpu() for name, value in given.items()})
        _check_samples(given, num_folds, seed)          # ... and again on what is left
        # class 0 (P) = posterior samples, class 1 (Q) = prior samples, paired with the same x
        self.theta_p, self.theta_q = given["posterior_samples"].float(), given["prior_samples"].float()
        self.x_p = self.x_q = given["xs"].float()
        self.z_score = z_score
        self.theta_p_mean, self.theta_p_std = _column_stats(self.theta_p)
        self.x_p_mean, self.x_p_std = _column_stats(self.x_p)
        self.seed, self.num_folds, self.num_ensemble, self.device = seed, num_folds, num_ensemble, device
        self.num_trials_null, self.permutation = num_trials_null, permutation
        self.null_distribution: Optional[torch.distributions.Distribution] = None
        self.hyper = resolve_hyper(classifier, classifier_kwargs, self.theta_p.shape[-1], self.x_p.shape[-1])
        self.clf_kwargs = dict(classifier_kwargs or {})
        self.epochs_per_launch = DEFAULT_EPOCHS_PER_LAUNCH
        self.trained_clfs: Optional[List[TrainedClassifier]] = None
        self.trained_clfs_null: Optional[Dict[int, List[TrainedClassifier]]] = None
        self._state = LC2STState.INITIALIZED

    @property
    def state(self) -> LC2STState:
        return self._state

    # -- normalisation ------------------------------------------------------------------------------------------------
    def _normalize_theta(self, theta: Tensor) -> Tensor:
        return theta.sub(self.theta_p_mean).div(self.theta_p_std) if self.z_score else theta

    def _normalize_x(self, x: Tensor) -> Tensor:
        return x.sub(self.x_p_mean).div(self.x_p_std) if self.z_score else x

    def _joint(self, theta_p: Tensor, theta_q: Tensor, x_p: Tensor, x_q: Tensor) -> Tensor:
        """[P rows; Q rows] of normalised [theta, x]: the layout `build_members` indexes."""
        halves = [torch.cat([self._normalize_theta(t), self._normalize_x(x)], dim=1) for t, x in ((theta_p, x_p),
                                                                                                   (theta_q, x_q))]
        return torch.cat(halves, dim=0).float()

    # -- training -----------------------------------------------------------------------------------------------------
    def _train_trials(self, data: Tensor, trials, seed: int) -> Dict[int, List[TrainedClassifier]]:
        """One trainer run over all members of `trials`; -> {trial: [one TrainedClassifier per fold]}.  `seed` reseeds
        the classifiers (epoch orders, validation split, initial weights); the folds always follow `self.seed`."""
        members = build_members(self.theta_p.shape[0], self.num_folds, self.num_ensemble, seed, trials,
                                fold_seed=self.seed)
        run = TrainerRun(self.hyper, data, members, seed).run(self.epochs_per_launch)
        history, best_epoch, epochs = (t.cpu().numpy() for t in (run.history, run.best_epoch, run.epoch))
        per_fold = [TrainedClassifier(self.hyper, run.best_params[s].clone(), history[s], best_epoch[s], epochs[s])
                    for s in (slice(i, i + self.num_ensemble) for i in range(0, run.M, self.num_ensemble))]
        return {trial: per_fold[i * self.num_folds:(i + 1) * self.num_folds] for i, (trial, _, _) in enumerate(trials)}

    def _null_trials(self) -> Tuple[Tensor, list]:
        """The shared data matrix and the (trial, permutation, row offset) list of the null trials: with
        `permutation` the observed rows under the labels of `permute_data(seed=t)`, otherwise one block of rows per
        trial with theta drawn from `null_distribution`."""
        n = self.theta_p.shape[0]
        if self.permutation:
            data = self._joint(self.theta_p, self.theta_q, self.x_p, self.x_q)
            return data, [(t + 1, _null_permutation(n, t), 0) for t in range(self.num_trials_null)]
        if self.null_distribution is None:
            raise ValueError("A null distribution must be provided when permutation=False. "
                             "Set null_distribution or use permutation=True.")
        blocks = []
        for _ in range(self.num_trials_null):
            draws = [self.null_distribution.sample((n,)).cpu() for _ in "pq"]
            blocks.append(self._joint(draws[0], draws[1], self.x_p, self.x_q))
        return torch.cat(blocks, dim=0), [(t + 1, None, 2 * n * t) for t in range(self.num_trials_null)]

    def train_on_observed_data(self, seed: Optional[int] = None, verbosity: int = 1) -> "LC2ST":
        """Trains the ``num_folds x num_ensemble`` classifiers on the observed data, in one trainer run.  ``seed``
        reseeds the classifiers only; the cross-validation folds stay those of the constructor's seed."""
        data = self._joint(self.theta_p, self.theta_q, self.x_p, self.x_q)
        self.trained_clfs = self._train_trials(data, [(0, None, 0)], self.seed if seed is None else seed)[0]
        self._state = _NEXT_STATE["observed"][self._state]
        return self

    def train_under_null_hypothesis(self, verbosity: int = 1) -> "LC2ST":
        """Trains the ``num_trials_null x num_folds x num_ensemble`` classifiers under (H0), in one trainer run."""
        if self.trained_clfs_null is not None:
            raise ValueError(_NULL_ALREADY_TRAINED)
        data, trials = self._null_trials()
        trained = self._train_trials(data, trials, self.seed) if trials else {}
        self.trained_clfs_null = {trial - 1: clfs for trial, clfs in trained.items()}
        self._state = _NEXT_STATE["null"][self._state]
        return self

    # -- evaluation: cores take theta explicitly, the public methods (and LC2ST_NF's) supply it -------------------------
    def _eval(self, theta_o: Tensor, x_o: Tensor, clfs: List[TrainedClassifier]) -> Tuple[np.ndarray, np.ndarray]:
        """-> probabilities (len(clfs), n), scores (len(clfs),); theta_o (n, D) shared or (len(clfs), n, D)."""
        x_o = self._normalize_x(x_o.detach().cpu().float().reshape(1, -1))
        theta_o = self._normalize_theta(theta_o.detach().cpu().float())
        proba, score = lc2st_eval(self.hyper, torch.cat([c.params for c in clfs], dim=0), theta_o, x_o,
                                  group_size=self.num_ensemble)
        return proba.cpu().numpy(), score.cpu().numpy()

    @staticmethod
    def _packed(probs: np.ndarray, scores: np.ndarray, return_probs: bool):
        if not return_probs:
            return LC2STScores(scores=scores, probabilities=probs)
        warnings.warn(_DEPRECATED_RETURN_PROBS, FutureWarning, stacklevel=3)
        return probs, scores

    def _observed_statistic(self, theta_o: Tensor, x_o: Tensor) -> float:
        if self._state not in (LC2STState.OBSERVED_TRAINED, LC2STState.READY):
            raise RuntimeError("Classifiers have not been trained on observed data. "
                               "Call train_on_observed_data() before computing statistics.")
        return float(self._eval(theta_o, x_o, self.trained_clfs)[1].mean())

    def _null_statistics(self, theta_o: Tensor, x_o: Tensor) -> Tuple[np.ndarray, np.ndarray]:
        """-> probabilities (trials, folds, n), statistics (trials,): every trial and fold in one launch."""
        if self._state not in (LC2STState.NULL_TRAINED, LC2STState.READY):
            raise RuntimeError("Classifiers have not been trained under the null hypothesis. "
                               "Call train_under_null_hypothesis() first.")
        have = len(self.trained_clfs_null or {})
        if have != self.num_trials_null:
            raise RuntimeError(f"Expected {self.num_trials_null} null classifiers, got {have}.")
        T, K = self.num_trials_null, self.num_folds
        if T == 0:
            return np.zeros((0, K, len(theta_o))), np.zeros(0)
        if not self.permutation:
            if self.null_distribution is None:
                raise ValueError("A null distribution must be provided when permutation=False.")
            draws = torch.stack([self.null_distribution.sample((len(theta_o),)).cpu() for _ in range(T)])
            theta_o = draws.repeat_interleave(K, dim=0)      # one block per (trial, fold)
        probs, scores = self._eval(theta_o, x_o, [c for t in range(T) for c in self.trained_clfs_null[t]])
        return probs.reshape(T, K, -1), scores.reshape(T, K).mean(axis=1)

    def _p_value(self, *where) -> float:
        """Share of null statistics above the observed one, through the public statistic methods at `where`
        (theta_o, x_o here; x_o alone for LC2ST_NF)."""
        if self._state is not LC2STState.READY:
            raise RuntimeError(f"LC2ST is not ready to compute p-values. Call {_STILL_TO_CALL[self._state]} first.")
        observed = self.get_statistic_on_observed_data(*where)
        return float(np.mean(observed < self.get_statistics_under_null_hypothesis(*where).scores))

    def get_scores(self, theta_o: Tensor, x_o: Tensor, trained_clfs: List[TrainedClassifier],
                   return_probs: bool = False) -> Union[LC2STScores, Tuple[np.ndarray, np.ndarray]]:
        """Scores (one per cross-validation fold) of ``trained_clfs`` at ``x_o`` over the samples ``theta_o``."""
        return self._packed(*self._eval(theta_o, x_o, trained_clfs), return_probs)

    def get_statistic_on_observed_data(self, theta_o: Tensor, x_o: Tensor) -> float:
        """The statistic at ``x_o``: the mean of the folds' scores."""
        return self._observed_statistic(theta_o, x_o)

    def get_statistics_under_null_hypothesis(self, theta_o: Tensor, x_o: Tensor, return_probs: bool = False,
                                             verbosity: int = 0
                                             ) -> Union[LC2STScores, Tuple[np.ndarray, np.ndarray]]:
        """The null statistics at ``x_o``, one per trial (mean over the folds)."""
        return self._packed(*self._null_statistics(theta_o, x_o), return_probs)

    def p_value(self, theta_o: Tensor, x_o: Tensor) -> float:
        r"""The share of null statistics above the observed one: :math:`1/H \sum_h I(T_o < T_h)`."""
        return self._p_value(theta_o, x_o)

    def reject_test(self, theta_o: Tensor, x_o: Tensor, alpha: float = 0.05) -> bool:
        return bool(self.p_value(theta_o, x_o) < alpha)


class LC2ST_NF(LC2ST):
    r"""L-C2ST in the base space of a normalizing flow: with :math:`z = T_\phi^{-1}(\theta; x)` the null hypothesis is
    :math:`p(T_\phi^{-1}(\theta; x_o) \mid x_o) = \mathcal{N}(0, I)`.  No ``theta_o`` is passed to the evaluation
    methods (``num_eval`` base samples are drawn at initialisation), no permutation is used (the null distribution is
    known), and the null classifiers do not depend on the estimator: ``trained_clfs_null`` of one instance can be given
    to the next.  ``flow_inverse_transform(theta, x) -> noise`` is e.g. the ``inverse_transform`` of this package's
    flow estimators."""

    def __init__(self, prior_samples: Optional[Tensor] = None, xs: Optional[Tensor] = None,
                 posterior_samples: Optional[Tensor] = None,
                 flow_inverse_transform: Optional[Callable[[Tensor, Tensor], Tensor]] = None,
                 flow_base_dist: Optional[torch.distributions.Distribution] = None, num_eval: int = 10_000,
                 trained_clfs_null: Optional[Dict[int, List[TrainedClassifier]]] = None, *,
                 thetas: Optional[Tensor] = None, **kwargs: Any) -> None:
        given = _take_samples(prior_samples, xs, posterior_samples, thetas)
        for name, value in (("flow_inverse_transform", flow_inverse_transform), ("flow_base_dist", flow_base_dist)):
            if value is None:
                raise ValueError(f"{name} is required.")
        self.flow_inverse_transform = flow_inverse_transform
        to_base = {name: flow_inverse_transform(given[name], given["xs"]).detach()
                   for name in ("prior_samples", "posterior_samples")}
        super().__init__(xs=given["xs"], **to_base, **kwargs)
        self.permutation, self.null_distribution = False, flow_base_dist
        if trained_clfs_null is not None:         # trained elsewhere: they depend on neither the data nor the estimator
            self.trained_clfs_null = trained_clfs_null
            self._state = LC2STState.NULL_TRAINED
        self.theta_o = flow_base_dist.sample(torch.Size([num_eval])).cpu()

    def train_under_null_hypothesis(self, verbosity: int = 1) -> "LC2ST_NF":
        super().train_under_null_hypothesis(verbosity=verbosity)
        return self

    # the evaluation methods of the parent, at the base samples drawn in the constructor
    def get_scores(self, x_o: Tensor, trained_clfs: List[TrainedClassifier], return_probs: bool = False, **kwargs: Any):
        return self._packed(*self._eval(self.theta_o, x_o, trained_clfs), return_probs)

    def get_statistic_on_observed_data(self, x_o: Tensor, **kwargs: Any) -> float:
        return self._observed_statistic(self.theta_o, x_o)

    def get_statistics_under_null_hypothesis(self, x_o: Tensor, return_probs: bool = False, verbosity: int = 0,
                                             **kwargs: Any):
        return self._packed(*self._null_statistics(self.theta_o, x_o), return_probs)

    def p_value(self, x_o: Tensor, **kwargs: Any) -> float:
        return self._p_value(x_o)

    def reject_test(self, x_o: Tensor, alpha: float = 0.05, **kwargs: Any) -> bool:
        return bool(self._p_value(x_o) < alpha)
