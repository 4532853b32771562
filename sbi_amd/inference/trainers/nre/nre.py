"""Neural Ratio Estimation on the NRE kernels: NRE_A (AALR), NRE_B (SRE), NRE_C (CNRE) and BNRE.

API mirror of sbi's trainers in sbi/inference/trainers/nre/.  The classifier is the ResNet ratio estimator
(``classifier_nn("resnet")``); training is NPE's device-resident epoch loop (minibatch gather, validation, early
stopping, best-weights bookkeeping) driven through its hooks, with one fused step per minibatch (``FusedNREStep``):

    contrasting atoms (sbi_amd_atomic_atoms) -> logits of all pairs + activation stash (sbi_amd_nre_train_forward)
    -> per-row losses and d loss / d logit (sbi_amd_nre_loss_weights) -> gradients (sbi_amd_nre_train_backward)
    -> clip + Adam (sbi_amd_adam_clip_step) -> re-pack (sbi_amd_nre_pack).

The pairs are laid out atoms-major (pair a * B + b is atom a of row b with x[b]); the reference's _classifier_logits
(nre_base.py:396-415) lays out the same pairs row-major.  Validation draws fresh contrasting atoms from a keyed seed.
The posterior is sampled by MCMC (default) or rejection on the ratio-based potential sum_i log r(theta, x_i) + log
p(theta).
"""

from __future__ import annotations

from copy import deepcopy
from typing import Any, Callable, Dict, Optional, Union

import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd import _lib
from sbi_amd.inference.trainers.npe.npe import ImproperEmpirical, PosteriorEstimatorTrainer, validate_theta_and_x
from sbi_amd.neural_nets.estimators.ratio_estimator import RatioEstimator
from sbi_amd.neural_nets.factory import classifier_nn
from sbi_amd.neural_nets.net_builders.estimator_configs import NSFConfig, ResNetClassifierConfig
from sbi_amd.utils.sbiutils import handle_invalid_x, mcmc_transform, warn_on_invalid_x
from sbi_amd.utils.torchutils import check_if_prior_on_device

MODE_A, MODE_B, MODE_C, MODE_BNRE = 0, 1, 2, 3


def draw_atoms(theta: Tensor, num_atoms: int, seed: int, choices: Optional[Tensor] = None) -> Tensor:
    """(num_atoms, B, D): atom 0 = theta itself, atoms 1 .. num_atoms - 1 = other rows of the batch drawn uniformly
    without replacement (keyed by `seed`, or the given `choices` (B, num_atoms - 1))."""
    B, D = theta.shape
    if num_atoms == 1:      # (NRE_C's joint set with one class: the row itself)
        return theta.reshape(1, B, D).clone()
    lib = _lib.load()
    out = torch.empty(num_atoms, B, D, dtype=torch.float32, device=theta.device)
    ch = None if choices is None else choices.to(theta.device, torch.int64).contiguous()
    with torch.cuda.device(theta.device):
        rc = lib.sbi_amd_atomic_atoms(_lib.ptr(theta), B, num_atoms, D, int(seed) & (2**64 - 1), _lib.ptr(ch), None,
                                      _lib.ptr(out), _lib.current_stream(theta.device))
    _lib.check(rc, "atomic_atoms")
    return out


def row_losses_torch(mode: int, logits: Tensor, B: int, num_atoms: int, gamma: float = 1.0,
                     regularization_strength: float = 100.0) -> Tensor:
    """The reference's losses as per-row values whose mean is the reference's scalar (atoms-major logits); used off
    the fused path (autograd) and by the tests."""
    if mode in (MODE_A, MODE_BNRE):
        lj, lm = logits[:B], logits[B : 2 * B]
        sj, sm = torch.sigmoid(lj), torch.sigmoid(lm)
        bce = 0.5 * (-torch.clamp(torch.log(sj), min=-100.0) - torch.clamp(torch.log(1 - sm), min=-100.0))
        if mode == MODE_A:
            return bce
        reg = (sj + sm - 1).mean().square()
        return bce + regularization_strength * reg
    if mode == MODE_B:
        lg = logits.reshape(num_atoms, B).t()
        return -(lg[:, 0] - torch.logsumexp(lg, dim=-1))
    K = num_atoms - 1
    lm = logits[: (K + 1) * B].reshape(K + 1, B).t()[:, 1:]
    lj = logits[(K + 1) * B :].reshape(K, B).t()
    loggamma = torch.tensor(gamma, dtype=logits.dtype, device=logits.device).log()
    logK = torch.tensor(K, dtype=logits.dtype, device=logits.device).log()
    den_m = torch.cat([loggamma + lm, logK.expand(B, 1)], dim=-1)
    den_j = torch.cat([loggamma + lj, logK.expand(B, 1)], dim=-1)
    lpm = logK - torch.logsumexp(den_m, dim=-1)
    lpj = loggamma + lj[:, 0] - torch.logsumexp(den_j, dim=-1)
    pj, pm = gamma / (1 + gamma), 1 / (1 + gamma)
    return -(pm * lpm + pj * lpj)


class FusedNREStep:
    """One NRE training step on the device (module docstring); the snapshot / restore surface of FusedTrainStep that
    NPE's pipelined epoch loop uses."""

    tail_extra_images = 0

    def __init__(self, estimator: RatioEstimator, mode: int, num_atoms: int, gamma: float = 1.0,
                 regularization_strength: float = 100.0, lr: float = 5e-4, clip_max_norm: Optional[float] = 5.0,
                 betas=(0.9, 0.999), eps: float = 1e-8):
        self.est, self.net = estimator, estimator.net
        p = self.net.flat_params
        _lib.require_device(p)
        self.mode, self.num_atoms = int(mode), int(num_atoms)
        self.gamma, self.lam = float(gamma), float(regularization_strength)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.clip = float(clip_max_norm) if clip_max_norm is not None else 0.0
        self.exp_avg = torch.zeros_like(p.data)
        self.exp_avg_sq = torch.zeros_like(p.data)
        self.grad = torch.zeros_like(p.data)
        self.scratch = torch.zeros(256, dtype=torch.float32, device=p.device)
        self.step_count = 0
        self.workspace: Optional[Tensor] = None
        self.seeds = torch.Generator()
        self.seeds.manual_seed(int(torch.randint(0, 2**62, (1,)).item()))

    # -- optimizer state ------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "step": self.step_count}

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])

    def snapshot(self) -> dict:
        return {"params": self.net.flat_params.data.clone(), "exp_avg": self.exp_avg.clone(),
                "exp_avg_sq": self.exp_avg_sq.clone(), "step": self.step_count}

    def snapshot_into(self, snap: Optional[dict]) -> dict:
        if snap is None:
            return self.snapshot()
        snap["params"].copy_(self.net.flat_params.data)
        snap["exp_avg"].copy_(self.exp_avg)
        snap["exp_avg_sq"].copy_(self.exp_avg_sq)
        snap["step"] = self.step_count
        return snap

    def restore_optimizer(self, snap: dict) -> None:
        self.exp_avg.copy_(snap["exp_avg"])
        self.exp_avg_sq.copy_(snap["exp_avg_sq"])
        self.step_count = int(snap["step"])

    def restore(self, snap: dict) -> None:
        self.net.flat_params.data.copy_(snap["params"])
        self.restore_optimizer(snap)
        self.net.__dict__.pop("_packed_cache", None)

    # -- the step -------------------------------------------------------------------------------------------------
    def _next_seed(self) -> int:
        return int(torch.randint(0, 2**62, (1,), generator=self.seeds).item())

    def pair_thetas(self, theta: Tensor, choices=None) -> Tensor:
        """(total atoms, B, D): NRE_C draws its marginal set (K + 1 atoms) and its joint set (K atoms) independently."""
        if self.mode == MODE_C:
            K = self.num_atoms - 1
            c0, c1 = (None, None) if choices is None else choices
            return torch.cat([draw_atoms(theta, K + 1, self._next_seed() if c0 is None else 0, c0),
                              draw_atoms(theta, K, self._next_seed() if c1 is None else 0, c1)])
        return draw_atoms(theta, self.num_atoms, self._next_seed() if choices is None else 0, choices)

    def loss_and_grad(self, theta: Tensor, x: Tensor, global_batch: Optional[int] = None, choices=None):
        """Per-row losses (B); the flat gradient of their mean (x B / global_batch) lands in self.grad."""
        lib = _lib.load()
        dev = self.net.flat_params.device
        cfg = self.net.hyper.c_config()
        theta = theta.to(torch.float32).contiguous()
        x = x.to(torch.float32).contiguous()
        B = theta.shape[0]
        atoms = self.pair_thetas(theta, choices)
        n = atoms.shape[0] * B
        need = int(lib.sbi_amd_nre_train_workspace_floats(cfg, n))
        if need < 0:
            _lib.check(need, "nre_train_workspace_floats")
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.float32, device=dev)
        pk, zs = self.net.packed(dev)
        logits = torch.empty(n, dtype=torch.float32, device=dev)
        w = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        parts = torch.empty((B + 255) // 256, dtype=torch.float32, device=dev)
        st = _lib.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sbi_amd_nre_train_forward(cfg, _lib.ptr(pk), _lib.ptr(zs), _lib.ptr(atoms), _lib.ptr(x), n, B,
                                                     _lib.ptr(logits), _lib.ptr(self.workspace), st), "nre_train_forward")
            _lib.check(lib.sbi_amd_nre_loss_weights(self.mode, _lib.ptr(logits), B, self.num_atoms, self.gamma, self.lam,
                                                    1.0 / float(global_batch or B), _lib.ptr(loss), _lib.ptr(w),
                                                    _lib.ptr(parts), st), "nre_loss_weights")
            _lib.check(lib.sbi_amd_nre_train_backward(cfg, _lib.ptr(pk), _lib.ptr(zs), n, _lib.ptr(w),
                                                      _lib.ptr(self.grad), None, _lib.ptr(self.workspace), st),
                       "nre_train_backward")
        return loss

    def apply(self) -> None:
        """clip + Adam on the flat buffer, then the new weight image."""
        lib = _lib.load()
        p = self.net.flat_params
        dev = p.device
        self.step_count += 1
        pk, _ = self.net.packed(dev)
        st = _lib.current_stream(dev)
        with torch.cuda.device(dev):
            _lib.check(lib.sbi_amd_adam_clip_step(_lib.ptr(p.data), _lib.ptr(self.grad), _lib.ptr(self.exp_avg),
                                                  _lib.ptr(self.exp_avg_sq), p.numel(), self.step_count, self.lr,
                                                  self.betas[0], self.betas[1], self.eps, self.clip,
                                                  _lib.ptr(self.scratch), st), "adam_clip_step")
            # the kernel wrote the weights behind autograd's back: refresh the cached image in place (same key)
            _lib.check(lib.sbi_amd_nre_pack(self.net.hyper.c_config(), _lib.ptr(p.data), _lib.ptr(pk), st), "nre_pack")

    def step(self, theta: Tensor, x: Tensor, global_batch: Optional[int] = None) -> Tensor:
        loss = self.loss_and_grad(theta, x, global_batch)
        self.apply()
        return loss


class NRE_B(PosteriorEstimatorTrainer):
    """sbi's NRE_B / SRE (nre_b.py): 1-out-of-num_atoms classification."""

    _MODE = MODE_B

    def __init__(self, prior: Optional[Distribution] = None,
                 classifier: Union[str, ResNetClassifierConfig, Callable, None] = "resnet", device: str = "cpu",
                 logging_level: Union[int, str] = "WARNING", summary_writer=None, tracker=None,
                 show_progress_bars: bool = True):
        super().__init__(prior=prior, density_estimator=NSFConfig(), device=device, logging_level=logging_level,
                         summary_writer=summary_writer, tracker=tracker, show_progress_bars=show_progress_bars)
        if classifier is None or isinstance(classifier, str):
            self._build_neural_net = classifier_nn(model=classifier or "resnet")
        elif isinstance(classifier, ResNetClassifierConfig):
            self._build_neural_net = classifier.build
        elif callable(classifier):
            self._build_neural_net = classifier
        else:
            raise TypeError(f"classifier must be a string, a ResNetClassifierConfig or a builder, got {classifier!r}")
        self._gamma, self._reg = 1.0, 100.0
        self._val_seed = None

    # -- data -------------------------------------------------------------------------------------------------------
    def append_simulations(self, theta: Tensor, x: Tensor, exclude_invalid_x: bool = False, from_round: int = 0,
                           algorithm: Optional[str] = None, data_device: Optional[str] = None) -> "NRE_B":
        """nre_base.py / base.py:343-404: invalid x kept unless `exclude_invalid_x`; `from_round` tags the data."""
        if data_device is None:
            data_device = self._device
        theta, x = validate_theta_and_x(theta, x, data_device=data_device, training_device=self._device)
        is_valid_x, num_nans, num_infs = handle_invalid_x(x, exclude_invalid_x=exclude_invalid_x)
        x, theta = x[is_valid_x], theta[is_valid_x]
        warn_on_invalid_x(num_nans, num_infs, exclude_invalid_x)
        self._data_round_index.append(int(from_round))
        self._theta_roundwise.append(theta)
        self._x_roundwise.append(x)
        self._prior_masks.append(torch.full((theta.shape[0], 1), int(from_round) == 0, dtype=torch.bool))
        self._proposal_roundwise.append(None)
        if self._prior is None or isinstance(self._prior, ImproperEmpirical):
            self._prior = ImproperEmpirical(self.get_simulations()[0].to(self._device))
        return self

    # -- hooks of the epoch loop ------------------------------------------------------------------------------------
    def _num_pair_atoms(self) -> int:
        return self._num_atoms

    def _fused_training(self, net, calibration_kernel, emb_trainable, atomic) -> bool:
        return isinstance(net, RatioEstimator) and torch.device(self._device).type == "cuda" and calibration_kernel is None

    def _make_stepper(self, net, cfg, dist_mod):
        return FusedNREStep(net, self._MODE, self._num_pair_atoms(), gamma=self._gamma,
                            regularization_strength=self._reg, lr=cfg.learning_rate, clip_max_norm=cfg.clip_max_norm)

    def _first_round_losses(self, net, theta: Tensor, x: Tensor) -> Tensor:
        """The loss of a batch with contrasting atoms drawn from the keyed validation seed (autograd-capable)."""
        B = theta.shape[0]
        A = self._num_pair_atoms()
        dev = net.net.flat_params.device if net.net.flat_params.is_cuda else torch.device("cuda")
        th = theta.to(dev, torch.float32).contiguous()
        self._val_seed = (self._val_seed or 0) + 1
        if self._MODE == MODE_C:
            atoms = torch.cat([draw_atoms(th, A, self._val_seed * 2), draw_atoms(th, A - 1, self._val_seed * 2 + 1)])
        else:
            atoms = draw_atoms(th, A, self._val_seed)
        logits = net._log_ratio_rows(atoms.reshape(-1, th.shape[1]), x.to(dev, torch.float32).contiguous(), B)
        return row_losses_torch(self._MODE, logits, B, A, self._gamma, self._reg).to(theta.device)

    # -- training -----------------------------------------------------------------------------------------------
    def _train(self, num_atoms: int, kw: Dict[str, Any]) -> RatioEstimator:
        d = self._dist()
        if d is not None and d.get_world_size() > 1:
            raise NotImplementedError("NRE trains on one device: data-parallel NRE (torch.distributed with world size "
                                      f"{d.get_world_size()}) is not implemented.")
        if kw.pop("dataloader_kwargs", None):
            raise NotImplementedError("The device-resident loop has no DataLoader; dataloader_kwargs is unsupported.")
        for k in ("self", "__class__", "num_atoms"):
            kw.pop(k, None)
        # the validation atoms: a keyed stream, seeded from torch's RNG once per train() call
        self._val_seed = int(torch.randint(0, 2**40, (1,)).item()) * 4096
        return super().train(num_atoms=num_atoms, force_first_round_loss=True, **kw)

    def train(self, num_atoms: int = 10, training_batch_size: int = 200, learning_rate: float = 5e-4,
              validation_fraction: float = 0.1, stop_after_epochs: int = 20, max_num_epochs: int = 2**31 - 1,
              clip_max_norm: Optional[float] = 5.0, resume_training: bool = False, discard_prior_samples: bool = False,
              retrain_from_scratch: bool = False, show_train_summary: bool = False,
              dataloader_kwargs: Optional[dict] = None) -> RatioEstimator:
        """nre_b.py:118-155."""
        return self._train(num_atoms, dict(locals()))

    # -- posterior ------------------------------------------------------------------------------------------------
    def build_posterior(self, density_estimator: Optional[RatioEstimator] = None, prior: Optional[Distribution] = None,
                        sample_with: str = "mcmc", mcmc_method: str = "slice_np_vectorized",
                        mcmc_parameters: Optional[Dict[str, Any]] = None,
                        rejection_sampling_parameters: Optional[Dict[str, Any]] = None, **kwargs):
        """nre_base.py:316-395: MCMC (default) or rejection sampling on the ratio-based potential."""
        if sample_with not in ("mcmc", "rejection"):
            raise NotImplementedError(
                f"sample_with={sample_with!r}: VI / importance posteriors are outside the accelerated path; NRE "
                "samples with 'mcmc' or 'rejection'."
            )
        from sbi_amd.inference.potentials.ratio_based_potential import ratio_estimator_based_potential

        if prior is None:
            if self._prior is None:
                raise ValueError("You did not pass a prior. You have to pass the prior either at initialization "
                                 "`inference = NRE(prior)` or to `.build_posterior(prior=prior)`.")
            prior = self._prior
        else:
            check_if_prior_on_device(self._device, prior)
        if density_estimator is None:
            if self._neural_net is None:
                raise ValueError("No trained estimator: call .train() first or pass density_estimator=...")
            estimator = deepcopy(self._neural_net)
            device = self._device
        else:
            estimator = density_estimator
            device = str(next(density_estimator.parameters()).device)
        if sample_with == "mcmc":
            from sbi_amd.inference.posteriors.mcmc_posterior import MCMCPosterior

            mcmc_parameters = dict(mcmc_parameters or {})
            enable_transform = mcmc_parameters.pop("enable_transform", True)
            potential_fn, theta_transform = ratio_estimator_based_potential(estimator, prior, x_o=None,
                                                                            enable_transform=enable_transform)
            self._posterior = MCMCPosterior(potential_fn=potential_fn, proposal=prior, theta_transform=theta_transform,
                                            method=mcmc_method, device=device, **mcmc_parameters)
            return deepcopy(self._posterior)
        from sbi_amd.inference.posteriors.rejection_posterior import RejectionPosterior

        params = dict(rejection_sampling_parameters or {})
        unknown = set(params) - {"max_sampling_batch_size", "num_samples_to_find_max", "num_iter_to_find_max", "m"}
        if unknown:
            raise TypeError(f"unexpected rejection_sampling_parameters: {sorted(unknown)}")
        potential_fn, _ = ratio_estimator_based_potential(estimator, prior, x_o=None)
        self._posterior = RejectionPosterior(potential_fn=potential_fn, proposal=prior,
                                             theta_transform=mcmc_transform(prior, device=device), device=device,
                                             **params)
        return deepcopy(self._posterior)


def _check_loss_kwargs(loss_kwargs, **expected) -> None:
    """Accept the reference's `loss_kwargs` (a LossArgs dataclass or a dict) when it restates what this trainer uses;
    refuse anything that cannot be honoured."""
    if loss_kwargs is None:
        return
    items = loss_kwargs if isinstance(loss_kwargs, dict) else dict(getattr(loss_kwargs, "__dict__", {}))
    for k, v in items.items():
        if k not in expected or v != expected[k]:
            raise NotImplementedError(f"loss_kwargs {k}={v!r}: this trainer uses {expected}; other loss arguments "
                                      "are not supported.")


class NRE_A(NRE_B):
    """sbi's NRE_A / AALR (nre_a.py): binary cross-entropy on two atoms (joint vs marginal)."""

    _MODE = MODE_A

    def train(self, training_batch_size: int = 200, learning_rate: float = 5e-4, validation_fraction: float = 0.1,
              stop_after_epochs: int = 20, max_num_epochs: int = 2**31 - 1, clip_max_norm: Optional[float] = 5.0,
              resume_training: bool = False, discard_prior_samples: bool = False, retrain_from_scratch: bool = False,
              show_train_summary: bool = False, dataloader_kwargs: Optional[dict] = None,
              loss_kwargs: Optional[Any] = None) -> RatioEstimator:
        """nre_a.py:105-163 (always two atoms).  `loss_kwargs` (sbi's LossArgsNRE_A) may only restate the two atoms."""
        kw = dict(locals())
        _check_loss_kwargs(kw.pop("loss_kwargs"), num_atoms=2)
        return self._train(2, kw)


class BNRE(NRE_A):
    """sbi's BNRE (bnre.py): NRE_A's loss plus the balancing regulariser."""

    _MODE = MODE_BNRE

    def train(self, regularization_strength: float = 100.0, training_batch_size: int = 200,
              learning_rate: float = 5e-4, validation_fraction: float = 0.1, stop_after_epochs: int = 20,
              max_num_epochs: int = 2**31 - 1, clip_max_norm: Optional[float] = 5.0, resume_training: bool = False,
              discard_prior_samples: bool = False, retrain_from_scratch: bool = False, show_train_summary: bool = False,
              dataloader_kwargs: Optional[dict] = None) -> RatioEstimator:
        """bnre.py:105-165."""
        self._reg = float(regularization_strength)
        kw = dict(locals())
        kw.pop("regularization_strength")
        return self._train(2, kw)


class NRE_C(NRE_B):
    """sbi's NRE_C / CNRE (nre_c.py): K + 1 classes with the gamma-weighted marginal class."""

    _MODE = MODE_C

    def train(self, num_classes: int = 5, gamma: float = 1.0, training_batch_size: int = 200,
              learning_rate: float = 5e-4, validation_fraction: float = 0.1, stop_after_epochs: int = 20,
              max_num_epochs: int = 2**31 - 1, clip_max_norm: Optional[float] = 5.0, resume_training: bool = False,
              discard_prior_samples: bool = False, retrain_from_scratch: bool = False, show_train_summary: bool = False,
              dataloader_kwargs: Optional[dict] = None) -> RatioEstimator:
        """nre_c.py:107-166: num_atoms = num_classes + 1."""
        if num_classes < 1:
            raise ValueError(f"num_classes = {num_classes} must be greater than 1.")
        self._gamma = float(gamma)
        kw = dict(locals())
        kw.pop("num_classes")
        kw.pop("gamma")
        return self._train(num_classes + 1, kw)


NRE = NRE_B      # sbi/inference/__init__.py
SNRE = NRE_B
SNRE_B = NRE_B
SRE = NRE_B
AALR = NRE_A
SNRE_A = NRE_A
CNRE = NRE_C
SNRE_C = NRE_C
