"""The divergence optimisers of ``VIPosterior`` (sbi/samplers/vi/vi_divergence_optimizers.py): rKL, IW, fKL, alpha.

Two routes with the same semantics.

* **Eager**: the surrogate losses as written in the reference, in torch with autograd, ``clip_grad_norm_``, the torch
  optimiser and scheduler.  It serves any q, any optimiser / scheduler, the host, and everything outside the envelope.
* **Kernel** (``kernel_route()``): q is a ``LearnableGaussian`` on a ROCm device with a per-dimension link, Adam +
  ExponentialLR with default options, identity ``weight_transform``, at most 65 536 rows per step.  An iteration is
  ``sbi_amd_vi_gauss_draw`` -> the potential and its gradient with respect to theta -> ``sbi_amd_vi_gauss_step``
  (include/sbi_amd_vi.h): the closed-form reverse mode of the surrogate loss, clip, Adam, the non-finite guard and the
  loss ring in one launch.  Nothing is read back inside ``kernel_steps``; the caller reads the ring and the status
  block every ``READBACK`` iterations.

Departures of the kernel route from the reference, all stated in DESIGN.md: the loss statistics advance at the
read-back cadence; a non-finite step is skipped on the device (phi restored, moments zeroed) and the warm-up of
``resolve_state`` follows at the next read-back; the fKL / IW weights are max-shifted.
"""

from __future__ import annotations

import math
from abc import ABC, abstractmethod
from contextlib import contextmanager
from typing import Callable, Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn
from torch.optim import Adam
from torch.optim.lr_scheduler import ExponentialLR

from sbi_amd.samplers.vi.vi_utils import (MAX_KERNEL_PARTICLES, LearnableGaussian, detach_and_deepcopy,
                                          filter_kwargs_for_func, move_distribution)

_VI_method: Dict[str, type] = {}
READBACK = 25                      # iterations between two reads of the loss ring / status block on the kernel route
RING = 64                          # slots of the loss ring (>= READBACK)
_METHOD_CODE = {"rKL": 0, "IW": 1, "alpha": 2, "fKL": 3}


def _identity_weight_transform(x):
    return x


class _KernelState:
    """Device buffers of the kernel route: phi, Adam's moments, the snapshot, the workspace, [status | ring]."""

    def __init__(self, q: LearnableGaussian, rows: int):
        from sbi_amd import _lib

        self.lib = _lib.load()
        phi = q.flat_parameters()
        dev = phi.device
        self.device = dev
        self.dim = q._dim
        self.phi = phi
        self.exp_avg = torch.zeros_like(phi)
        self.exp_avg_sq = torch.zeros_like(phi)
        self.snapshot = phi.clone()
        self.block = torch.zeros(4 + RING, dtype=torch.int32, device=dev)         # one copy brings both back
        self.status, self.ring = self.block[:4], self.block[4:].view(torch.float32)
        self.scratch_ring = torch.zeros(RING, dtype=torch.float32, device=dev)    # the warm-up's losses
        self.adam_t = 0
        self.step = 0
        self.seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
        self.nonfinite_seen = 0
        self.rows = 0
        self.workspace: Optional[Tensor] = None
        self.reserve(rows)

    def reserve(self, rows: int) -> None:
        from ctypes import byref, c_int64

        from sbi_amd import _lib

        if rows <= self.rows:
            return
        need = c_int64(0)
        _lib.check(self.lib.sbi_amd_vi_gauss_plan(self.dim, rows, byref(need)), "vi_gauss_plan")
        self.workspace = torch.empty((need.value + 3) // 4, dtype=torch.float32, device=self.device)
        self.rows = rows

    def forget_moments(self) -> None:
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.adam_t = 0


class DivergenceOptimizer(ABC):
    """A torch optimiser and scheduler around q, the loss statistics that decide convergence, and the way back to a
    valid state after non-finite values.  Subclasses define `_loss` (eager) and `_kernel_config` (kernel route)."""

    def __init__(self, potential_fn, q, prior=None, n_particles: int = 256, clip_value: float = 5.0,
                 optimizer=Adam, scheduler=ExponentialLR, eps: float = 1e-5, **kwargs):
        self.potential_fn = potential_fn
        self.q = q
        self.prior = prior
        self.device = potential_fn.device
        self.to(self.device)
        self.n_particles = n_particles
        self.clip_value = clip_value
        self.learning_rate = kwargs.get("lr", 1e-3)
        self.retain_graph = kwargs.get("retain_graph", False)
        self.force_eager = False
        self._kwargs = kwargs
        if isinstance(self.q, nn.Module):
            self.modules = nn.ModuleList([self.q])
            self.modules.train()
        else:
            self.modules = None
        if not hasattr(self.q, "parameters"):
            raise ValueError("The variational distribution has no parameters to optimize.")
        self.to(self.device)
        self.state_dict = [p.detach().clone() for p in self.q.parameters()]      # the last finite parameters
        self._build_torch_optimizer(optimizer, scheduler, dict(kwargs))
        self.eps = eps
        self.num_step = 0
        self.warm_up_was_done = False
        self.reset_loss_stats()
        self.HYPER_PARAMETERS = ["n_particles", "clip_value", "eps"]
        self._kstate: Optional[_KernelState] = None
        self._sched_steps = 0

    def _build_torch_optimizer(self, opt_type, sched_type, kwargs: Dict) -> None:
        kwargs["lr"] = kwargs.get("lr", self.learning_rate)
        opt_kwargs = filter_kwargs_for_func(opt_type.__init__, kwargs)
        kwargs.pop("lr")                                    # (CyclicLR names an `lr` of its own)
        sched_kwargs = filter_kwargs_for_func(sched_type.__init__, kwargs)
        self._opt_kwargs, self._sched_kwargs = opt_kwargs, sched_kwargs
        self._optimizer = opt_type(self.q.parameters(), **opt_kwargs)
        self._scheduler = sched_type(self._optimizer, **sched_kwargs)

    @abstractmethod
    def _loss(self, x_o: Tensor) -> Tuple[Tensor, Tensor]:
        """(surrogate loss to differentiate, loss to display)."""

    def _kernel_config(self) -> Optional[dict]:
        """Fields of `sbi_amd_vi_config` besides D / full_cov, or None when the method has no kernel."""
        return None

    def _rows_per_step(self) -> int:
        return self.n_particles

    # -- devices ----------------------------------------------------------------------------------------------
    def to(self, device) -> None:
        self.device = device
        self.potential_fn.to(self.device)
        if hasattr(self.q, "to"):
            self.q.to(self.device)
        self.prior = move_distribution(self.prior, self.device)
        if getattr(self, "_kstate", None) is not None and str(self._kstate.device) != str(self.q.loc.device):
            self._kstate = None

    # -- routing ----------------------------------------------------------------------------------------------
    def kernel_route(self) -> Tuple[bool, str]:
        if self.force_eager:
            return False, "force_eager is set"
        if not isinstance(self.q, LearnableGaussian):
            return False, f"q is a {type(self.q).__name__}: the kernels implement the Gaussian families only"
        ok, reason = self.q.kernel_route()
        if not ok:
            return False, reason
        if self._kernel_config() is None:
            return False, f"{type(self).__name__} has no kernel"
        if type(self._optimizer) is not Adam or set(self._opt_kwargs) - {"lr", "betas"}:
            return False, "the optimizer is not Adam with default options (lr and betas aside)"
        if type(self._scheduler) is not ExponentialLR or set(self._sched_kwargs) - {"gamma"}:
            return False, "the scheduler is not ExponentialLR"
        rows = self._rows_per_step()
        if rows > MAX_KERNEL_PARTICLES:
            return False, f"{rows} particles per step > {MAX_KERNEL_PARTICLES}"
        wt = getattr(self, "weight_transform", _identity_weight_transform)
        if wt is not _identity_weight_transform:
            return False, "a custom weight_transform"
        return True, ""

    # -- warm-up and recovery ---------------------------------------------------------------------------------
    WARM_UP_DRAWS = 32

    @contextmanager
    def _q_in_torch(self):
        """While an eager iteration runs, a `LearnableGaussian` draws and evaluates with torch only."""
        q = self.q
        pinned = isinstance(q, LearnableGaussian) and not q.force_eager
        if pinned:
            q.force_eager = True
        try:
            yield
        finally:
            if pinned:
                q.force_eager = False

    def _reparameterised_draws(self, n: int) -> Tuple[Tensor, Tensor]:
        """(theta, log q(theta)) with gradients to q's parameters through both: the family's own joint method where
        it has one, `rsample` then `log_prob` for a plain distribution."""
        joint = getattr(self.q, "sample_and_log_prob", None)
        if joint is not None:
            return joint(torch.Size((n,)))
        theta = self.q.rsample(torch.Size((n,)))
        return theta, self.q.log_prob(theta)

    def warm_up(self, num_steps: int, method: str = "prior") -> None:
        """Moves q onto the prior before the first real step: `num_steps` reverse-KL steps against the prior's density
        with 32 draws each, the optimiser applied without clipping and without a scheduler step."""
        if method != "prior":
            raise NotImplementedError(f"Only 'prior' warmup method is supported. Got: {method}")
        if self.prior is None:
            raise ValueError("Prior must be provided for warmup.")
        if self.kernel_route()[0]:
            self._kernel_warm_up(num_steps)
        else:
            with self._q_in_torch():
                for _ in range(num_steps):
                    theta, log_q = self._reparameterised_draws(self.WARM_UP_DRAWS)
                    kl = (log_q - self.prior.log_prob(theta)).mean()
                    self._optimizer.zero_grad()
                    kl.backward(retain_graph=self.retain_graph)
                    self._optimizer.step()
        self.warm_up_was_done = True

    def update_state(self) -> None:
        """Remembers every parameter tensor that is finite; one that is not is re-drawn uniformly in [-0.5, 0.5]."""
        with torch.no_grad():
            for slot, para in enumerate(self.q.parameters()):
                if bool(torch.isfinite(para).all()):
                    self.state_dict[slot] = para.detach().clone()
                else:
                    para.uniform_(-0.5, 0.5)

    def resolve_state(self, warm_up_rounds: int = 100) -> None:
        """After non-finite values: the remembered parameters, an optimiser without history at the initial learning
        rate, then `warm_up_rounds` warm-up steps."""
        if self._kstate is not None and self.kernel_route()[0]:
            self._kstate.forget_moments()          # (the step kernel has restored phi from the snapshot already)
        else:
            with torch.no_grad():
                for remembered, para in zip(self.state_dict, self.q.parameters()):
                    para.copy_(remembered.to(para.device))
            self._optimizer.state.clear()
            for group in self._optimizer.param_groups:
                group["lr"] = self.learning_rate
        self.warm_up(warm_up_rounds)

    # -- the eager iteration ----------------------------------------------------------------------------------
    def loss(self, x_o: Tensor) -> Tuple[Tensor, Tensor]:
        return self._loss(x_o)

    def _set_x(self, x_o: Tensor) -> None:
        if hasattr(self.potential_fn, "set_x"):
            self.potential_fn.set_x(x_o)
        else:
            self.potential_fn.x_o = x_o

    def step(self, x_o: Tensor) -> None:
        """One eager iteration: differentiate the surrogate loss, recover if it is not finite, clip the gradient norm
        to `clip_value`, optimiser and scheduler step, the displayed loss into the statistics; every 50th iteration
        the parameters are remembered (`update_state`)."""
        with self._q_in_torch():
            self._optimizer.zero_grad()
            surrogate, shown = self._loss(x_o.to(self.device))
            surrogate.backward(retain_graph=self.retain_graph)
            if not bool(torch.isfinite(surrogate)):
                self.resolve_state()
            nn.utils.clip_grad_norm_(self.q.parameters(), self.clip_value)
            self._optimizer.step()
        self._scheduler.step()
        self._sched_steps += 1
        self.update_loss_stats(shown.detach().cpu())
        if self.num_step % 50 == 0:
            self.update_state()

    # -- the kernel iteration ---------------------------------------------------------------------------------
    def _kernel_state(self, rows: int) -> _KernelState:
        if self._kstate is None:
            self._kstate = _KernelState(self.q, rows)
        self._kstate.reserve(rows)
        return self._kstate

    def _current_lr(self) -> float:
        gamma = float(self._sched_kwargs.get("gamma", 0.1))
        return float(self.learning_rate) * gamma ** self._sched_steps

    def _kernel_iteration(self, target: Callable, rows: int, cfg: dict, clip: float, ring: Tensor, lr: float,
                          export: bool = False):
        """draw -> target and its theta-gradient -> step.  `target(theta, track_gradients)` returns (rows,)."""
        from ctypes import byref

        from sbi_amd import _lib
        from sbi_amd._lib import VIConfigC

        q = self.q
        ks = self._kernel_state(rows)
        ks.step = (ks.step + 1) & 0xFFFFFFFF
        ks.adam_t += 1
        theta, _, eps = q._kernel_draw(rows, want_eps=export, seed=ks.seed, step=ks.step, phi=ks.phi)
        if cfg["method"] == _METHOD_CODE["fKL"]:
            with torch.no_grad():
                p = target(theta, False)
            r = None
        else:
            theta_g = theta.requires_grad_(True)
            with torch.enable_grad():
                p = target(theta_g, True)
                if p.requires_grad:
                    (r,) = torch.autograd.grad(p.sum(), theta_g, allow_unused=True)
                else:
                    r = None
            r = torch.zeros_like(theta) if r is None else r.to(torch.float32).contiguous()
        p = p.detach().to(torch.float32).reshape(-1).contiguous()
        c = VIConfigC(D=q._dim, full_cov=int(q._full_cov), method=cfg["method"], K=cfg.get("K", 1),
                      stick_the_landing=int(cfg.get("stick_the_landing", False)), dreg=int(cfg.get("dreg", False)),
                      unbiased=int(cfg.get("unbiased", False)), alpha=float(cfg.get("alpha", 0.0)))
        betas = self._opt_kwargs.get("betas", (0.9, 0.999))
        table, _ = q.link_table()
        grad_out = torch.empty_like(ks.phi) if export else None
        dev = ks.device
        with torch.cuda.device(dev):
            _lib.check(ks.lib.sbi_amd_vi_gauss_step(
                byref(c), _lib.ptr(p), _lib.ptr(r), rows, _lib.ptr(ks.phi), _lib.ptr(ks.exp_avg),
                _lib.ptr(ks.exp_avg_sq), _lib.ptr(ks.snapshot), _lib.ptr(table), float(clip), float(lr),
                float(betas[0]), float(betas[1]), 1e-8, ks.adam_t, ks.seed, ks.step, _lib.ptr(ks.workspace),
                _lib.ptr(ring), RING, _lib.ptr(ks.status), _lib.ptr(grad_out), _lib.current_stream(dev)),
                "vi_gauss_step")
        return theta.detach(), eps, grad_out

    def _kernel_warm_up(self, num_steps: int) -> None:
        prior = self.prior
        ks = self._kernel_state(32)
        cfg = {"method": _METHOD_CODE["rKL"]}
        lr = self._current_lr()
        for _ in range(num_steps):
            self._kernel_iteration(lambda th, track: prior.log_prob(th), 32, cfg, 0.0, ks.scratch_ring, lr)
        self.q.load_flat_parameters(ks.phi)

    def kernel_steps(self, x_o: Tensor, num_iters: int) -> None:
        """`num_iters` (<= READBACK) iterations on the kernel route with no host synchronisation."""
        assert 0 < num_iters <= READBACK
        rows = self._rows_per_step()
        cfg = self._kernel_config()
        ks = self._kernel_state(rows)
        self._set_x(x_o.to(self.device))
        ks.ring.fill_(float("nan"))                # a step the guard skips leaves its slot non-finite
        potential = self.potential_fn
        self._block_t0 = ks.adam_t
        for _ in range(num_iters):
            self._kernel_iteration(lambda th, track: potential(th, track_gradients=track), rows, cfg,
                                   self.clip_value, ks.ring, self._current_lr())
            self._sched_steps += 1
        self._block_iters = num_iters

    def kernel_read_back(self) -> Tuple[Tensor, bool]:
        """The ONE synchronisation of a block: (its losses in order, whether the guard skipped a step since the last
        read-back).  Also copies phi into q's parameters."""
        ks = self._kstate
        host = ks.block.cpu()
        ring = host[4:].view(torch.float32)
        ts = [(self._block_t0 + 1 + i) % RING for i in range(self._block_iters)]
        losses = ring[ts].clone()
        skipped = int(host[0]) > ks.nonfinite_seen
        ks.nonfinite_seen = int(host[0])
        self.q.load_flat_parameters(ks.phi)
        return losses, skipped

    def kernel_gradient_probe(self, x_o: Tensor):
        """One kernel-route iteration with eps and the gradient exported: (theta, eps, grad) -- for the tests."""
        rows = self._rows_per_step()
        ks = self._kernel_state(rows)
        self._set_x(x_o.to(self.device))
        potential = self.potential_fn
        out = self._kernel_iteration(lambda th, track: potential(th, track_gradients=track), rows,
                                     self._kernel_config(), self.clip_value, ks.scratch_ring, self._current_lr(),
                                     export=True)
        self.q.load_flat_parameters(ks.phi)
        return out

    # -- convergence ------------------------------------------------------------------------------------------
    # One (4, capacity) fp32 table holds the history: rows = displayed loss, its moving average, the moving spread and
    # the slope estimate.  sbi's attribute names are views of its rows.  Entries not yet written hold 1 in the first
    # 2000 columns and 0 in columns added later.
    _LOSS, _AVG, _STD, _SLOPE = range(4)
    _CHUNK = 2000

    losses = property(lambda self: self._history[self._LOSS])
    moving_average = property(lambda self: self._history[self._AVG])
    moving_std = property(lambda self: self._history[self._STD])
    moving_slope = property(lambda self: self._history[self._SLOPE])

    def reset_loss_stats(self) -> None:
        self._history = torch.ones(4, self._CHUNK)
        self.num_step = 0

    def converged(self, considered_values: int = 50) -> bool:
        """True once the slope estimates of the last `considered_values` iterations average to less than `eps` in
        magnitude."""
        n = self.num_step
        if n < considered_values:
            return False
        return abs(float(self.moving_slope[n - considered_values:n].mean())) < self.eps

    def update_loss_stats(self, loss: Tensor, window: int = 20) -> None:
        """Appends one displayed loss.  With L the losses, A the moving average, S the spread, G the slope, w the
        window and b = max(n - w, 0):  A_n = A_{n-1} + (L_n - L_b) / w;  S_n = |S_{n-1} + (L_n - L_b) / w - S_{n-1} /
        (w - 1)|;  G_n = (L_n - A_b) / w.  The first loss starts L and A; a non-finite loss leaves L_n unwritten and
        repeats A, S and G."""
        n = self.num_step
        H = self._history
        if n >= H.shape[1]:
            H = self._history = torch.cat([H, torch.zeros(4, self._CHUNK)], dim=1)
        value = torch.as_tensor(loss, dtype=H.dtype).reshape(())
        if n == 0:
            H[self._LOSS, 0] = H[self._AVG, 0] = value
        elif not bool(torch.isfinite(value)):
            H[self._AVG:, n] = H[self._AVG:, n - 1]
        else:
            b = max(n - window, 0)
            drift = (value - H[self._LOSS, b]) / window
            H[self._LOSS, n] = value
            H[self._SLOPE, n] = (value - H[self._AVG, b]) / window
            H[self._STD, n] = (H[self._STD, n - 1] + drift - H[self._STD, n - 1] / (window - 1)).abs()
            H[self._AVG, n] = H[self._AVG, n - 1] + drift
        self.num_step = n + 1

    def get_loss_stats(self):
        """(moving average, moving spread) after the last iteration."""
        last = self.num_step - 1
        return self._history[self._AVG, last], self._history[self._STD, last]

    def update(self, kwargs: Dict) -> None:
        """Takes new settings from `VIPosterior.train` (its arguments plus its keyword arguments): the posterior
        itself under "self" hands over q, potential and prior; `learning_rate`, `retain_graph` and every name in
        `HYPER_PARAMETERS` are stored; then optimiser and scheduler are built anew (classes from "optimizer" /
        "scheduler" when given) from whichever settings their constructors name."""
        settings = dict(kwargs)
        posterior = settings.pop("self", None)
        if posterior is not None:
            if posterior.q is not self.q:
                self._kstate = None
            self.q, self.potential_fn, self.prior = posterior.q, posterior.potential_fn, posterior._prior
        self.retain_graph = settings.get("retain_graph", self.retain_graph)
        self.learning_rate = settings.get("learning_rate", self.learning_rate)
        for name in self.HYPER_PARAMETERS:
            if name in settings:
                setattr(self, name, settings[name])
        opt_type = settings.pop("optimizer", type(self._optimizer))
        sched_type = settings.pop("scheduler", type(self._scheduler))
        settings["lr"] = self.learning_rate
        self._build_torch_optimizer(opt_type, sched_type, settings)
        self._sched_steps = 0                      # (a new optimiser and scheduler: fresh moments, lr from the start)
        if self._kstate is not None:
            self._kstate.forget_moments()


def register_VI_method(name: Optional[str] = None) -> Callable:
    def _register(cls):
        cls_name = cls.__name__ if name is None else name
        if cls_name in _VI_method:
            raise ValueError(f"The VI method {cls_name} is already registered")
        _VI_method[cls_name] = cls
        return cls

    return _register


def get_VI_method(name: str):
    return _VI_method[name]


def get_default_VI_method() -> List[str]:
    return list(_VI_method.keys())


@register_VI_method(name="rKL")
class ElboOptimizer(DivergenceOptimizer):
    r"""Reverse KL, D_KL(q || p(.|x_o)), by maximising the ELBO.  `stick_the_landing` (Roeder et al. 2017) evaluates
    log q with the parameters held fixed, so that the gradient flows through the draws only: lower variance near
    convergence."""

    def __init__(self, *args, stick_the_landing: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.stick_the_landing = stick_the_landing
        self._frozen_q = detach_and_deepcopy(self.q)          # same family, parameters without gradient
        for p in self._frozen_q.parameters():
            p.requires_grad_(False)
        self.eps = 1e-5
        self.HYPER_PARAMETERS += ["stick_the_landing"]

    def _kernel_config(self) -> Optional[dict]:
        return {"method": _METHOD_CODE["rKL"], "stick_the_landing": self.stick_the_landing}

    def _frozen_log_q(self, theta: Tensor) -> Tensor:
        with torch.no_grad():
            for live, frozen in zip(self.q.parameters(), self._frozen_q.parameters()):
                if frozen.shape != live.shape or frozen.device != live.device:
                    frozen.data = live.detach().clone()
                else:
                    frozen.copy_(live)
        if isinstance(self._frozen_q, LearnableGaussian):
            self._frozen_q.force_eager = True
        return self._frozen_q.log_prob(theta)

    def _elbo_terms(self, x_o: Tensor, n: int) -> Tensor:
        """e_i = potential(theta_i) - log q(theta_i) at n reparameterised draws."""
        theta, log_q = self._reparameterised_draws(n)
        if self.stick_the_landing:
            log_q = self._frozen_log_q(theta)
        self._set_x(x_o)
        return self.potential_fn(theta, track_gradients=True) - log_q

    def _loss(self, x_o: Tensor) -> Tuple[Tensor, Tensor]:
        negative_elbo = -self._elbo_terms(x_o, self.n_particles).mean()
        return negative_elbo, negative_elbo.detach().clone()


@register_VI_method(name="IW")
class IWElboOptimizer(ElboOptimizer):
    """The importance-weighted ELBO (Burda et al. 2016) over `n_particles` groups of K draws; `dreg`: the doubly
    reparameterised estimator (Tucker et al. 2018), which implies `stick_the_landing`."""

    def __init__(self, *args, K: int = 8, dreg: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.K = K
        self.loss_name = "iwelbo"
        self.eps = 1e-7
        self.dreg = dreg
        self.HYPER_PARAMETERS += ["K", "dreg"]
        self.stick_the_landing = self.stick_the_landing or dreg

    def _rows_per_step(self) -> int:
        return self.n_particles * self.K

    def _kernel_config(self) -> Optional[dict]:
        return {"method": _METHOD_CODE["IW"], "K": self.K, "dreg": self.dreg,
                "stick_the_landing": self.stick_the_landing or self.dreg}

    def _loss(self, x_o: Tensor) -> Tuple[Tensor, Tensor]:
        """Surrogate: the group-wise self-normalised weights (held constant; squared under dreg) times the terms, summed
        per group, averaged over groups.  Displayed: -mean_g log(mean_k exp(e_gk) + 1e-20)."""
        e = self._elbo_terms(x_o, self._rows_per_step()).reshape(self.n_particles, self.K)
        with torch.no_grad():
            w = torch.softmax(e, dim=1)
            w = w.square() if self.dreg else w
            shown = -torch.log((e.exp() + 1e-20).mean(dim=1)).mean()
        return -(w * e).sum(dim=1).mean(), shown


@register_VI_method(name="fKL")
class ForwardKLOptimizer(DivergenceOptimizer):
    """Forward KL, D_KL(p(.|x_o) || q), by self-normalised importance sampling with q as the proposal (Jerfel et al.
    2021).  `n_particles` reduces the bias too."""

    def __init__(self, *args, proposal: str = "q", weight_transform: Callable = _identity_weight_transform, **kwargs):
        super().__init__(*args, **kwargs)
        self.proposal = proposal
        self.weight_transform = weight_transform
        self._loss_name = "forward_kl"
        self.HYPER_PARAMETERS += ["weight_transform", "proposal"]
        self.eps = 1e-5

    def _kernel_config(self) -> Optional[dict]:
        return {"method": _METHOD_CODE["fKL"]}

    def _loss(self, x_o: Tensor) -> Tuple[Tensor, Tensor]:
        """Draws of q without gradient; w = weight_transform(p / q), normalised to sum 1 and held constant.
        Surrogate: -sum w log q.  Displayed: sum w (log p - log q)."""
        theta = self.q.sample((self.n_particles,))
        if hasattr(self.q, "clear_cache"):
            self.q.clear_cache()
        log_q = self.q.log_prob(theta)
        self._set_x(x_o)
        log_p = self.potential_fn(theta, track_gradients=False)
        with torch.no_grad():
            w = self.weight_transform(torch.exp(log_p - log_q))
            w = w / w.sum()
            shown = (w * (log_p - log_q)).sum()
        return -(w * log_q).sum(), shown


@register_VI_method(name="alpha")
class RenyiDivergenceOptimizer(ElboOptimizer):
    """Renyi alpha divergences (Li & Turner 2016): alpha < 1 mass covering, alpha > 1 mode seeking."""

    def __init__(self, *args, alpha: float = 0.5, unbiased: bool = False, dreg: bool = False, **kwargs):
        self.alpha = alpha
        self.unbiased = unbiased
        super().__init__(*args, **kwargs)
        self.HYPER_PARAMETERS += ["alpha", "unbiased", "dreg"]
        self.eps = 1e-5
        self.dreg = dreg
        self.stick_the_landing = self.stick_the_landing or dreg

    def _kernel_config(self) -> Optional[dict]:
        return {"method": _METHOD_CODE["alpha"], "alpha": self.alpha, "unbiased": self.unbiased, "dreg": self.dreg,
                "stick_the_landing": self.stick_the_landing or self.dreg}

    def _log_mean_weight(self, e: Tensor) -> Tuple[Tensor, Tensor]:
        """((1 - alpha) e, log of the mean of exp of it)."""
        scaled = (1.0 - self.alpha) * e
        return scaled, torch.logsumexp(scaled, dim=0) - math.log(self.n_particles)

    def _loss(self, x_o: Tensor) -> Tuple[Tensor, Tensor]:
        """The variational Renyi bound, displayed as -m / (1 - alpha) with m the log mean weight.  Biased surrogate:
        -mean(w e) with w = exp((1 - alpha) e - m) held constant (squared under dreg).  Unbiased surrogate: -exp(m)
        itself, differentiated through m -- with the particles scaled by (1 - alpha) BEFORE the weights scale them
        again, as the reference does."""
        e = self._elbo_terms(x_o, self.n_particles)
        if self.unbiased:
            _, m = self._log_mean_weight((1.0 - self.alpha) * e)
            return -m.exp(), (-m / (1.0 - self.alpha)).detach().clone()
        with torch.no_grad():
            scaled, m = self._log_mean_weight(e)
            w = torch.exp(scaled - m)
            w = w.square() if self.dreg else w
        return -(w * e).mean(), -m / (1.0 - self.alpha)
