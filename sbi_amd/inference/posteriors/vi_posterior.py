"""``VIPosterior`` -- variational inference over a potential.

Mirror of sbi/inference/posteriors/vi_posterior.py (constructor, ``set_q`` / ``q``, ``set_vi_method`` / ``vi_method``,
``set_default_x``, ``sample``, the NORMALISED ``log_prob``, ``train`` with its hyper-parameter validation, ``evaluate``,
``map``, ``to``, pickling without the optimiser) for the single-x mode.  It gives the likelihood- and ratio-based
methods a posterior that samples at no extra cost and has a normalised density.

Two routes with the same semantics (``kernel_route()`` says which, and why):

* kernel route -- q is ``"gaussian"`` / ``"gaussian_diag"`` (or a ``LearnableGaussian``) in fp32 on a ROCm device,
  D <= 16, at most 65 536 particles per step, Adam + ExponentialLR, identity ``weight_transform`` and a link transform
  that decomposes per dimension: an iteration is two launches of our own around the potential
  (samplers/vi/vi_divergence_optimizers.py, include/sbi_amd_vi.h) and the host reads the loss ring and the status block
  every 25 iterations.  Training therefore stops at the first multiple of 25 at which the reference would have
  stopped, up to 24 iterations later.
* eager route -- the written formulas in torch with autograd: the host, anything outside the envelope, a user
  ``torch.distributions.Distribution`` and a builder ``Callable(event_shape, link_transform, device)``.
  ``posterior.force_eager = True`` pins it.

Refused with NotImplementedError: the flow families (``"maf"`` -- the reference's default --, ``"nsf"``, ``"naf"``,
``"unaf"``, ``"nice"``, ``"sospf"``, ``"gf"``: Zuko is not available and a reparameterised flow needs a reverse-mode
pass through the sampling direction that no kernel here has) and ``train_amortized``.
"""

from __future__ import annotations

import copy
from functools import partial
from typing import Callable, Dict, Iterable, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor
from torch.distributions import Distribution

from sbi_amd.samplers.vi.vi_divergence_optimizers import READBACK, get_VI_method
from sbi_amd.samplers.vi.vi_quality_control import get_quality_metric
from sbi_amd.samplers.vi.vi_utils import (AdaptedVariationalDistribution, LearnableGaussian,
                                          check_variational_distribution, detach_and_deepcopy,
                                          move_distribution)
from sbi_amd.utils.sbiutils import gradient_ascent, mcmc_transform
from sbi_amd.utils.torchutils import ensure_theta_batched, process_device

_FLOW_FAMILIES = {"maf", "nsf", "naf", "unaf", "nice", "sospf", "gf"}
_GAUSSIAN_FAMILIES = ("gaussian", "gaussian_diag")


def _flow_refusal(name: str) -> NotImplementedError:
    return NotImplementedError(
        f"sbi_amd: the variational family q='{name}' is a normalizing flow, which VIPosterior does not provide here "
        "(Zuko is not available, and a reparameterised flow needs a reverse-mode pass through the sampling direction "
        "that no kernel has). Use q='gaussian' (full covariance) or q='gaussian_diag', pass your own "
        "torch.distributions.Distribution, or a builder Callable(event_shape, link_transform, device).")


class _QRecipe:
    """What it takes to make a FRESH variational distribution of the kind `set_q` was given (`retrain_from_scratch`):
    a family name needs only its covariance structure, a builder is called again, a user distribution is restored from
    the copy taken before any training; a ready-made family instance ("instance") cannot be made again."""

    def __init__(self, kind: str, payload=None):
        self.kind, self.payload = kind, payload

    def copy(self) -> "_QRecipe":
        return _QRecipe(self.kind, self.payload)

    def make(self, posterior: "VIPosterior"):
        event_shape = posterior._prior.event_shape
        if self.kind == "gaussian":
            return LearnableGaussian(event_shape[0], full_covariance=self.payload,
                                     link_transform=posterior.link_transform, device=posterior._device)
        if self.kind == "callable":
            return self.payload(event_shape, posterior.link_transform, device=posterior._device)
        if self.kind == "distribution":
            return detach_and_deepcopy(self.payload)
        raise ValueError("Cannot rebuild `q`: it was passed as an already-built distribution, which does not say how "
                         "to build a new one. To use `retrain_from_scratch`, pass `q` as a variational family name, a "
                         "`Callable`, or a `Distribution`.")


class VIPosterior:
    def __init__(self, potential_fn: Callable, prior: Optional[Distribution] = None, q="maf", theta_transform=None,
                 vi_method: str = "rKL", device: Optional[Union[str, torch.device]] = None,
                 x_shape: Optional[torch.Size] = None, parameters: Optional[Iterable] = None,
                 modules: Optional[Iterable] = None, num_transforms: int = 5, hidden_features: int = 50,
                 z_score_theta: str = "independent", z_score_x: str = "independent"):
        if not callable(potential_fn):
            raise TypeError("potential_fn must be a callable potential (BasePotential / CustomPotential role).")
        self.potential_fn = potential_fn
        if device is None:
            device = getattr(potential_fn, "device", "cpu")
        self._device = process_device(device)
        self.theta_transform = theta_transform
        self.x_shape = x_shape
        self._x: Optional[Tensor] = None
        self._map: Optional[Tensor] = None
        self._trained_on: Optional[Tensor] = None
        self.force_eager = False
        try:
            self.potential_fn.device = self._device
        except AttributeError:
            pass
        if hasattr(self.potential_fn, "to"):
            self.potential_fn.to(self._device)

        if prior is not None:
            self._prior = prior
        elif isinstance(getattr(self.potential_fn, "prior", None), Distribution):
            self._prior = self.potential_fn.prior
        elif isinstance(q, VIPosterior) and isinstance(q._prior, Distribution):
            self._prior = q._prior
        else:
            raise ValueError("We could not find a suitable prior distribution within `potential_fn` or `q` (if a "
                             "VIPosterior is given). Please explicitly specify a prior.")
        self._prior = move_distribution(self._prior, self._device)
        self._optimizer = None
        self._mode: Optional[str] = None           # None (not trained) or "single_x"
        self._num_transforms = num_transforms
        self._hidden_features = hidden_features
        self._z_score_theta = z_score_theta
        self._z_score_x = z_score_x

        # in contrast to MCMC, q lives in constrained space: the link maps unconstrained -> constrained
        if theta_transform is None:
            self.link_transform = mcmc_transform(self._prior, device=self._device).inv
        else:
            self.link_transform = theta_transform.inv
        self.set_q(q, parameters=parameters, modules=modules)
        self.set_vi_method(vi_method)
        self._purpose = ("It provides Variational inference to .sample() from the posterior and can evaluate the "
                         "_normalized_ posterior density with .log_prob().")

    # -- x_o handling ---------------------------------------------------------------------------------------
    @property
    def default_x(self) -> Optional[Tensor]:
        return self._x

    def set_default_x(self, x: Tensor) -> "VIPosterior":
        x = torch.as_tensor(x, dtype=torch.float32)
        if not torch.isfinite(x).all():
            raise ValueError("x_o contains NaN or Inf values.")
        self._x = x.reshape(1, -1).to(self._device) if x.dim() <= 1 else x.to(self._device)
        self._map = None
        return self

    def _x_else_default_x(self, x: Optional[Tensor]) -> Tensor:
        if x is not None:
            x = torch.as_tensor(x, dtype=torch.float32)
            return (x.reshape(1, -1) if x.dim() <= 1 else x).to(self._device)
        if self._x is None:
            raise ValueError("Context `x` needed when a default has not been set. If you'd like to have a default, "
                             "use the `.set_default_x()` method.")
        return self._x

    def _fit_on(self, x: Tensor) -> bool:
        t = self._trained_on
        return t is not None and tuple(t.shape) == tuple(x.shape) and not bool((x != t.to(x.device)).any())

    def to(self, device: Union[str, torch.device]) -> "VIPosterior":
        device = process_device(device)
        self._device = device
        if hasattr(self.potential_fn, "to"):
            self.potential_fn.to(device)
        self._prior = move_distribution(self._prior, device)
        if self.theta_transform is None:
            self.link_transform = mcmc_transform(self._prior, device=device).inv
        else:
            self.link_transform = self.theta_transform.inv
        for name in ("_x", "_map", "_trained_on"):
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name).to(device))
        if hasattr(self._q, "to"):
            self._q.to(device)
        if hasattr(self._q, "_link_transform"):
            self._q._link_transform = self.link_transform
        self._optimizer = None                     # (its buffers live on the old device; `train` builds a new one)
        return self

    # -- the variational family -------------------------------------------------------------------------------
    @property
    def q(self):
        """The variational posterior."""
        return self._q

    @q.setter
    def q(self, q) -> None:
        self.set_q(q)

    def set_q(self, q, parameters: Optional[Iterable] = None, modules: Optional[Iterable] = None) -> None:
        """Defines the variational family: "gaussian" / "gaussian_diag", a `LearnableGaussian`, a parameterised
        `torch.distributions.Distribution` (its trainable tensors through `parameters()` or the `parameters` argument),
        a builder `Callable(event_shape, link_transform, device) -> Distribution`, or another `VIPosterior` (copied:
        multi-round training).  Anything but another posterior forgets what q was trained on."""
        if isinstance(q, VIPosterior):
            built, recipe = self._adopt(q)
        else:
            if isinstance(q, str):
                recipe = self._recipe_for_name(q)
                built = recipe.make(self)
            elif isinstance(q, LearnableGaussian):
                built, recipe = q, _QRecipe("instance")
            elif isinstance(q, Distribution):
                built = q if isinstance(q, AdaptedVariationalDistribution) else AdaptedVariationalDistribution(
                    q, self._prior, self.link_transform, parameters=parameters or [], modules=modules or [])
                recipe = _QRecipe("distribution", detach_and_deepcopy(built))      # (an adapted q is never wrapped twice)
            elif callable(q):
                recipe = _QRecipe("callable", q)
                built = recipe.make(self)
            else:
                built, recipe = q, _QRecipe("instance")
            self._trained_on = None
        if not isinstance(built, LearnableGaussian):
            if not isinstance(built, Distribution):
                raise ValueError(f"Variational distribution must be a Distribution, got {type(built)}. Please create "
                                 "an issue on github https://github.com/mackelab/sbi/issues")
            check_variational_distribution(built, self._prior)
        self._q, self._q_recipe = built, recipe

    @staticmethod
    def _recipe_for_name(name: str) -> _QRecipe:
        if name in _FLOW_FAMILIES:
            raise _flow_refusal(name)
        if name not in _GAUSSIAN_FAMILIES:
            supported = sorted(_FLOW_FAMILIES) + list(_GAUSSIAN_FAMILIES)
            raise ValueError(f"Unknown variational family '{name}'. Supported options: {supported}")
        return _QRecipe("gaussian", name == "gaussian")

    def _adopt(self, other: "VIPosterior"):
        """An independent copy of another posterior's q on this device, with what goes with it: its recipe, method,
        prior, default x and the x it was trained on."""
        self._trained_on, self._mode, self._prior, self._x = other._trained_on, other._mode, other._prior, other._x
        self.vi_method = other.vi_method
        copied = detach_and_deepcopy(other.q)
        if hasattr(copied, "to"):
            copied.to(self._device)
        return copied, other._q_recipe.copy()

    @property
    def vi_method(self) -> str:
        """One of [rKL, fKL, IW, alpha]."""
        return self._vi_method

    @vi_method.setter
    def vi_method(self, method: str) -> None:
        self.set_vi_method(method)

    def set_vi_method(self, method: str) -> "VIPosterior":
        self._vi_method = method
        self._optimizer_builder = get_VI_method(method)
        return self

    def kernel_route(self) -> Tuple[bool, str]:
        """(True, "") when `train` runs on the HIP kernels, else (False, why it runs eager).  Before the first `train`
        the answer is for the default optimiser arguments."""
        if self.force_eager:
            return False, "force_eager is set"
        if self._optimizer is not None and isinstance(self._optimizer, self._optimizer_builder) \
                and self._optimizer.q is self._q:
            return self._optimizer.kernel_route()
        probe = self._optimizer_builder(self.potential_fn, self._q, lr=1e-3, gamma=0.999, prior=self._prior)
        return probe.kernel_route()

    # -- sampling and evaluation ------------------------------------------------------------------------------
    def _not_fit(self, x: Tensor) -> ValueError:
        return ValueError(f"The variational posterior was not fit on the specified observation {x}. Please train "
                          "using posterior.train().")

    def _q_respects_route(self):
        if isinstance(self._q, LearnableGaussian):
            self._q.force_eager = self.force_eager
        return self._q

    def sample(self, sample_shape=torch.Size(), x: Optional[Tensor] = None, show_progress_bars: bool = True) -> Tensor:
        """Draws from q; `x` must be the observation q was trained on (or None for the default)."""
        x = self._x_else_default_x(x)
        if not self._fit_on(x):
            raise self._not_fit(x)
        sample_shape = torch.Size(sample_shape)
        samples = self._q_respects_route().sample(sample_shape)
        return samples.reshape((*sample_shape, samples.shape[-1]))

    def sample_batched(self, sample_shape, x: Tensor, max_sampling_batch_size: int = 10000,
                       show_progress_bars: bool = True) -> Tensor:
        raise NotImplementedError("Batched sampling is not implemented for single-x VI mode. Use train_amortized() to "
                                  "train an amortized posterior, or call sample() in a loop: "
                                  "[posterior.sample(shape, x_o) for x_o in x].")

    def log_prob(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False) -> Tensor:
        """log q(theta): the NORMALISED density of the variational posterior."""
        with torch.set_grad_enabled(track_gradients):
            theta = ensure_theta_batched(torch.as_tensor(theta)).to(self._device)
            x = self._x_else_default_x(x)
            if not self._fit_on(x):
                raise self._not_fit(x)
            return self._q_respects_route().log_prob(theta)

    # -- training ---------------------------------------------------------------------------------------------
    def _new_optimizer(self, learning_rate, clip_value, gamma, n_particles, kwargs):
        return self._optimizer_builder(self.potential_fn, self.q, lr=learning_rate, clip_value=clip_value, gamma=gamma,
                                       n_particles=n_particles, prior=self._prior, **kwargs)

    def train(self, x: Optional[Tensor] = None, n_particles: int = 256, learning_rate: float = 1e-3,
              gamma: float = 0.999, max_num_iters: int = 2000, min_num_iters: int = 10, clip_value: float = 10.0,
              warm_up_rounds: int = 100, retrain_from_scratch: bool = False, reset_optimizer: bool = False,
              show_progress_bar: bool = True, check_for_convergence: bool = True, quality_control: bool = True,
              quality_control_metric: str = "psis", **kwargs) -> "VIPosterior":
        """Fits q to the posterior at one observation.  `kwargs` go to the `DivergenceOptimizer`: eps, retain_graph,
        optimizer, scheduler, alpha, K, stick_the_landing, dreg, unbiased, weight_transform."""
        for ok, complaint in ((n_particles > 0, f"n_particles must be positive, got {n_particles}"),
                              (learning_rate > 0, f"learning_rate must be positive, got {learning_rate}"),
                              (0 < gamma <= 1, f"gamma must be in (0, 1], got {gamma}"),
                              (max_num_iters > 0, f"max_num_iters must be positive, got {max_num_iters}"),
                              (min_num_iters >= 0, f"min_num_iters must be non-negative, got {min_num_iters}"),
                              (clip_value > 0, f"clip_value must be positive, got {clip_value}")):
            if not ok:
                raise ValueError(complaint)

        settings = dict(x=x, n_particles=n_particles, learning_rate=learning_rate, gamma=gamma,
                        max_num_iters=max_num_iters, min_num_iters=min_num_iters, clip_value=clip_value,
                        warm_up_rounds=warm_up_rounds, **kwargs)
        settings["self"] = self
        fresh = lambda: self._new_optimizer(learning_rate, clip_value, gamma, n_particles, kwargs)     # noqa: E731
        if retrain_from_scratch:
            recipe = self._q_recipe
            self.set_q(recipe.make(self))              # (raises for a ready-made instance)
            self._q_recipe = recipe                    # (set_q took the new q for an instance)
            self._optimizer = fresh()
        elif reset_optimizer or not isinstance(self._optimizer, self._optimizer_builder):
            self._optimizer = fresh()                  # (none yet, asked for, or one of another divergence)
        else:
            self._optimizer.update(settings)
        optimizer = self._optimizer

        x = self._x_else_default_x(x)
        if not torch.isfinite(x).all():
            raise ValueError("x contains NaN or Inf values.")
        seen_before = self._fit_on(x)
        optimizer.to(self._device)
        optimizer.force_eager = self.force_eager
        optimizer.reset_loss_stats()
        on_kernels = optimizer.kernel_route()[0]
        if on_kernels and optimizer._kstate is not None:
            optimizer._kstate.phi.copy_(self._q.flat_parameters())      # (q may have been touched in between)

        bar = None
        if show_progress_bar:
            from tqdm.auto import tqdm

            bar = tqdm(total=max_num_iters)
        if reset_optimizer or not (optimizer.warm_up_was_done or seen_before):
            if bar is not None:
                bar.set_description("Warmup phase, this may take a few seconds...")
            optimizer.warm_up(warm_up_rounds)

        def finished(i: int) -> bool:
            """After iteration i's loss has entered the statistics: moves the bar, asks for convergence."""
            mean_loss, std_loss = optimizer.get_loss_stats()
            if bar is not None:
                bar.update(1)
                bar.set_description(f"Loss: {np.round(float(mean_loss), 2)}, Std: {np.round(float(std_loss), 2)}")
            if check_for_convergence and i > min_num_iters and optimizer.converged():
                if bar is not None:
                    print(f"\nConverged with loss: {np.round(float(mean_loss), 2)}")
                return True
            return False

        if on_kernels:
            self._train_on_kernels(optimizer, x, max_num_iters, finished)
        else:
            for i in range(max_num_iters):
                optimizer.step(x)
                if finished(i):
                    break
        if bar is not None:
            bar.close()
        self._trained_on, self._mode = x, "single_x"

        if quality_control:
            try:
                self.evaluate(quality_control_metric=quality_control_metric)
            except Exception as e:
                print(f"Quality control showed a low quality of the variational posterior. We are automatically "
                      f"retraining the variational posterior from scratch with a smaller learning rate. "
                      f"Alternatively, if you want to skip quality control, please retrain with "
                      f"`VIPosterior.train(..., quality_control=False)`. \nThe error that occured is: {e}")
                self.train(learning_rate=learning_rate * 0.1, retrain_from_scratch=True, reset_optimizer=True)
        return self

    @staticmethod
    def _train_on_kernels(optimizer, x: Tensor, max_num_iters: int, finished: Callable[[int], bool]) -> None:
        """Blocks of READBACK iterations without a host synchronisation; after each, the block's losses enter the
        statistics in order.  The first loss at which the eager loop would have stopped ends the bookkeeping (later
        losses of that block are dropped) and the training."""
        done = 0
        while done < max_num_iters:
            block = min(READBACK, max_num_iters - done)
            optimizer.kernel_steps(x, block)
            losses, skipped = optimizer.kernel_read_back()
            for j in range(block):
                optimizer.update_loss_stats(losses[j])
                if finished(done + j):
                    return
            done += block
            if skipped:
                optimizer.resolve_state()

    def train_amortized(self, *args, **kwargs):
        raise NotImplementedError(
            "sbi_amd: amortized variational inference (`train_amortized`) needs a conditional normalizing flow as q, "
            "which VIPosterior does not provide here. Use `train(x=x_o)` per observation with q='gaussian' or "
            "q='gaussian_diag'.")

    def evaluate(self, quality_control_metric: str = "psis", N: int = int(5e4)) -> float:
        """Prints (and returns) a quality score of q: "psis" (tails of the importance weights), "prop" or "prop_prior"
        (proportionality of q and the potential)."""
        quality_control_fn, quality_control_msg = get_quality_metric(quality_control_metric)
        metric = round(float(quality_control_fn(self, N=N)), 3)
        print(f"Quality Score: {metric} " + quality_control_msg)
        return metric

    def map(self, x: Optional[Tensor] = None, num_iter: int = 1_000, num_to_optimize: int = 100,
            learning_rate: float = 0.01, init_method: Union[str, Tensor] = "proposal", num_init_samples: int = 10_000,
            save_best_every: int = 10, show_progress_bars: bool = False, force_update: bool = False) -> Tensor:
        """Gradient ascent on the potential from draws of q (`init_method="proposal"` or "posterior") or from given
        points (base_posterior.py:216-323)."""
        if x is None and self._map is not None and not force_update:
            return self._map
        self.proposal = self.q
        self.potential_fn.set_x(self._x_else_default_x(x))
        if isinstance(init_method, Tensor):
            starts = init_method
        elif init_method in ("proposal", "posterior"):
            with torch.no_grad():
                starts = self._q_respects_route().sample(torch.Size((num_init_samples,)))
        else:
            raise ValueError("init_method must be 'posterior', 'proposal' or a tensor of initial parameters.")
        transform = self.theta_transform
        if transform is None:
            transform = mcmc_transform(self._prior, device=self._device)
        best, _ = gradient_ascent(partial(self.potential_fn, track_gradients=True), starts.to(self._device), transform,
                                  num_iter, num_to_optimize, learning_rate, save_best_every, show_progress_bars)
        self._map = best
        return best

    # -- pickling -----------------------------------------------------------------------------------------------
    def __getstate__(self) -> Dict:
        """Without the optimiser (device buffers, closures): `train` builds a new one when it is missing."""
        state = self.__dict__.copy()
        state["_optimizer"] = None
        state.pop("proposal", None)
        return state

    def __setstate__(self, state: Dict) -> None:
        self.__dict__.update(state)

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update({k: copy.deepcopy(v, memo) for k, v in self.__getstate__().items()})
        return new
