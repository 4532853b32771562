"""``MCMCPosterior`` -- sample a potential with the device-resident vectorised slice sampler.

Mirror of sbi/inference/posteriors/mcmc_posterior.py:41-368, :517-812 for ``method="slice_np_vectorized"``
(sbi's default; ``"slice_np"`` runs the same sampler here -- the serial numpy variant has no reason to exist
on a GPU).  Sampling happens in the unconstrained / z-scored space of ``theta_transform``
(``mcmc_transform(prior)``), chains are initialised by ``proposal`` / ``sir`` / ``resample`` /
``latest_sample`` for all chains at once, every tick evaluates the potential of all chains with the batched
log_prob kernel (single x_o broadcast, 44 B per evaluation) and advances them with
``sbi_amd_mcmc_slice_tick``.  Pyro / PyMC samplers are not part of this path.
"""

from __future__ import annotations

from math import ceil
from typing import Any, Callable, Dict, Optional, Union

import torch
from torch import Tensor

from sbi_amd.neural_nets.estimators.shape_handling import reshape_to_batch_event
from sbi_amd.samplers.mcmc import SliceSamplerVectorized, proposal_init, resample_given_potential_fn, sir_init
from sbi_amd.utils.sbiutils import mcmc_transform
from sbi_amd.utils.torchutils import ensure_theta_batched, process_device

_SLICE_METHODS = ("slice_np", "slice_np_vectorized")
# Batched init (`sir` / `resample`): candidate rows per paired potential call.  Observations are grouped so that a call
# weighs at most this many (theta, x) pairs -- 2^20 rows are 4 MiB per fp32 column -- and one observation's
# num_chains x num_candidate_samples candidates always go through in one call, however many they are.
INIT_ROWS_PER_CALL = 1 << 20
_OTHER_METHODS = ("hmc_pyro", "nuts_pyro", "slice_pymc", "hmc_pymc", "nuts_pymc")


def unconstrained_potential(potential_fn, transform, device):
    """The slice sampler walks UNCONSTRAINED space: returns u -> potential of the constrained point T^-1(u), corrected
    by the volume change of the map (what mcmc_posterior.py:953-986 gets from utils/potentialutils.py:15-51)."""

    def density_of(u) -> Tensor:
        u = ensure_theta_batched(torch.as_tensor(u, dtype=torch.float32)).to(device)
        constrained = transform.inv(u)
        volume = transform.log_abs_det_jacobian(constrained, u).to(device)
        return potential_fn(constrained, track_gradients=False).to(device) - volume

    return density_of


def _process_thin_default(thin: int) -> int:
    """mcmc_posterior.py:1069-1082: the default changed from 10 to 1 upstream; -1 selects it."""
    return 1 if thin == -1 else thin


class MCMCPosterior:
    def __init__(self, potential_fn: Callable, proposal: Any, theta_transform=None,
                 method: str = "slice_np_vectorized", thin: int = -1, warmup_steps: int = 200, num_chains: int = 20,
                 init_strategy: str = "resample", init_strategy_parameters: Optional[Dict[str, Any]] = None,
                 num_workers: int = 1, mp_context: str = "spawn", device: Optional[str] = None,
                 x_shape: Optional[torch.Size] = None):
        if method not in _SLICE_METHODS + _OTHER_METHODS:
            raise NameError(f"The sampling method {method} is not implemented!")
        self.potential_fn = potential_fn
        self.proposal = proposal
        if device is None:
            device = getattr(potential_fn, "device", "cpu")
        self._device = process_device(device)
        # keep the constrained <- unconstrained direction and build its inverse on demand: an
        # `_InverseTransform` is tied to its parent through a weak reference that deepcopy / pickling breaks
        tt = torch.distributions.transforms.identity_transform if theta_transform is None else theta_transform
        self._to_constrained = tt.inv
        self.method = method
        self.thin = _process_thin_default(thin)
        self.warmup_steps = warmup_steps
        self.num_chains = num_chains
        self.init_strategy = init_strategy
        self.init_strategy_parameters = init_strategy_parameters or {}
        self.num_workers = num_workers
        self.mp_context = mp_context
        self._posterior_sampler = None
        self._mcmc_init_params: Optional[Tensor] = None
        self._x: Optional[Tensor] = None
        self._x_shape = x_shape
        # batched sampling on a ratio potential: True / False picks the persistent one-lane-per-chain kernel or the
        # two-launch tick; None leaves it to the sampler's default (samplers/mcmc/slice_vectorized.py)
        self.batched_persistent: Optional[bool] = None
        self._purpose = "It provides MCMC to .sample() from the posterior and can evaluate the _unnormalized_ " \
                        "posterior density with .log_prob()."

    @property
    def theta_transform(self):
        """constrained -> unconstrained (what `mcmc_transform` returns)."""
        # `.inv` of a plain transform builds its `_InverseTransform`; `.inv` of an `_InverseTransform` hands back the
        # parent it wraps -- either way the transform the caller passed in (wrapping unconditionally double-inverted a
        # plain transform and raised NotImplementedError in .sample())
        return self._to_constrained.inv

    # -- x handling (base_posterior.py:170-214) ------------------------------------------
    @property
    def default_x(self) -> Optional[Tensor]:
        return self._x

    def set_default_x(self, x: Tensor) -> "MCMCPosterior":
        x = torch.as_tensor(x, dtype=torch.float32)
        if not torch.isfinite(x).all():
            raise ValueError("x_o contains NaN or Inf values.")
        self._x = x.to(self._device)
        return self

    def _x_else_default_x(self, x: Optional[Tensor]) -> Tensor:
        if x is not None:
            return torch.as_tensor(x, dtype=torch.float32).to(self._device)
        if self._x is None:
            raise ValueError("Context `x` needed when a default has not been set. If you'd like to have a default, "
                             "use the `.set_default_x()` method.")
        return self._x

    @property
    def mcmc_method(self) -> str:
        return self.method

    def set_mcmc_method(self, method: str) -> "MCMCPosterior":
        self.method = method
        return self

    @property
    def posterior_sampler(self):
        return self._posterior_sampler

    # -- density --------------------------------------------------------------------------
    def log_prob(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False) -> Tensor:
        """The potential: the UNNORMALISED posterior log-density (mcmc_posterior.py:208-235)."""
        import warnings

        warnings.warn("`.log_prob()` is deprecated for methods that can only evaluate the log-probability up to a "
                      "normalizing constant. Use `.potential()` instead.", stacklevel=2)
        return self.potential(theta, x, track_gradients)

    def potential(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False) -> Tensor:
        self.potential_fn.set_x(self._x_else_default_x(x))
        theta = ensure_theta_batched(torch.as_tensor(theta)).to(self._device)
        return self.potential_fn(theta, track_gradients=track_gradients)

    # -- sampling -------------------------------------------------------------------------
    def sample(self, sample_shape=torch.Size(), x: Optional[Tensor] = None, method: Optional[str] = None,
               thin: Optional[int] = None, warmup_steps: Optional[int] = None, num_chains: Optional[int] = None,
               init_strategy: Optional[str] = None, init_strategy_parameters: Optional[Dict[str, Any]] = None,
               num_workers: Optional[int] = None, mp_context: Optional[str] = None,
               show_progress_bars: bool = True, **kwargs) -> Tensor:
        x = self._x_else_default_x(x)
        self.potential_fn.set_x(x, x_is_iid=True)
        method = self.method if method is None else method
        thin = self.thin if thin is None else _process_thin_default(thin)
        warmup_steps = self.warmup_steps if warmup_steps is None else warmup_steps
        num_chains = self.num_chains if num_chains is None else num_chains
        init_strategy = self.init_strategy if init_strategy is None else init_strategy
        init_strategy_parameters = (self.init_strategy_parameters if init_strategy_parameters is None
                                    else init_strategy_parameters)
        if method in _OTHER_METHODS:
            raise NotImplementedError(f"method={method!r}: the Pyro / PyMC samplers are outside the accelerated "
                                      "path; use 'slice_np_vectorized'.")
        if method not in _SLICE_METHODS:
            raise NameError(f"The sampling method {method} is not implemented!")

        potential_ = unconstrained_potential(self.potential_fn, self.theta_transform, self._device)

        fused = self._fused_potential()
        if fused is not None:
            potential_ = fused
        self.potential_ = potential_
        initial_params = self._get_initial_params(init_strategy, num_chains, **init_strategy_parameters)
        num_samples = torch.Size(sample_shape).numel()
        with torch.no_grad():
            transformed = self._slice_np_mcmc(num_samples, potential_, initial_params, thin, warmup_steps)
        samples = self.theta_transform.inv(transformed)
        return samples.reshape((*torch.Size(sample_shape), -1))

    def sample_batched(self, sample_shape, x: Tensor, method: Optional[str] = None, thin: Optional[int] = None,
                       warmup_steps: Optional[int] = None, num_chains: Optional[int] = None,
                       init_strategy: Optional[str] = None, init_strategy_parameters: Optional[Dict[str, Any]] = None,
                       num_workers: Optional[int] = None, mp_context: Optional[str] = None,
                       show_progress_bars: bool = True) -> Tensor:
        """Samples of p(theta | x_b) for every row of `x`, shape (*sample_shape, B, D) (mcmc_posterior.py:369-515):
        `num_chains` chains PER observation, laid out AAABBBCCC, every tick of all B x num_chains chains one kernel pass
        over (theta, x) pairs.  Chains of different observations are never pooled.  Tick routes, first match: the
        persistent one-lane-per-chain kernel (ratio potential with a box prior), the fused two-launch
        tick (NSF posterior / NSF likelihood / ratio potentials), the generic loop on `potential_fn` with
        `set_x(x_repeated, x_is_iid=False)`."""
        import warnings

        method = self.method if method is None else method
        thin = self.thin if thin is None else _process_thin_default(thin)
        warmup_steps = self.warmup_steps if warmup_steps is None else warmup_steps
        num_chains = self.num_chains if num_chains is None else num_chains
        init_strategy = self.init_strategy if init_strategy is None else init_strategy
        init_strategy_parameters = dict(self.init_strategy_parameters if init_strategy_parameters is None
                                        else init_strategy_parameters)
        # (an AssertionError, as upstream: get_posterior_samples_on_batch catches it to fall back to a loop)
        assert method in _SLICE_METHODS, "Batched sampling only supported for vectorized samplers!"
        num_per_x = torch.Size(sample_shape).numel()
        if num_chains > num_per_x:
            warnings.warn("The passed number of MCMC chains is larger than the number of requested samples: "
                          f"{num_chains} > {num_per_x}, resetting it to {num_per_x}.", stacklevel=2)
            num_chains = num_per_x
        x = torch.as_tensor(x, dtype=torch.float32).to(self._device)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        batch_size = x.shape[0]
        if batch_size == 0 or num_per_x == 0:
            raise ValueError("sample_batched needs at least one observation and one sample per observation.")
        initial_params = self._get_initial_params_batched(x, init_strategy, num_chains, **init_strategy_parameters)
        # ABC -> AAABBBCCC: chain c belongs to observation c // num_chains
        x_repeated = x.repeat_interleave(num_chains, dim=0)
        self.potential_fn.set_x(x_repeated, x_is_iid=False)
        potential_ = self._fused_potential_batched(x, num_chains)
        if potential_ is None:
            potential_ = unconstrained_potential(self.potential_fn, self.theta_transform, self._device)
        self.potential_ = potential_
        with torch.no_grad():
            transformed = self._slice_np_mcmc_batched(num_per_x, num_chains, potential_, initial_params, thin, warmup_steps)
        per_chain = self.theta_transform.inv(transformed.reshape(-1, transformed.shape[-1]))
        dim_theta = per_chain.shape[-1]
        # (B * K, n, D) -> (B, K * n, D) -> (K * n, B, D): the draws of one observation stay together
        per_x = per_chain.reshape(batch_size, -1, dim_theta).permute(1, 0, 2)
        return per_x[:num_per_x].reshape((*torch.Size(sample_shape), batch_size, dim_theta))

    def _slice_np_mcmc_batched(self, num_per_x: int, chains_per_x: int, potential_function: Callable, initial_params: Tensor, thin: int,
                               warmup_steps: int, init_width: float = 0.01) -> Tensor:
        """(chains, kept sweeps, D) of all B x K chains, warm-up removed (`interchangeable_chains=False` upstream):
        every chain keeps ceil(num_per_x * thin / K) sweeps, thinned."""
        num_chains_total, dim_samples = initial_params.shape
        sampler = SliceSamplerVectorized(init_params=initial_params, log_prob_fn=potential_function,
                                         num_chains=num_chains_total, thin=thin, verbose=False, init_width=init_width,
                                         persistent=self.batched_persistent)
        warmup_ = warmup_steps * thin
        num_samples_ = ceil((num_per_x * thin) / chains_per_x)
        samples = sampler.run(warmup_ + num_samples_)
        samples = samples[:, warmup_steps:, :]
        self._posterior_sampler = sampler
        self._mcmc_init_params = samples[:, -1, :].reshape(num_chains_total, dim_samples)
        return samples.to(torch.float32).to(self._device)

    def _get_initial_params_batched(self, x: Tensor, init_strategy: str, num_chains_per_x: int, **kwargs) -> Tensor:
        """(B * K, D) initial parameters, K per observation (mcmc_posterior.py:661-740).  `sir` / `resample` weigh each
        observation's candidates against that observation; the candidates of several observations go through the
        potential in ONE paired call (`x_is_iid=False`), grouped so that a call has at most INIT_ROWS_PER_CALL rows."""
        import copy

        from sbi_amd.samplers.mcmc.init_strategy import _pick

        B, K = x.shape[0], int(num_chains_per_x)
        kwargs.pop("num_return_samples", None)
        if init_strategy == "proposal":
            init = proposal_init(self.proposal, transform=self.theta_transform, num_chains=B * K)
        elif init_strategy in ("sir", "resample"):
            per_chain = int(kwargs.get("num_candidate_samples", 10_000))
            if init_strategy == "resample":
                per_chain *= int(kwargs.get("num_batches", 1))
            pot = copy.copy(self.potential_fn)           # its own x_o; the estimator is shared, not copied
            obs_per_call = max(1, INIT_ROWS_PER_CALL // max(K * per_chain, 1))
            picked = []
            with torch.no_grad():
                for b0 in range(0, B, obs_per_call):
                    xb = x[b0 : b0 + obs_per_call]
                    nb = xb.shape[0]
                    cand = self.proposal.sample((nb * K * per_chain,)).detach()
                    pot.set_x(xb.repeat_interleave(K * per_chain, dim=0), x_is_iid=False)
                    log_w = pot(cand.to(self._device), track_gradients=False).detach().reshape(-1)
                    if init_strategy == "sir":
                        log_w = log_w - self.proposal.log_prob(cand).detach().reshape(-1).to(log_w.device)
                    picked.append(_pick(cand.to(log_w.device), log_w, nb * K, per_chain))
            init = self.theta_transform(torch.cat(picked))
        elif init_strategy == "latest_sample":
            stored = self._mcmc_init_params
            if stored is None:
                raise ValueError("`init_strategy='latest_sample'` continues the chains of an earlier `sample()` or "
                                 "`sample_batched()` call, but this posterior holds no chain states. Use another init "
                                 "strategy, for example 'proposal' or 'sir'.")
            if B * K > stored.shape[0]:
                raise ValueError(f"`init_strategy='latest_sample'` has {stored.shape[0]} chain state(s) from the last "
                                 f"run, but this call needs {B * K}. Run at most {stored.shape[0]} chain(s), or use "
                                 "another init strategy.")
            init = stored[: B * K]
        else:
            raise NotImplementedError(f"Init strategy {init_strategy} is not implemented.")
        init = init.reshape(B * K, -1).to(self._device)
        assert init.shape[0] == B * K, "Initial params shape mismatch."
        return init

    def _fused_potential_batched(self, x: Tensor, num_chains: int) -> Optional[Callable]:
        """The two-launch tick of `_fused_potential` with one observation PER CHAIN: theta = T^-1(u) and log|det| from
        `sbi_amd_mcmc_to_constrained`, then the paired log-density kernel (x_rows == number of chains) on the repeated
        observations, which are materialised once, here.  NPE on an NSF: log q(theta_c | x_c).  NLE on an NSF: the flow's
        input is the chain's observation and its condition is theta, plus log p(theta).  NRE: log r(theta_c, x_c) plus
        log p(theta); with a box prior its spec also carries what sbi_amd_nre_mcmc_slice_run needs.  None when anything
        does not match (the generic route is always correct)."""
        from sbi_amd import _lib
        from sbi_amd.inference.potentials.likelihood_based_potential import LikelihoodBasedPotential
        from sbi_amd.inference.potentials.posterior_based_potential import PosteriorBasedPotential
        from sbi_amd.inference.potentials.ratio_based_potential import RatioBasedPotential
        from sbi_amd.neural_nets.estimators.nsf_flow import NSFFlow, NSFNet
        from sbi_amd.neural_nets.estimators.ratio_estimator import RatioEstimator, _kernel_log_ratio

        pot = self.potential_fn
        dev = torch.device(self._device)
        if dev.type != "cuda":
            return None
        B, K = x.shape[0], int(num_chains)
        n = B * K
        nre = None
        if isinstance(pot, PosteriorBasedPotential) and isinstance(pot.posterior_estimator, NSFFlow):
            est = pot.posterior_estimator
            D = est.input_shape[0]
            with torch.no_grad():
                emb = est._embed(reshape_to_batch_event(x, est.condition_shape).to(dev)).reshape(B, -1).to(torch.float32)
            if emb.shape[1] != est.net.hyper.C:
                return None
            x_rows = emb.repeat_interleave(K, dim=0).contiguous()

            def log_q(theta: Tensor) -> Tensor:
                return est._kernel_log_prob(theta, x_rows, False)[0]
        elif isinstance(pot, LikelihoodBasedPotential):
            est = pot.likelihood_estimator
            if not isinstance(est, NSFFlow) or type(est)._raw_log_prob is not NSFFlow._raw_log_prob:
                return None
            if not isinstance(est.net, NSFNet) or est._embedding_net is not None:
                return None
            D = int(est.condition_shape[0])
            x_rows = x.reshape(B, -1).to(dev, torch.float32).repeat_interleave(K, dim=0).contiguous()
            if x_rows.shape[1] != est.input_shape[0]:
                return None
            prior = pot.prior

            def log_q(theta: Tensor) -> Tensor:      # the observation is the flow's input, theta its condition
                return est._kernel_log_prob(x_rows, theta, False)[0] + prior.log_prob(theta)
        elif isinstance(pot, RatioBasedPotential) and isinstance(pot.ratio_estimator, RatioEstimator):
            est = pot.ratio_estimator
            h = est.net.hyper
            D = h.D
            if x[0].numel() != h.C:
                return None
            x_obs = x.reshape(B, h.C).to(dev, torch.float32).contiguous()
            x_rows = x_obs.repeat_interleave(K, dim=0).contiguous()
            prior = pot.prior

            def log_q(theta: Tensor) -> Tensor:
                return _kernel_log_ratio(est.net, theta, x_rows, n, dev) + prior.log_prob(theta)

            nre = dict(net=est.net, x=x_obs, num_x=B, chains_per_x=K, low=None, high=None, prior_log_prob=0.0)
        else:
            return None
        spec = self._constrained_map(pot.prior, D)
        if spec is None:
            return None
        kind, p0, p1 = spec
        lib = _lib.load()
        if nre is not None and kind == 2:
            # a box prior: one constant inside the support, asked of the prior itself at the centre of the box
            support = pot.prior.support
            base_c = support.base_constraint if hasattr(support, "base_constraint") else support
            low = torch.as_tensor(base_c.lower_bound, dtype=torch.float32, device=dev).expand(D).contiguous()
            high = torch.as_tensor(base_c.upper_bound, dtype=torch.float32, device=dev).expand(D).contiguous()
            centre = (0.5 * (low + high)).reshape(1, D)
            nre.update(low=low, high=high, prior_log_prob=float(pot.prior.log_prob(centre).reshape(-1)[0].item()))

        def potential_(u: Tensor):
            u = u.to(torch.float32).contiguous()
            C = u.shape[0]
            theta = torch.empty_like(u)
            lad = torch.empty(C, dtype=torch.float32, device=u.device)
            with torch.cuda.device(u.device):
                rc = lib.sbi_amd_mcmc_to_constrained(kind, C, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u),
                                                     _lib.ptr(theta), _lib.ptr(lad), _lib.current_stream(u.device))
            _lib.check(rc, "mcmc_to_constrained")
            return log_q(theta), lad

        potential_.fused_spec = (kind, p0, p1, log_q, None, None)
        potential_.persistent_capable = False        # sbi_amd_mcmc_slice_run evaluates ONE x_o for all chains
        if nre is not None:
            potential_.nre_persistent = nre
        return potential_

    def __getstate__(self):
        """`potential_` is the closure the last `sample()` call ran its chains on (the reference keeps a picklable
        `partial` there, mcmc_posterior.py:145); it is rebuilt by every `sample()` call, so it is simply not part of
        the pickled state.  The live object is left untouched (tests/save_and_load_test.py:23-45)."""
        state = dict(self.__dict__)
        state["potential_"] = None
        state["_posterior_sampler"] = None      # holds the same closure as its log_prob_fn (diagnostics only)
        return state

    def _fused_potential(self) -> Optional[Callable]:
        """Four launches per tick instead of ~15: when the potential is the NSF estimator's log-prob inside the
        prior support and the parameter transform is one `mcmc_transform` builds (z-scoring of an unbounded
        prior, logit map of a box, identity on an unbounded prior), theta = T^-1(u) and log|det| come from
        `sbi_amd_mcmc_to_constrained`, log q from the batched log_prob kernel, and the subtraction happens inside
        the tick kernel.  Returns None when anything does not match (the generic path is always correct)."""
        from sbi_amd import _lib
        from sbi_amd.inference.potentials.likelihood_based_potential import LikelihoodBasedPotential
        from sbi_amd.inference.potentials.posterior_based_potential import PosteriorBasedPotential
        from sbi_amd.neural_nets.estimators.nsf_flow import NSFFlow

        pot = self.potential_fn
        if torch.device(self._device).type != "cuda":
            return None
        if isinstance(pot, LikelihoodBasedPotential):
            return self._fused_likelihood_potential(pot)
        from sbi_amd.inference.potentials.ratio_based_potential import RatioBasedPotential

        if isinstance(pot, RatioBasedPotential):
            return self._fused_ratio_potential(pot)
        if not isinstance(pot, PosteriorBasedPotential) or not isinstance(pot.posterior_estimator, NSFFlow):
            return None
        x_o = reshape_to_batch_event(pot.x_o, pot.posterior_estimator.condition_shape)
        if x_o.shape[0] != 1:
            return None
        D = pot.posterior_estimator.input_shape[0]
        spec = self._constrained_map(pot.prior, D)
        if spec is None:
            return None
        kind, p0, p1 = spec
        dev = torch.device(self._device)
        lib = _lib.load()
        net = pot.posterior_estimator.net
        # the kernels take the EMBEDDED condition (standardizing_net -> embedding_net in front of the flow,
        # flow.py:1395-1416): embed x_o once, outside the chain loop -- never hand raw x to the kernel
        est = pot.posterior_estimator
        with torch.no_grad():
            x_row = est._embed(x_o.to(dev)).reshape(1, -1).to(torch.float32).contiguous()
        if x_row.shape[1] != net.hyper.C:
            return None

        def potential_(u: Tensor):
            u = u.to(torch.float32).contiguous()
            C = u.shape[0]
            theta = torch.empty_like(u)
            lad = torch.empty(C, dtype=torch.float32, device=u.device)
            with torch.cuda.device(u.device):
                rc = lib.sbi_amd_mcmc_to_constrained(kind, C, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u),
                                                     _lib.ptr(theta), _lib.ptr(lad), _lib.current_stream(u.device))
            _lib.check(rc, "mcmc_to_constrained")
            logp, _ = est._kernel_log_prob(theta, x_row, False)
            return logp, lad

        def log_q(theta: Tensor) -> Tensor:      # the estimator's log-density at constrained points, one launch
            return est._kernel_log_prob(theta, x_row, False)[0]

        # the slice sampler's tick kernel applies the transform itself (sbi_amd_mcmc_slice_tick): two launches per tick
        potential_.fused_spec = (kind, p0, p1, log_q, net, x_row)
        # the persistent sampler (sbi_amd_mcmc_slice_run) evaluates the NSF itself from its packed image: any other
        # family behind the NSFFlow surface (maf_rqs, zuko_nsf, mdn) keeps the two-launch tick on its own log_q
        from sbi_amd.neural_nets.estimators.nsf_flow import NSFNet

        if not isinstance(net, NSFNet):
            potential_.persistent_capable = False
        return potential_

    def _fused_likelihood_potential(self, pot) -> Optional[Callable]:
        """NLE's potential in the same tick structure: theta = T^-1(u) and log|det| from `sbi_amd_mcmc_to_constrained`,
        sum_i log q(x_i | theta) from the trials kernel (sbi_amd_nsf_log_prob_trials) plus log p(theta), the subtraction
        inside the tick kernel.  The persistent sampler (sbi_amd_mcmc_slice_run) evaluates NPE's density with x_o as
        the condition, so the spec is marked for the two-launch loop.  None when anything does not match."""
        from sbi_amd import _lib
        from sbi_amd.neural_nets.estimators.nsf_flow import NSFFlow, NSFNet

        est = pot.likelihood_estimator
        if not isinstance(est, NSFFlow) or type(est)._raw_log_prob is not NSFFlow._raw_log_prob:
            return None
        if not isinstance(est.net, NSFNet) or est._embedding_net is not None or not pot.x_is_iid:
            return None
        dev = torch.device(self._device)
        x_trials = pot.x_o.reshape(-1, est.input_shape[0]).to(dev, torch.float32).contiguous()
        lib = _lib.load()
        if lib.sbi_amd_nsf_log_prob_trials_workspace_floats(est.net.hyper.c_config(), x_trials.shape[0], 1) < 0:
            return None                                  # (hidden 65 - 128: no trials kernel)
        D = int(est.condition_shape[0])
        spec = self._constrained_map(pot.prior, D)
        if spec is None:
            return None
        kind, p0, p1 = spec
        prior = pot.prior

        def log_q(theta: Tensor) -> Tensor:      # sum over the trials (one pass, no pairs) + log prior
            ll = est.log_prob_iid_trials(x_trials, theta)
            if ll is None:
                raise RuntimeError("sbi_amd: the trials kernel refused a configuration it accepted before")
            return ll + prior.log_prob(theta)

        def potential_(u: Tensor):
            u = u.to(torch.float32).contiguous()
            C = u.shape[0]
            theta = torch.empty_like(u)
            lad = torch.empty(C, dtype=torch.float32, device=u.device)
            with torch.cuda.device(u.device):
                rc = lib.sbi_amd_mcmc_to_constrained(kind, C, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u),
                                                     _lib.ptr(theta), _lib.ptr(lad), _lib.current_stream(u.device))
            _lib.check(rc, "mcmc_to_constrained")
            return log_q(theta), lad

        potential_.fused_spec = (kind, p0, p1, log_q, None, None)
        potential_.persistent_capable = False
        return potential_

    def _fused_ratio_potential(self, pot) -> Optional[Callable]:
        """NRE's potential in the same two-launch tick structure as NLE's: theta = T^-1(u) and log|det| from
        `sbi_amd_mcmc_to_constrained`, sum_i log r(theta, x_i) from the trials kernel (sbi_amd_nre_log_ratio_trials)
        plus log p(theta), the subtraction inside the tick kernel.  None when anything does not match."""
        from sbi_amd import _lib
        from sbi_amd.neural_nets.estimators.ratio_estimator import RatioEstimator

        est = pot.ratio_estimator
        if not isinstance(est, RatioEstimator) or not pot.x_is_iid:
            return None
        dev = torch.device(self._device)
        h = est.net.hyper
        x_trials = pot.x_o.reshape(-1, h.C).to(dev, torch.float32).contiguous()
        D = h.D
        spec = self._constrained_map(pot.prior, D)
        if spec is None:
            return None
        kind, p0, p1 = spec
        lib = _lib.load()
        prior = pot.prior

        def log_q(theta: Tensor) -> Tensor:      # sum over the trials (one pass, no pairs) + log prior
            return est.log_ratio_iid_trials(x_trials, theta) + prior.log_prob(theta)

        def potential_(u: Tensor):
            u = u.to(torch.float32).contiguous()
            C = u.shape[0]
            theta = torch.empty_like(u)
            lad = torch.empty(C, dtype=torch.float32, device=u.device)
            with torch.cuda.device(u.device):
                rc = lib.sbi_amd_mcmc_to_constrained(kind, C, D, _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(u),
                                                     _lib.ptr(theta), _lib.ptr(lad), _lib.current_stream(u.device))
            _lib.check(rc, "mcmc_to_constrained")
            return log_q(theta), lad

        potential_.fused_spec = (kind, p0, p1, log_q, None, None)
        potential_.persistent_capable = False
        return potential_

    def _constrained_map(self, prior, D: int):
        """(kind, p0, p1) of `sbi_amd_mcmc_to_constrained` for the parameter transform, or None: z-scoring of an
        unbounded prior, logit map of a box, identity on an unbounded prior."""
        import torch.distributions.transforms as tf
        from torch.distributions import constraints

        try:
            support = prior.support
        except (NotImplementedError, AttributeError):
            return None
        base_c = support.base_constraint if hasattr(support, "base_constraint") else support
        t = self._to_constrained                         # unconstrained -> constrained
        if isinstance(t, tf.IndependentTransform):
            t = t.base_transform
        dev = torch.device(self._device)

        def vec(v):
            return torch.as_tensor(v, dtype=torch.float32, device=dev).expand(D).contiguous()

        unbounded = isinstance(base_c, constraints._Real)
        if isinstance(t, tf.ComposeTransform) and len(t.parts) == 0 and unbounded:
            kind, p0, p1 = 0, None, None
        elif isinstance(t, tf.AffineTransform) and unbounded:
            kind, p0, p1 = 1, vec(t.loc), vec(t.scale)
        elif (isinstance(t, tf.ComposeTransform) and len(t.parts) == 2 and isinstance(t.parts[0], tf.SigmoidTransform)
              and isinstance(t.parts[1], tf.AffineTransform) and isinstance(base_c, constraints._Interval)):
            low, high = vec(base_c.lower_bound), vec(base_c.upper_bound)
            p0, p1 = vec(t.parts[1].loc), vec(t.parts[1].scale)
            if not (torch.allclose(p0, low) and torch.allclose(p0 + p1, high)):
                return None                              # the box of the transform is not the prior's support
            kind = 2
        else:
            return None
        return kind, p0, p1

    def _get_initial_params(self, init_strategy: str, num_chains: int, **kwargs) -> Tensor:
        """mcmc_posterior.py:517-659, all chains in one batched call."""
        from sbi_amd.inference.potentials.likelihood_based_potential import LikelihoodBasedPotential

        potential_fn = self.potential_fn
        from sbi_amd.inference.potentials.ratio_based_potential import RatioBasedPotential

        if isinstance(potential_fn, (LikelihoodBasedPotential, RatioBasedPotential)):
            # the init weights are detached: evaluate NLE's candidates (10 000 x num_trials pairs) with the trials kernel
            def potential_fn(theta, _pot=self.potential_fn):
                return _pot(theta, track_gradients=False)
        if init_strategy == "proposal":
            init = proposal_init(self.proposal, transform=self.theta_transform, num_chains=num_chains, **kwargs)
        elif init_strategy == "sir":
            init = sir_init(self.proposal, potential_fn, transform=self.theta_transform, num_chains=num_chains,
                            **kwargs)
        elif init_strategy == "resample":
            init = resample_given_potential_fn(self.proposal, potential_fn, transform=self.theta_transform,
                                               num_chains=num_chains, **kwargs)
        elif init_strategy == "latest_sample":
            stored = self._mcmc_init_params
            if stored is None:
                raise ValueError("`init_strategy='latest_sample'` continues the chains of an earlier `sample()` call, "
                                 "but this posterior holds no chain states. Use another init strategy, for example "
                                 "'proposal' or 'sir'.")
            if num_chains > stored.shape[0]:
                raise ValueError(f"`init_strategy='latest_sample'` has {stored.shape[0]} chain state(s) from the last "
                                 f"run, but this call needs {num_chains}. Run at most {stored.shape[0]} chain(s), or "
                                 "use another init strategy.")
            init = stored[:num_chains]
        else:
            raise NotImplementedError(f"Init strategy {init_strategy} is not implemented.")
        init = init.reshape(num_chains, -1).to(self._device)
        assert init.shape[0] == num_chains, "Initial params shape mismatch."
        return init

    def _slice_np_mcmc(self, num_samples: int, potential_function: Callable, initial_params: Tensor, thin: int,
                       warmup_steps: int, init_width: float = 0.01) -> Tensor:
        """mcmc_posterior.py:737-811."""
        num_chains, dim_samples = initial_params.shape
        sampler = SliceSamplerVectorized(init_params=initial_params, log_prob_fn=potential_function,
                                         num_chains=num_chains, thin=thin, verbose=False, init_width=init_width)
        warmup_ = warmup_steps * thin
        num_samples_ = ceil((num_samples * thin) / num_chains)
        samples = sampler.run(warmup_ + num_samples_)            # chains x samples x dim (already thinned)
        samples = samples[:, warmup_steps:, :]                   # discard warmup steps
        self._posterior_sampler = sampler
        self._mcmc_init_params = samples[:, -1, :].reshape(num_chains, dim_samples)
        samples = samples.reshape(-1, dim_samples)[:num_samples]  # chains are interchangeable
        return samples.to(torch.float32).to(self._device)
