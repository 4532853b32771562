"""The variational families of ``VIPosterior`` (sbi/samplers/vi/vi_utils.py).

``LearnableGaussian`` keeps sbi's parameters and ``state_dict`` keys (``loc`` and ``scale_tril``, read through
``.tril()``, or ``log_scale``).  On a ROCm device its ``sample`` and, without autograd, its ``log_prob`` /
``sample_and_log_prob`` are one launch of ``sbi_amd_vi_gauss_draw`` / ``sbi_amd_vi_gauss_log_prob``
(include/sbi_amd_vi.h) whenever the link transform decomposes per dimension (``link_descriptor``); everything else,
and everything under autograd, is the written formula in torch.  ``AdaptedVariationalDistribution`` and the checks
that ``set_q`` runs on a user distribution follow the reference.
"""

from __future__ import annotations

import inspect
from copy import deepcopy
from typing import Callable, Dict, Iterable, Optional, Tuple, Union

import torch
from torch import Tensor, nn
from torch.distributions import Distribution, Independent, MultivariateNormal, Normal, TransformedDistribution
from torch.distributions.transforms import (AffineTransform, CatTransform, ComposeTransform, ExpTransform,
                                            IndependentTransform, SigmoidTransform)
from torch.nn import Module

MAX_KERNEL_DIM = 16                # SBI_AMD_VI_MAX_D
MAX_KERNEL_PARTICLES = 65_536      # SBI_AMD_VI_MAX_PARTICLES
LINK_AFFINE, LINK_INTERVAL, LINK_LOWER, LINK_UPPER = 0.0, 1.0, 2.0, 3.0


class _Unrecognised(Exception):
    pass


def _vec(v, D: int) -> Tensor:
    t = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
    if t.dim() > 1 or (t.dim() == 1 and t.shape[0] not in (1, D)):
        raise _Unrecognised(f"a transform parameter of shape {tuple(t.shape)} does not act per dimension")
    return t.reshape(-1).expand(D).clone()


def _flatten(transform) -> list:
    if isinstance(transform, IndependentTransform):
        return _flatten(transform.base_transform)
    if isinstance(transform, ComposeTransform):
        return [p for part in transform.parts for p in _flatten(part)]
    return [transform]


def _describe(transform, D: int) -> Tensor:
    """(4, D) fp64 rows [kind | a | b | c] of one transform acting on D dimensions."""
    if isinstance(transform, CatTransform):
        if transform.dim not in (-1, 0) or sum(transform.lengths) != D:
            raise _Unrecognised("a CatTransform that does not split the last dimension")
        return torch.cat([_describe(t, n) for t, n in zip(transform.transforms, transform.lengths)], dim=1)
    parts = _flatten(transform)
    for p in parts:
        if isinstance(p, CatTransform):
            raise _Unrecognised("a CatTransform inside a composition")
    head = None
    if parts and isinstance(parts[0], (SigmoidTransform, ExpTransform)):
        head, parts = parts[0], parts[1:]
    loc, scale = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    for p in parts:
        if type(p) is not AffineTransform:
            raise _Unrecognised(f"{type(p).__name__} is not one of the affine / interval / half-bounded link kinds")
        loc, scale = _vec(p.loc, D) + _vec(p.scale, D) * loc, _vec(p.scale, D) * scale
    zeros = torch.zeros(D, dtype=torch.float64)
    if head is None:
        if bool((scale == 0).any()):
            raise _Unrecognised("an affine link with scale 0")
        return torch.stack([zeros + LINK_AFFINE, loc, scale, zeros])
    if isinstance(head, SigmoidTransform):
        if bool((scale <= 0).any()):
            raise _Unrecognised("an interval link with a non-positive width")
        return torch.stack([zeros + LINK_INTERVAL, loc, scale, loc + scale])
    if bool((scale.abs() != 1).any()):
        raise _Unrecognised("a half-bounded link with a scale other than +-1")
    kind = torch.where(scale > 0, zeros + LINK_LOWER, zeros + LINK_UPPER)
    return torch.stack([kind, loc, scale, zeros])


def link_descriptor(link_transform, dim: int) -> Tuple[Optional[Tensor], str]:
    """The per-dimension link table of include/sbi_amd_vi.h, read off the transform objects: ((4, D) fp32 host tensor,
    "") or (None, reason).  Recognised: None / the identity, ``AffineTransform``, ``SigmoidTransform`` then affine (what
    ``biject_to`` gives for an interval), ``ExpTransform`` then an affine of scale +-1 (half-bounded supports), their
    ``IndependentTransform`` / ``ComposeTransform`` wrappers, and a ``CatTransform`` of those along the last dimension."""
    try:
        if link_transform is None:
            table = _describe(ComposeTransform([]), dim)
        else:
            table = _describe(link_transform, dim)
    except _Unrecognised as e:
        return None, f"the link transform does not decompose per dimension into the kernel's kinds ({e})"
    return table.to(torch.float32), ""


def _sum_rightmost(log_det: Tensor, like: Tensor) -> Tensor:
    return log_det.sum(dim=-1) if log_det.dim() > like.dim() else log_det


class LearnableGaussian(nn.Module):
    """q(theta) = T#N(loc, L L^T): full covariance (``scale_tril``, only its lower triangle is read) or diagonal
    (``log_scale``); T = ``link_transform`` maps unconstrained to constrained space (None: the identity)."""

    def __init__(self, dim: int, full_covariance: bool = True, link_transform=None,
                 device: Union[str, torch.device] = "cpu"):
        super().__init__()
        self._dim = int(dim)
        self._full_cov = bool(full_covariance)
        self._link_transform = link_transform
        self.force_eager = False
        self.loc = nn.Parameter(torch.zeros(dim, device=device))
        if full_covariance:
            self.scale_tril = nn.Parameter(torch.eye(dim, device=device))
        else:
            self.log_scale = nn.Parameter(torch.zeros(dim, device=device))

    # -- the kernel route -------------------------------------------------------------------------------------
    def flat_parameters(self) -> Tensor:
        """phi = [loc | scale_tril row-major] or [loc | log_scale] as one detached fp32 vector (a copy)."""
        second = self.scale_tril if self._full_cov else self.log_scale
        return torch.cat([self.loc.detach().reshape(-1), second.detach().reshape(-1)]).contiguous()

    def load_flat_parameters(self, phi: Tensor) -> None:
        D = self._dim
        with torch.no_grad():
            self.loc.copy_(phi[:D])
            if self._full_cov:
                self.scale_tril.copy_(phi[D:].reshape(D, D))
            else:
                self.log_scale.copy_(phi[D:])

    def link_table(self) -> Tuple[Optional[Tensor], str]:
        """The (4, D) table on the parameters' device (cached per transform object and device)."""
        key = (id(self._link_transform), str(self.loc.device))
        cached = self.__dict__.get("_link_cache")
        if cached is None or cached[0] != key:
            table, reason = link_descriptor(self._link_transform, self._dim)
            if table is not None and self.loc.is_cuda:
                table = table.to(self.loc.device).contiguous()
            self.__dict__["_link_cache"] = cached = (key, table, reason)
        return cached[1], cached[2]

    def kernel_route(self) -> Tuple[bool, str]:
        if self.force_eager:
            return False, "force_eager is set"
        if not self.loc.is_cuda:
            return False, f"the parameters live on {self.loc.device}: the kernels run on a ROCm device"
        if any(p.dtype != torch.float32 for p in self.parameters()):
            return False, "the parameters are not float32"
        if self._dim > MAX_KERNEL_DIM:
            return False, f"dim {self._dim} > {MAX_KERNEL_DIM}"
        table, reason = self.link_table()
        if table is None:
            return False, reason
        return True, ""

    def _kernel_draw(self, n: int, want_eps: bool = False, seed: Optional[int] = None, step: int = 0,
                     row_offset: int = 0, phi: Optional[Tensor] = None):
        from sbi_amd import _lib

        lib = _lib.load()
        table, _ = self.link_table()
        phi = self.flat_parameters() if phi is None else phi
        dev = phi.device
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())      # torch.manual_seed fixes a run
        theta = torch.empty((n, self._dim), dtype=torch.float32, device=dev)
        log_q = torch.empty((n,), dtype=torch.float32, device=dev)
        eps = torch.empty((n, self._dim), dtype=torch.float32, device=dev) if want_eps else None
        with torch.cuda.device(dev):
            _lib.check(lib.sbi_amd_vi_gauss_draw(self._dim, int(self._full_cov), _lib.ptr(phi), _lib.ptr(table), n, seed,
                                                 step, row_offset, _lib.ptr(theta), _lib.ptr(log_q), _lib.ptr(eps),
                                                 _lib.current_stream(dev)), "vi_gauss_draw")
        return theta, log_q, eps

    def _kernel_log_prob(self, theta: Tensor) -> Tensor:
        from sbi_amd import _lib

        lib = _lib.load()
        table, _ = self.link_table()
        phi = self.flat_parameters()
        flat = theta.detach().to(phi.device, torch.float32).reshape(-1, self._dim).contiguous()
        out = torch.empty((flat.shape[0],), dtype=torch.float32, device=phi.device)
        with torch.cuda.device(phi.device):
            _lib.check(lib.sbi_amd_vi_gauss_log_prob(self._dim, int(self._full_cov), _lib.ptr(phi), _lib.ptr(table),
                                                     _lib.ptr(flat), flat.shape[0], _lib.ptr(out),
                                                     _lib.current_stream(phi.device)), "vi_gauss_log_prob")
        return out.reshape(theta.shape[:-1])

    # -- the written formulas ---------------------------------------------------------------------------------
    def _cholesky(self) -> Tensor:
        return self.scale_tril.tril()

    def _base_dist(self) -> Distribution:
        # validate_args=False: the parameters are unconstrained; NaN log-probs beat a mid-training exception
        if self._full_cov:
            return MultivariateNormal(self.loc, scale_tril=self._cholesky(), validate_args=False)
        return Independent(Normal(self.loc, self.log_scale.exp(), validate_args=False), 1)

    def sample(self, sample_shape=torch.Size()) -> Tensor:
        shape = torch.Size(sample_shape)
        if self.kernel_route()[0]:
            theta, _, _ = self._kernel_draw(shape.numel())
            return theta.reshape((*shape, self._dim))
        with torch.no_grad():
            samples = self._base_dist().sample(shape)
            if self._link_transform is not None:
                samples = self._link_transform(samples)
        return samples

    def log_prob(self, theta: Tensor) -> Tensor:
        if not torch.is_grad_enabled() and self.kernel_route()[0]:
            return self._kernel_log_prob(theta)
        if self._link_transform is None:
            return self._base_dist().log_prob(theta)
        z = self._link_transform.inv(theta)
        log_prob_z = self._base_dist().log_prob(z)
        return log_prob_z + _sum_rightmost(self._link_transform.inv.log_abs_det_jacobian(theta, z), log_prob_z)

    def sample_and_log_prob(self, sample_shape=torch.Size()) -> Tuple[Tensor, Tensor]:
        shape = torch.Size(sample_shape)
        if not torch.is_grad_enabled() and self.kernel_route()[0]:
            theta, log_q, _ = self._kernel_draw(shape.numel())
            return theta.reshape((*shape, self._dim)), log_q.reshape(shape)
        dist = self._base_dist()
        z = dist.rsample(shape)
        log_prob_z = dist.log_prob(z)
        if self._link_transform is None:
            return z, log_prob_z
        theta = self._link_transform(z)
        return theta, log_prob_z - _sum_rightmost(self._link_transform.log_abs_det_jacobian(z, theta), log_prob_z)

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_link_cache", None)
        return state


def move_distribution(dist, device):
    """`dist` on `device` when it knows how to move (`BoxUniform.to`, a module), else `dist` as it is."""
    mover = getattr(dist, "to", None)
    if dist is None or mover is None:
        return dist
    moved = mover(device)
    return dist if moved is None else moved


def filter_kwargs_for_func(f: Callable, kwargs: Dict) -> Dict:
    """The entries of `kwargs` whose key is a parameter name of `f`."""
    accepted = set(inspect.signature(f).parameters)
    return {key: kwargs[key] for key in kwargs if key in accepted}


def _callable_attribute(q, name: str):
    member = getattr(q, name, None)
    if member is None:
        raise ValueError(f"The variational distribution needs a `{name}()` method that returns an iterable (pass "
                         f"`{name}=` to `set_q` for a distribution that has none).")
    if not callable(member):
        raise AssertionError(f"`{name}` of the variational distribution must be a method, got {type(member).__name__}")
    return member


def check_parameters_modules_attribute(q) -> None:
    """`q.parameters()` must yield tensors, at least one of them trainable; `q.modules()` must yield `nn.Module`s."""
    tensors = list(_callable_attribute(q, "parameters")())
    if not all(isinstance(t, Tensor) for t in tensors):
        raise AssertionError("`parameters()` of the variational distribution must yield tensors only")
    if not any(t.requires_grad for t in tensors):
        raise AssertionError("Nothing to train: none of the variational distribution's parameters requires a gradient")
    if not all(isinstance(m, Module) for m in _callable_attribute(q, "modules")()):
        raise AssertionError("`modules()` of the variational distribution must yield torch modules only")


def check_sample_shape_and_support(q: Distribution, prior: Distribution, num_draws: int = 1000) -> None:
    """q and the prior must describe the same kind of variable: equal event and batch shapes, draws of q inside the
    prior's support (when it publishes one), and finite densities of each at the other's draws."""
    for what in ("event_shape", "batch_shape"):
        if getattr(q, what) != getattr(prior, what):
            raise AssertionError(f"The {what} of q, {tuple(getattr(q, what))}, must match the prior's, "
                                 f"{tuple(getattr(prior, what))}")
    own = q.sample(torch.Size((num_draws,)))
    from_prior = prior.sample(torch.Size((num_draws,))).to(own.device)
    if own.shape != from_prior.shape:
        raise AssertionError(f"q draws {tuple(own.shape)} where the prior draws {tuple(from_prior.shape)}")
    try:
        support = prior.support
    except (NotImplementedError, AttributeError):
        support = None
    if support is not None and not bool(support.check(own).all()):
        raise AssertionError("The support of q must match that of the prior: some draws of q lie outside it")
    if not bool(torch.isfinite(q.log_prob(from_prior)).all()):
        raise AssertionError("q.log_prob is not finite at some prior draws")
    if not bool(torch.isfinite(prior.log_prob(own)).all()):
        raise AssertionError("prior.log_prob is not finite at some draws of q")


def check_variational_distribution(q: Distribution, prior: Distribution) -> None:
    """What `set_q` asks of a user distribution."""
    check_parameters_modules_attribute(q)
    check_sample_shape_and_support(q, prior)


def _transforms_hold_parameters(transforms) -> bool:
    """Whether any transform in the list -- or nested inside a composed / independent one -- exposes `parameters`."""
    pending = list(transforms)
    while pending:
        t = pending.pop()
        if hasattr(t, "parameters"):
            return True
        pending.extend(getattr(t, "parts", None) or [])
        inner = getattr(t, "base_transform", None)
        if inner is not None:
            pending.append(inner)
    return False


class AdaptedVariationalDistribution(Distribution):
    """A user's variational distribution in the shape the divergence optimisers expect.

    * Its support is the prior's: when the two differ, the link transform is appended.
    * `parameters()`, `modules()` and `to()` are methods of THIS class, so the object pickles; the tensors come from
      the `parameters` argument, else from the distribution, else from the base of a `TransformedDistribution`.
    * It deliberately is no `nn.Module` and has no `sample_and_log_prob`: the optimisers take either as the sign of a
      family of their own."""

    arg_constraints: Dict = {}

    def __init__(self, q: Distribution, prior: Distribution, link_transform: Callable,
                 parameters: Optional[Iterable] = None, modules: Optional[Iterable] = None) -> None:
        self._given_parameters = [] if parameters is None else list(parameters)
        self._given_modules = [] if modules is None else list(modules)
        self._owner = self._find_owner(q)
        self._q = self._on_prior_support(q, prior, link_transform)
        super().__init__(batch_shape=self._q.batch_shape, event_shape=self._q.event_shape, validate_args=False)

    def _find_owner(self, q):
        """The object whose `parameters()` is used when none were given."""
        if self._given_parameters or hasattr(q, "parameters"):
            return q
        base = getattr(q, "base_dist", None)
        if not hasattr(base, "parameters"):
            raise ValueError("The variational distribution has no parameters to optimize. Pass the trainable tensors "
                             "as `parameters` (and any modules as `modules`).")
        if _transforms_hold_parameters(getattr(q, "transforms", [])):
            raise ValueError("The variational distribution keeps trainable tensors in its transforms, and only those "
                             "of its base distribution would be found. Pass ALL trainable tensors as `parameters` "
                             "(and any modules as `modules`) so that none is left out of training.")
        return base

    @staticmethod
    def _on_prior_support(q, prior, link_transform):
        if not hasattr(prior, "support") or q.support == prior.support:
            return q
        if isinstance(q, TransformedDistribution):
            return TransformedDistribution(q.base_dist, [*q.transforms, link_transform])
        return TransformedDistribution(q, [link_transform])

    def parameters(self) -> Iterable:
        return iter(self._given_parameters) if self._given_parameters else self._owner.parameters()

    def modules(self) -> Iterable:
        if self._given_modules:
            return iter(self._given_modules)
        lister = getattr(self._owner, "modules", None)
        return lister() if lister is not None else iter(())

    def to(self, device: Union[str, torch.device]) -> None:
        """Moves everything trainable IN PLACE: the optimiser holds the very same tensor objects."""
        for thing in [self._owner, *self._given_modules]:
            if hasattr(thing, "to"):
                thing.to(device)
        for tensor in self.parameters():             # plain tensors have no in-place `to`
            tensor.data = tensor.data.to(device)
            if tensor.grad is not None:
                tensor.grad.data = tensor.grad.data.to(device)

    @property
    def support(self):
        return self._q.support

    @property
    def has_rsample(self) -> bool:
        return self._q.has_rsample

    def sample(self, sample_shape=torch.Size()) -> Tensor:
        return self._q.sample(sample_shape)

    def rsample(self, sample_shape=torch.Size()) -> Tensor:
        return self._q.rsample(sample_shape)

    def log_prob(self, value: Tensor) -> Tensor:
        return self._q.log_prob(value)

    def __repr__(self) -> str:
        return f"AdaptedVariationalDistribution({self._q!r})"


def _detach_non_leaves(obj, seen=None) -> None:
    """Replace every non-leaf tensor that `obj` caches (distribution constructors `expand` their arguments) by a
    detached one: `deepcopy` refuses non-leaf tensors."""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, dict):
        items = obj
    elif hasattr(obj, "__dict__") and not isinstance(obj, (type, Tensor)):
        items = obj.__dict__
    else:
        items = None
    if items is not None:
        for key, val in list(items.items()):
            if isinstance(val, Tensor) and val.requires_grad and not val.is_leaf:
                items[key] = val.detach()
            elif isinstance(val, (list, tuple)):
                for v in val:
                    _detach_non_leaves(v, seen)
            elif isinstance(val, dict) or hasattr(val, "__dict__"):
                _detach_non_leaves(val, seen)


def detach_and_deepcopy(obj):
    """An independent copy of `obj`, non-leaf tensors detached first."""
    with torch.no_grad():
        _detach_non_leaves(obj)
    return deepcopy(obj)
