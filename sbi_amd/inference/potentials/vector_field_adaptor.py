"""Score composition for N iid observations (NPSE) on the fused kernels of csrc/npse_iid_kernel.h.

Host-side mirror of sbi's iid score functions (same class names, constructor arguments and defaults):
  FactorizedNPEScoreFunction ("fnpe"), GaussCorrectedScoreFn ("gauss"), AutoGaussCorrectedScoreFn ("auto_gauss"),
  get_iid_method                 sbi/inference/potentials/vector_field_adaptor.py:33-47, 640-1270, 1357-1410

Under a Gaussian prior (``MultivariateNormal`` or ``Independent(Normal)``) everything those classes compute per call
except the per-observation scores s_i = score(theta, t | x_i) is independent of theta.  ``tables(times, conditions)``
evaluates that part once, in fp64 on the host, as

    score(theta, t) = Linv_t (C_t sum_i s_i + sum_i Lam_i s_i) + A_t theta + b_t

with c = m^2 / s^2, P0 = Sigma0^-1 + c I, M = (m^2 Sigma0 + s^2 I)^-1 and

  gauss family   P_i = c I + Lam_i + corr,  Lam = (1 - N) P0 + sum_i P_i,  Linv = Lam^-1,  C = c I + corr,
                 A = -(1 - N) Linv P0 M,  b = -A (m mu0);  corr is sbi's ``ensure_lam_positive_definite`` correction:
                 V diag(max(-lambda, 0) / (N - 1)) V^T + nugget I from the eigendecomposition of the uncorrected Lam,
                 or its element-wise variant when prior and posterior precisions are all diagonal; zero when off
  fnpe           Linv = C = I, Lam_i = 0, A = -(1 - N) w(t) Sigma0^-1, b = -A mu0, w(t) = (t_max - t) / t_max; under a
                 ``BoxUniform`` prior A = b = 0; the initial draw uses std_base / sqrt(N)

so the ill-conditioned linear algebra (inverses, the eigendecomposition) never runs in fp32 nor inside the sampling
loop; the kernels do N trunk passes and four 16 x 16 mat-vecs per step.  One observation (N = 1) composes to the plain
score: Linv = C = I, Lam = 0, A = b = 0.

Refused with ``NotImplementedError``: ``jac_gauss`` (its precision is a Jacobian of the score network at every theta),
``gauss`` / ``auto_gauss`` under a non-Gaussian prior (the denoised prior precision then depends on theta) and ``fnpe``
under a prior that is neither Gaussian nor ``BoxUniform``.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple, Type

import torch
from torch import Tensor
from torch.distributions import Independent, MultivariateNormal, Normal, Uniform


@dataclass
class IIDTables:
    """fp64 host tables of one time grid: lam (N, D, D) or None (all zero), mats (K, 3, D, D) = Linv, C, A per time,
    vecs (K, D) = b per time, base_scale = factor on std_base of the initial draw."""

    lam: Optional[Tensor]
    mats: Tensor
    vecs: Tensor
    base_scale: float = 1.0

    def on(self, device) -> Tuple[Optional[Tensor], Tensor, Tensor]:
        f = lambda t: None if t is None else t.to(device=device, dtype=torch.float32).contiguous()
        return f(self.lam), f(self.mats), f(self.vecs)


def gaussian_prior_moments(prior) -> Optional[Tuple[Tensor, Tensor, bool]]:
    """(mu0 (D,), Sigma0 (D, D), is_diagonal) in fp64 on the host, or None when the prior is not Gaussian."""
    if isinstance(prior, MultivariateNormal) and len(prior.batch_shape) == 0:
        return prior.loc.detach().double().cpu(), prior.covariance_matrix.detach().double().cpu(), False
    if isinstance(prior, Independent) and isinstance(prior.base_dist, Normal) and prior.reinterpreted_batch_ndims == 1 \
            and len(prior.batch_shape) == 0:
        loc, scale = prior.base_dist.loc.detach().double().cpu(), prior.base_dist.scale.detach().double().cpu()
        return loc.reshape(-1), torch.diag(scale.reshape(-1) ** 2), True
    return None


def _is_box_uniform(prior) -> bool:
    return isinstance(prior, Independent) and isinstance(prior.base_dist, Uniform)


class IIDScoreFunction:
    """Base of the iid score compositions: the estimator must be a score estimator of this package.  ``device`` is kept
    for sbi's signature and recorded; the tables are built on the host and the evaluation follows the device of the
    inputs (which must be a ROCm device: there is no host path)."""

    def __init__(self, vector_field_estimator, prior, device="cpu") -> None:
        if not getattr(vector_field_estimator, "SCORE_DEFINED", False):
            raise ValueError("Score is not defined for this vector field estimator; IID methods require it.")
        if not getattr(vector_field_estimator, "MARGINALS_DEFINED", False):
            raise ValueError("Marginals are not defined for this vector field estimator; IID methods require them.")
        from sbi_amd.neural_nets.estimators.score_estimator import ConditionalScoreEstimator

        if not isinstance(vector_field_estimator, ConditionalScoreEstimator):
            raise NotImplementedError("sbi_amd: iid score composition runs for the score estimators of this package "
                                      "(NPSE); flow-matching estimators are sampled through their ODE, one "
                                      "observation at a time")
        if getattr(vector_field_estimator, "embedding_net", None) is not None:
            raise NotImplementedError("sbi_amd NPSE iid: embedding nets are outside the HIP path (flat x only)")
        self.vector_field_estimator = vector_field_estimator
        self.prior = prior
        self.device = device

    # ------------------------------------------------------------------ tables
    def _ms(self, times: Tensor) -> Tuple[Tensor, Tensor]:
        est = self.vector_field_estimator
        t = torch.as_tensor(times, dtype=torch.float64).detach().cpu().reshape(-1)
        return est.mean_t_fn(t).reshape(-1), est.std_fn(t).reshape(-1)

    def tables(self, times: Tensor, conditions: Tensor) -> IIDTables:
        raise NotImplementedError

    @staticmethod
    def _single(K: int, D: int) -> IIDTables:
        eye = torch.eye(D, dtype=torch.float64)
        mats = torch.stack([eye, eye, torch.zeros_like(eye)]).expand(K, 3, D, D).clone()
        return IIDTables(None, mats, torch.zeros(K, D, dtype=torch.float64))

    # ------------------------------------------------------------------ evaluation
    def __call__(self, inputs: Tensor, conditions: Tensor, time: Optional[Tensor] = None) -> Tensor:
        """inputs (b, 1, D), conditions (N, C), one time -> composed score (b, 1, D) (``score_estimator.score_iid``)."""
        from sbi_amd.neural_nets.estimators.score_estimator import score_iid

        assert inputs.ndim == 3, "Inputs must have shape [b,iid,d]"
        assert conditions.ndim == 2, "Conditions must have shape [iid,...]"
        est = self.vector_field_estimator
        if time is None:
            time = torch.tensor([est.t_min])
        time = torch.as_tensor(time, dtype=torch.float32).reshape(-1)[:1]
        tb = self.tables(time, conditions)
        D = est.input_shape[0]
        th = inputs.to(torch.float32).reshape(-1, D).contiguous()
        lam, mats, vecs = tb.on(th.device)
        xs = conditions.to(device=th.device, dtype=torch.float32).contiguous()
        out = score_iid(est, th, xs, time.to(th.device).contiguous(), lam, mats[0].contiguous(), vecs[0].contiguous())
        return out.reshape(inputs.shape)


class FactorizedNPEScoreFunction(IIDScoreFunction):
    """sum_i s_i + (1 - N) w(t) grad log prior (Geffner et al. 2023; vector_field_adaptor.py:725-813)."""

    def __init__(self, vector_field_estimator, prior, device="cpu",
                 prior_score_weight: Optional[Callable[[Tensor], Tensor]] = None) -> None:
        super().__init__(vector_field_estimator, prior, device)
        if prior_score_weight is None:
            t_max = vector_field_estimator.t_max

            def prior_score_weight(t: Tensor) -> Tensor:
                return (t_max - t) / t_max

        self.prior_score_weight_fn = prior_score_weight
        self._moments = gaussian_prior_moments(prior)
        if self._moments is None and not _is_box_uniform(prior):
            raise NotImplementedError("sbi_amd NPSE iid: 'fnpe' runs under a Gaussian (MultivariateNormal, "
                                      "Independent(Normal)) or BoxUniform prior; the score of any other prior is "
                                      "not linear in theta")

    def tables(self, times: Tensor, conditions: Tensor) -> IIDTables:
        N = conditions.shape[0]
        D = self.vector_field_estimator.input_shape[0]
        t = torch.as_tensor(times, dtype=torch.float64).detach().cpu().reshape(-1)
        tb = self._single(t.numel(), D)
        tb.base_scale = 1.0 / math.sqrt(N)
        if N == 1 or self._moments is None:      # one observation, or a flat prior: no prior term
            return tb
        mu0, sigma0, _ = self._moments
        w = torch.as_tensor(self.prior_score_weight_fn(t), dtype=torch.float64).reshape(-1)
        A = -(1 - N) * w[:, None, None] * torch.linalg.inv(sigma0)
        tb.mats[:, 2] = A
        tb.vecs = -(A @ mu0)
        return tb


class BaseGaussCorrectedScoreFunction(IIDScoreFunction):
    """Linhart et al. 2024 / Gloeckler et al. 2024 (vector_field_adaptor.py:816-1031), Gaussian priors."""

    def __init__(self, vector_field_estimator, prior, ensure_lam_psd: bool = True, lam_psd_nugget: float = 0.01,
                 device="cpu") -> None:
        super().__init__(vector_field_estimator, prior, device)
        self.ensure_lam_psd = ensure_lam_psd
        self.lam_psd_nugget = lam_psd_nugget
        self._moments = gaussian_prior_moments(prior)
        if self._moments is None:
            raise NotImplementedError("sbi_amd NPSE iid: 'gauss' / 'auto_gauss' need a Gaussian prior "
                                      "(MultivariateNormal or Independent(Normal)): under BoxUniform or any other prior "
                                      "the denoised prior precision depends on theta; what runs there is 'fnpe'")

    def posterior_precision_est_fn(self, conditions: Tensor) -> Tensor:
        """(N, D) diagonal or (N, D, D) dense posterior precisions, fp64 on the host."""
        raise NotImplementedError

    def tables(self, times: Tensor, conditions: Tensor) -> IIDTables:
        N = conditions.shape[0]
        D = self.vector_field_estimator.input_shape[0]
        m, s = self._ms(times)
        K = m.numel()
        if N == 1:
            return self._single(K, D)
        mu0, sigma0, prior_diag = self._moments
        prec = self.posterior_precision_est_fn(conditions).double().cpu()
        lam_diag = prec.dim() == 2
        lam = torch.diag_embed(prec) if lam_diag else prec
        eye = torch.eye(D, dtype=torch.float64)
        sigma0_inv = torch.linalg.inv(sigma0)
        mats = torch.empty(K, 3, D, D, dtype=torch.float64)
        vecs = torch.empty(K, D, dtype=torch.float64)
        for k in range(K):
            c = m[k] ** 2 / s[k] ** 2
            P0 = sigma0_inv + c * eye
            M = torch.linalg.inv(m[k] ** 2 * sigma0 + s[k] ** 2 * eye)
            Lam = (1 - N) * P0 + N * c * eye + lam.sum(0)
            corr = torch.zeros_like(eye)
            if self.ensure_lam_psd:
                if (prior_diag and lam_diag) or D == 1:      # sbi's element-wise branch (Lam is a vector there)
                    d = torch.diagonal(Lam)
                    corr = torch.diag(torch.where(d > 0, torch.zeros_like(d), -d) / (N - 1) + self.lam_psd_nugget)
                else:
                    ev, V = torch.linalg.eigh(Lam)
                    fix = torch.where(ev <= 0, -ev, torch.zeros_like(ev)) / (N - 1)
                    corr = (V * fix) @ V.T + self.lam_psd_nugget * eye
            Linv = torch.linalg.inv(Lam + N * corr)
            A = -(1 - N) * Linv @ P0 @ M
            mats[k, 0], mats[k, 1], mats[k, 2] = Linv, c * eye + corr, A
            vecs[k] = -(A @ (m[k] * mu0))
        return IIDTables(lam, mats, vecs)


class GaussCorrectedScoreFn(BaseGaussCorrectedScoreFunction):
    """Posterior precision = ``scale_from_prior_precision`` / prior variance unless given
    (vector_field_adaptor.py:1034-1135)."""

    def __init__(self, vector_field_estimator, prior, posterior_precision: Optional[Tensor] = None,
                 scale_from_prior_precision: float = 2.0, enable_lam_psd: bool = False, lam_psd_nugget: float = 0.01,
                 device="cpu") -> None:
        super().__init__(vector_field_estimator, prior, enable_lam_psd, lam_psd_nugget, device=device)
        if posterior_precision is None:      # scale / prior.variance, from the prior's parameters in fp64
            posterior_precision = scale_from_prior_precision / torch.diagonal(self._moments[1])
        self.posterior_precision = torch.as_tensor(posterior_precision).detach().double().cpu()

    def posterior_precision_est_fn(self, conditions: Tensor) -> Tensor:
        p = self.posterior_precision
        return p.expand(conditions.shape[0], *p.shape).clone()


class AutoGaussCorrectedScoreFn(BaseGaussCorrectedScoreFunction):
    """Posterior precisions estimated from draws of every single-observation posterior
    (vector_field_adaptor.py:1138-1270): ``sample_batched((budget,), x=conditions, steps=...)`` on the fused SDE sampler,
    second moment / (budget - 1), inverse (or 1 / variance with ``precision_est_only_diag``).  Cached per estimator and
    conditions."""

    def __init__(self, vector_field_estimator, prior, enable_lam_psd: bool = True, lam_psd_nugget: float = 0.01,
                 precision_est_only_diag: bool = False, precision_est_budget: Optional[int] = None,
                 precision_initial_sampler_steps: int = 100, device="cpu") -> None:
        super().__init__(vector_field_estimator, prior, enable_lam_psd, lam_psd_nugget, device=device)
        self.precision_est_only_diag = precision_est_only_diag
        self.precision_est_budget = precision_est_budget
        self.precision_initial_sampler_steps = precision_initial_sampler_steps

    def posterior_precision_est_fn(self, conditions: Tensor) -> Tensor:
        return self.estimate_posterior_precision(
            self.vector_field_estimator, self.prior, conditions, self.precision_est_only_diag,
            self.precision_est_budget, self.precision_initial_sampler_steps)

    @classmethod
    def estimate_posterior_precision(cls, vector_field_estimator, prior, conditions: Tensor,
                                     precision_est_only_diag: bool = False, precision_est_budget: Optional[int] = None,
                                     precision_initial_sampler_steps: int = 100) -> Tensor:
        from sbi_amd.inference.posteriors.vector_field_posterior import VectorFieldPosterior

        D = vector_field_estimator.input_shape[0]
        if precision_est_budget is None:
            precision_est_budget = int(math.sqrt(D) * 1000) if precision_est_only_diag else min(int(D * 1000), 5000)
        params = vector_field_estimator.net.flat_params
        key = (params._version, params.data_ptr(), conditions.detach().cpu().numpy().tobytes(),
               tuple(conditions.shape), precision_est_only_diag, precision_est_budget, precision_initial_sampler_steps)
        cache = vector_field_estimator.__dict__.setdefault("_iid_precision_cache", {})      # lives and dies with the estimator
        if key in cache:
            return cache[key]
        posterior = VectorFieldPosterior(vector_field_estimator, prior, device=str(conditions.device), sample_with="sde")
        thetas = posterior.sample_batched(torch.Size([precision_est_budget]), x=conditions,
                                          steps=precision_initial_sampler_steps).double().cpu()
        if precision_est_only_diag:
            precisions = 1 / torch.var(thetas, dim=0)
        else:
            cov = torch.einsum("bnd,bne->nde", thetas, thetas) / (precision_est_budget - 1)
            precisions = torch.linalg.inv(cov)
        while len(cache) >= 8:                       # oldest first
            cache.pop(next(iter(cache)))
        cache[key] = precisions
        return precisions


IID_METHODS: Dict[str, Type[IIDScoreFunction]] = {
    "fnpe": FactorizedNPEScoreFunction,
    "gauss": GaussCorrectedScoreFn,
    "auto_gauss": AutoGaussCorrectedScoreFn,
}


def get_iid_method(name: str) -> Type[IIDScoreFunction]:
    if name == "jac_gauss":
        raise NotImplementedError("sbi_amd NPSE iid: 'jac_gauss' is not implemented (its precision is the Jacobian of the "
                                  "score network at every theta and step); what runs: 'fnpe', 'gauss', 'auto_gauss'")
    if name not in IID_METHODS:
        raise NotImplementedError(f"Method {name} for iid score accumulation not implemented. Use one of "
                                  f"{sorted(IID_METHODS)}.")
    return IID_METHODS[name]
