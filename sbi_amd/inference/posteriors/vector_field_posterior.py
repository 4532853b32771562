"""Posterior that samples a vector-field estimator on the device: the probability-flow ODE of a flow-matching or score
estimator, or the reverse SDE of a score estimator (NPSE) with the fused Euler-Maruyama kernel.

Mirror of sbi's ``VectorFieldPosterior`` for ``sample_with="ode"``
(sbi/inference/posteriors/vector_field_posterior.py:155-330, 436-466): draw theta_1 ~ N(mean_base, std_base),
integrate d theta / dt = v(theta, t; x_o) from t_max to t_min, reject draws outside the prior support.
``log_prob`` integrates the same ODE in the other direction together with the exact divergence of the vector field
(zuko's exact-trace transform in sbi; here one HIP launch returns velocity and Jacobian trace).

``sample_with="sde"`` (:331-434 -> samplers/score/diffuser.py:124-172, predictors.py:112-120) is for score estimators:
draw theta ~ N(mean_base, std_base) at ``ts[0]`` and take ``len(ts) - 1`` Euler-Maruyama steps of the reverse SDE, all in
one launch per batch (``sbi_amd_npse_sample_sde``).  The draws come from Philox keyed by a seed taken from torch's
generator once per call and indexed by the candidate's running number, so for a given ``torch.manual_seed`` the returned
samples do NOT depend on how ``max_sampling_batch_size`` splits the work.

Several rows of ``x`` in ``sample`` are N iid observations (:331-397 with ``iid_method``, default "auto_gauss"): the score
of every step is the fnpe / gauss / auto_gauss composition of the per-observation scores
(``sbi_amd.inference.potentials.vector_field_adaptor``: its theta-independent part is tabulated in fp64 on the host once
per call).  Two legs evaluate it with the same Philox keying: a host loop with one ``sbi_amd_npse_score`` launch per step
on the n N expanded rows and a per-row composition kernel (the default: it measured faster, profiles/npse_iid_bench.json), and
the fused sampler ``sbi_amd_npse_sample_sde_iid`` (all steps in one launch; D <= 16, N <= 1024, at most 65535 steps).  The composition runs on a ROCm device only: a posterior on any other
device refuses iid observations and ``iid_method``.

Refused with ``NotImplementedError``: correctors, guidance, predictors other than "euler_maruyama", ``iid_method``
"jac_gauss", gauss / auto_gauss under a non-Gaussian prior, iid observations with ``sample_with="ode"`` or with a
flow-matching estimator, and ``log_prob`` of a score-based posterior (it needs the divergence of ``ode_fn``).
"""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from sbi_amd.samplers.ode_solvers import odeint_dopri5
from sbi_amd.utils.sbiutils import within_support


class VectorFieldPosterior:
    def __init__(self, vector_field_estimator, prior, device: Optional[str] = None, atol: float = 1e-6,
                 rtol: float = 1e-5, max_sampling_batch_size: int = 100_000, sample_with: Optional[str] = None):
        if sample_with not in (None, "ode", "sde"):
            raise ValueError(f"sample_with must be 'ode' or 'sde', but is {sample_with}.")
        self.sample_with = sample_with or "ode"
        self.vector_field_estimator = vector_field_estimator
        self.prior = prior
        self._device = device or str(next(vector_field_estimator.parameters()).device)
        self.atol, self.rtol = atol, rtol
        self.max_sampling_batch_size = max_sampling_batch_size
        self._x: Optional[Tensor] = None

    @property
    def default_x(self) -> Optional[Tensor]:
        return self._x

    def set_default_x(self, x: Tensor) -> "VectorFieldPosterior":
        self._x = self._process_x(x)
        return self

    def _process_x(self, x: Tensor) -> Tensor:
        x = torch.as_tensor(x, dtype=torch.float32)
        cshape = self.vector_field_estimator.condition_shape
        if x.dim() == len(cshape):
            x = x.unsqueeze(0)
        if self._is_score() and x.dim() == len(cshape) + 1 and x.shape[0] > 1 and x.shape[1:] == cshape:
            if not self._on_rocm():
                raise NotImplementedError("sbi_amd NPSE: iid observations (several rows of x: the fnpe / gauss / auto_gauss "
                                          "score composition) run on the device only; this posterior lives on "
                                          f"{self._device!r}.  One observation per call, or sample_batched for "
                                          "independent observations")
            return x.to(self._device).contiguous()
        if not self._is_score() and x.dim() == len(cshape) + 1 and x.shape[0] > 1 and x.shape[1:] == cshape:
            raise NotImplementedError("sbi_amd FMPE: sampling given iid observations (several rows of x) is not "
                                      "implemented: the score composition runs for score estimators (NPSE) only; "
                                      "log_prob accepts iid observations, sample_batched independent ones")
        if x.shape[0] != 1 or x.shape[1:] != cshape:
            raise ValueError(f"expected one observation of shape {tuple(cshape)}, got {tuple(x.shape)}; use "
                             "sample_batched for several observations")
        return x.to(self._device)

    def _x_else_default_x(self, x: Optional[Tensor]) -> Tensor:
        if x is not None:
            return self._process_x(x)
        if self._x is None:
            raise ValueError("Context `x` needed when a default has not been set. Use `.set_default_x(x)` or pass "
                             "`x` explicitly.")
        return self._x

    def _on_rocm(self) -> bool:
        return torch.device(self._device).type == "cuda"

    def _is_score(self) -> bool:
        from sbi_amd.neural_nets.estimators.score_estimator import ConditionalScoreEstimator

        return isinstance(self.vector_field_estimator, ConditionalScoreEstimator)

    def _sde_setup(self, steps, ts, predictor, corrector, predictor_params, corrector_params, iid_method=None):
        """Arguments of `_sample_via_diffusion` (vector_field_posterior.py:331-397) -> (ts on the device, eta, seed)."""
        if not self._is_score():
            raise NotImplementedError("sbi_amd FMPE posterior samples with the probability-flow ODE only")
        if corrector is not None or corrector_params:
            raise NotImplementedError("sbi_amd NPSE: correctors are not implemented (predictor-only Euler-Maruyama)")
        if predictor != "euler_maruyama":
            raise NotImplementedError(f"sbi_amd NPSE implements the 'euler_maruyama' predictor only, got {predictor!r}")
        if iid_method is not None:
            from sbi_amd.inference.potentials.vector_field_adaptor import get_iid_method

            get_iid_method(iid_method)        # unknown names and jac_gauss are refused here
            if not self._on_rocm():
                raise NotImplementedError("sbi_amd NPSE: iid score composition (iid_method) runs on the device only; this "
                                          f"posterior lives on {self._device!r}")
        params = dict(predictor_params or {})
        eta = float(params.pop("eta", 1.0))
        if params:
            raise TypeError(f"unsupported predictor_params: {sorted(params)}")
        if not eta > 0:
            raise AssertionError("eta must be positive.")
        est = self.vector_field_estimator
        ts = est.solve_schedule(steps) if ts is None else torch.as_tensor(ts, dtype=torch.float32)
        ts = ts.to(device=self._device, dtype=torch.float32).reshape(-1).contiguous()
        seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
        return ts, eta, seed

    @torch.no_grad()
    def sample_via_sde(self, num_samples: int, x: Tensor, ts: Tensor, eta: float = 1.0, seed: int = 0,
                       row_offset: int = 0) -> Tensor:
        from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_fused, sample_sde_loop

        est = self.vector_field_estimator
        cond = (x if x.shape[0] == num_samples else x[:1]).contiguous()
        if ts.numel() - 1 > 65535:        # beyond the fused kernel's step counter: one score launch per step
            return sample_sde_loop(est, num_samples, cond, ts, eta)
        return sample_sde_fused(est, num_samples, cond, ts, eta, None, seed, row_offset)

    def _iid_setup(self, x: Tensor, grid: Tensor, iid_method: Optional[str], iid_params: Optional[dict]):
        """Tables of the composed score at grid[:-1] on the device: (lam, step_mats, step_vecs, base_scale)."""
        from sbi_amd.inference.potentials.vector_field_adaptor import get_iid_method

        fn = get_iid_method(iid_method or "auto_gauss")(self.vector_field_estimator, self.prior, device=self._device,
                                                        **(iid_params or {}))
        tb = fn.tables(grid[:-1].cpu(), x)
        return (*tb.on(self._device), tb.base_scale)

    @torch.no_grad()
    def sample_via_sde_iid(self, num_samples: int, x: Tensor, ts: Tensor, tables, eta: float = 1.0, seed: int = 0,
                           row_offset: int = 0) -> Tensor:
        from sbi_amd.neural_nets.estimators.score_estimator import sample_sde_iid

        lam, mats, vecs, base_scale = tables
        return sample_sde_iid(self.vector_field_estimator, num_samples, x, ts, lam, mats, vecs, eta, seed, row_offset,
                              base_scale)

    @torch.no_grad()
    def sample_via_ode(self, num_samples: int, x: Tensor) -> Tensor:
        est = self.vector_field_estimator
        D = est.input_shape[0]
        eps = est.mean_base + est.std_base * torch.randn(num_samples, D, device=self._device)
        cond = x if x.shape[0] == num_samples else x[:1]
        return odeint_dopri5(lambda t, y: est.ode_fn(y, cond, t), eps.contiguous(), est.t_max, est.t_min,
                             atol=self.atol, rtol=self.rtol)

    @torch.no_grad()
    def sample(self, sample_shape=torch.Size(), x: Optional[Tensor] = None, max_sampling_batch_size: Optional[int] = None,
               sample_with: Optional[str] = None, show_progress_bars: bool = False,
               reject_outside_prior: bool = True, predictor: str = "euler_maruyama", corrector: Optional[str] = None,
               predictor_params: Optional[dict] = None, corrector_params: Optional[dict] = None, steps: int = 500,
               ts: Optional[Tensor] = None, iid_method: Optional[str] = None, iid_params: Optional[dict] = None,
               guidance_method: Optional[str] = None, guidance_params: Optional[dict] = None, **unsupported) -> Tensor:
        sample_with = sample_with or self.sample_with
        if sample_with not in ("ode", "sde"):
            raise ValueError(f"Expected sample_with to be 'ode' or 'sde', but got {sample_with}.")
        if guidance_method is not None or guidance_params:
            raise NotImplementedError("sbi_amd NPSE: guidance is not implemented; what runs: the plain score and the "
                                      "fnpe / gauss / auto_gauss composition of iid observations")
        if sample_with == "sde":
            grid, eta, seed = self._sde_setup(steps, ts, predictor, corrector, predictor_params, corrector_params,
                                              iid_method)
        x = self._x_else_default_x(x)
        iid = None            # one observation: iid_method is accepted and ignored, as in sbi
        if x.shape[0] > 1:
            if sample_with != "sde":
                raise NotImplementedError("sbi_amd NPSE: iid observations are sampled with sample_with='sde' only (the "
                                          "composed score drives the reverse SDE)")
            iid = self._iid_setup(x, grid, iid_method, iid_params)
        num = int(torch.Size(sample_shape).numel())
        cap = max_sampling_batch_size or self.max_sampling_batch_size
        out, have, tries, drawn = [], 0, 0, 0
        while have < num:
            n = min(cap, max(num - have, 16))
            if iid is not None:
                draws = self.sample_via_sde_iid(n, x, grid, iid, eta, seed, row_offset=drawn)
            elif sample_with == "ode":
                draws = self.sample_via_ode(n, x)
            else:
                draws = self.sample_via_sde(n, x, grid, eta, seed, row_offset=drawn)
            drawn += n
            if reject_outside_prior and self.prior is not None:
                draws = draws[within_support(self.prior, draws)]
            out.append(draws)
            have += draws.shape[0]
            tries += 1
            if tries > 1000:
                raise RuntimeError("VectorFieldPosterior.sample: acceptance rate too low")
        return torch.cat(out)[:num].reshape(*torch.Size(sample_shape), -1)

    @torch.no_grad()
    def sample_batched(self, sample_shape, x: Tensor, predictor: str = "euler_maruyama", corrector: Optional[str] = None,
                       predictor_params: Optional[dict] = None, corrector_params: Optional[dict] = None,
                       steps: int = 500, ts: Optional[Tensor] = None, **kwargs) -> Tensor:
        """(sample_shape, batch, D): every observation integrates its own draws in one batched ODE solve (or one
        launch of the SDE sampler, every row conditioned on its own observation)."""
        x = torch.as_tensor(x, dtype=torch.float32).to(self._device)
        num = int(torch.Size(sample_shape).numel())
        B = x.shape[0]
        xs = x.repeat_interleave(num, dim=0).contiguous()
        if self.sample_with == "sde":
            grid, eta, seed = self._sde_setup(steps, ts, predictor, corrector, predictor_params, corrector_params)
            draws = self.sample_via_sde(num * B, xs, grid, eta, seed)
        else:
            draws = self.sample_via_ode(num * B, xs)
        return draws.reshape(B, num, -1).permute(1, 0, 2).reshape(*torch.Size(sample_shape), B, -1)

    @torch.no_grad()
    def log_prob(self, theta: Tensor, x: Optional[Tensor] = None, track_gradients: bool = False,
                 ode_kwargs: Optional[dict] = None, max_batch_size: Optional[int] = None) -> Tensor:
        r"""``(len(theta),)`` log posterior density :math:`\log p(\theta | x)` through the probability-flow ODE, -inf
        outside the prior support (sbi/inference/posteriors/vector_field_posterior.py:467-504 ->
        potentials/vector_field_potential.py:149-207): integrate the augmented state
        :math:`(\theta_t, \ell_t)' = (v, \nabla \cdot v)` from ``t_min`` (data) to ``t_max`` (noise) and add the
        base log-density of the end point -- zuko's ``FreeFormJacobianTransform(exact=True)`` inside a
        ``NormalizingFlow`` with ``DiagNormal(mean_base, std_base)`` (samplers/ode_solvers/zuko_ode.py:100-124).  The
        exact Jacobian trace comes out of the same HIP launch as the velocity (``sbi_amd_fmpe_velocity_div``); the
        state of all rows, log-det included, stays on the device for the whole solve (``odeint_dopri5``).

        ``x`` with more than one row is a set of iid observations (vector_field_posterior.py:489-497,
        vector_field_potential.py:175-192): the log-densities of the per-observation flows are summed and
        ``(n_iid - 1) * prior.log_prob(theta)`` is subtracted; that needs a prior.

        ``ode_kwargs``: ``atol`` / ``rtol`` (defaults: the posterior's, sbi's 1e-6 / 1e-5); ``exact=False`` (zuko's
        Hutchinson estimate) is not offered."""
        if self._is_score():
            raise NotImplementedError("sbi_amd NPSE: log_prob of a score-based posterior is not implemented (it needs the "
                                      "divergence of ode_fn); sample with 'sde' or 'ode'")
        if track_gradients:
            raise NotImplementedError("sbi_amd: log_prob of the flow-matching posterior does not track gradients")
        kw = dict(ode_kwargs or {})
        if not kw.pop("exact", True):
            raise NotImplementedError("sbi_amd: only the exact Jacobian trace (zuko's exact=True, sbi's default)")
        atol, rtol = float(kw.pop("atol", self.atol)), float(kw.pop("rtol", self.rtol))
        if kw:
            raise TypeError(f"unsupported ode_kwargs: {sorted(kw)}")
        est = self.vector_field_estimator
        if x is not None and torch.as_tensor(x).dim() == len(est.condition_shape) + 1 and torch.as_tensor(x).shape[0] > 1:
            xs = torch.as_tensor(x, dtype=torch.float32).to(self._device)
            if xs.shape[1:] != est.condition_shape:
                raise ValueError(f"expected observations of shape {tuple(est.condition_shape)}, got {tuple(xs.shape[1:])}")
            if self.prior is None:
                raise AssertionError("Prior is required for evaluating log_prob with iid observations.")
        else:
            xs = self._x_else_default_x(x)
        D = est.input_shape[0]
        theta = torch.as_tensor(theta, dtype=torch.float32)
        if theta.dim() == 1:
            theta = theta.unsqueeze(0)
        if theta.dim() != 2 or theta.shape[1] != D:
            raise ValueError(f"theta must have shape (batch, {D}), got {tuple(theta.shape)}")
        theta = theta.to(self._device).contiguous()
        if theta.shape[0] == 0:
            return torch.empty(0, dtype=torch.float32, device=self._device)
        cap = max_batch_size or self.max_sampling_batch_size
        log_probs = torch.zeros(theta.shape[0], dtype=torch.float32, device=self._device)
        for i_obs in range(xs.shape[0]):          # one flow per iid observation (one observation: the usual case)
            x_i = xs[i_obs : i_obs + 1]
            log_probs = log_probs + torch.cat([self._log_prob_via_ode(theta[i : i + cap], x_i, atol, rtol)
                                               for i in range(0, theta.shape[0], cap)])
        if xs.shape[0] > 1:
            log_probs = log_probs - (xs.shape[0] - 1) * self.prior.log_prob(theta).reshape(-1)
        if self.prior is not None:
            inside = within_support(self.prior, theta)
            log_probs = torch.where(inside, log_probs, torch.full_like(log_probs, float("-inf")))
        return log_probs

    def _log_prob_via_ode(self, theta: Tensor, x: Tensor, atol: float, rtol: float) -> Tensor:
        est = self.vector_field_estimator
        n, D = theta.shape
        if n == 0:
            return torch.empty(0, device=theta.device)
        # flat augmented state [theta (n x D) | ladj (n)]: both halves are contiguous views, so the right-hand side
        # kernel reads theta_t from, and writes velocity and divergence straight into, the solver's buffers
        y0 = torch.cat([theta.reshape(-1), torch.zeros(n, dtype=torch.float32, device=theta.device)])

        def rhs(t: Tensor, y: Tensor) -> Tensor:
            out = torch.empty_like(y)
            est.ode_fn_and_divergence(y[: n * D].view(n, D), x, t, v_out=out[: n * D].view(n, D), div_out=out[n * D :])
            return out

        y1 = odeint_dopri5(rhs, y0, est.t_min, est.t_max, atol=atol, rtol=rtol)
        z = (y1[: n * D].view(n, D) - est.mean_base) / est.std_base
        base = (-0.5 * z * z - torch.log(est.std_base) - 0.9189385332046727).sum(-1)
        return base + y1[n * D :]
