"""CPU restatement of the NPSE score estimator -- TEST INFRASTRUCTURE ONLY (never imported by sbi_amd/).

The trunk is `oracle.fmpe_oracle.FMPEOracle.net` (the same VectorFieldMLP the flow-matching estimator uses); around it
this module restates, literally and in the module's dtype, what sbi computes in

* ConditionalScoreEstimator.forward / loss / ode_fn     sbi/neural_nets/estimators/score_estimator.py:149-316, 511-528
* VP / SubVP / VE mean_t_fn, std_fn, drift_fn, diffusion_fn, weights          score_estimator.py:499-509, 582-975
* Diffuser.run with the Euler-Maruyama predictor          sbi/samplers/score/diffuser.py:124-172, predictors.py:112-120

tests/test_npse_host_cpu.py pins it to outputs of the real classes (tests/golden/npse_reference.pt): in fp64 it must
reproduce the fp64 record of loss and gradient to 1e-9, so it can be trusted on configurations the fixture lacks.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor, nn

from oracle.fmpe_oracle import FMPEOracle

SDE_DEFAULT_T_MIN = {"ve": 1e-3, "vp": 1e-3, "subvp": 1e-2}


class NPSEOracle(nn.Module):
    def __init__(self, D: int, C: int, sde: str = "ve", H: int = 100, L: int = 5, E: int = 32,
                 weight: str = "max_likelihood", beta_min: float = 0.01, beta_max: float = 10.0,
                 sigma_min: float = 1e-4, sigma_max: float = 10.0, t_min: Optional[float] = None, t_max: float = 1.0):
        super().__init__()
        assert sde in ("ve", "vp", "subvp") and weight in ("identity", "max_likelihood", "variance")
        self.o = FMPEOracle(D, C, H=H, L=L, E=E)
        self.D, self.C, self.sde, self.weight = D, C, sde, weight
        self.beta_min, self.beta_max, self.sigma_min, self.sigma_max = beta_min, beta_max, sigma_min, sigma_max
        self.t_min, self.t_max = SDE_DEFAULT_T_MIN[sde] if t_min is None else t_min, t_max

    def load_reference_state_dict(self, sd: Dict[str, Tensor]) -> None:
        self.o.load_reference_state_dict(sd)
        # the reference keeps the base moments as fp32 buffers computed once at construction
        self._base = (sd["_mean_base"].reshape(1, -1), sd["_std_base"].reshape(1, -1)) if "_mean_base" in sd else None

    # ------------------------------------------------------------------ SDE pieces, times (N,) -> (N,)
    def mean_t(self, t: Tensor) -> Tensor:
        if self.sde == "ve":
            return torch.ones_like(t)
        return torch.exp(-0.25 * t**2.0 * (self.beta_max - self.beta_min) - 0.5 * t * self.beta_min)

    def std_t(self, t: Tensor) -> Tensor:
        if self.sde == "ve":
            return self.sigma_min * (self.sigma_max / self.sigma_min) ** t
        v = 1.0 - torch.exp(-0.5 * t**2.0 * (self.beta_max - self.beta_min) - t * self.beta_min)
        return torch.sqrt(v) if self.sde == "vp" else v

    def noise_schedule(self, t: Tensor) -> Tensor:
        if self.sde == "ve":
            return self.sigma_min * (self.sigma_max / self.sigma_min) ** t
        return self.beta_min + (self.beta_max - self.beta_min) * t

    def drift(self, theta: Tensor, t: Tensor) -> Tensor:
        if self.sde == "ve":
            return torch.zeros_like(theta)
        return (-0.5 * self.noise_schedule(t))[:, None] * theta

    def diffusion(self, t: Tensor) -> Tensor:
        if self.sde == "ve":
            return self.noise_schedule(t) * math.sqrt(2 * math.log(self.sigma_max / self.sigma_min))
        if self.sde == "vp":
            return torch.sqrt(self.noise_schedule(t))
        return torch.sqrt(torch.abs(self.noise_schedule(t) * (
            1 - torch.exp(-2 * self.beta_min * t - (self.beta_max - self.beta_min) * t**2))))

    def weight_fn(self, t: Tensor) -> Tensor:
        if self.weight == "identity":
            return torch.ones_like(t)
        return self.diffusion(t) ** 2 if self.weight == "max_likelihood" else self.std_t(t) ** 2

    def marginal(self, t: Tensor):
        m = self.mean_t(t)[:, None]
        mean = m * self.o.mean_0[None, :]
        std = torch.sqrt(m**2 * self.o.std_0[None, :] ** 2 + self.std_t(t)[:, None] ** 2)
        return mean, std

    def base(self):
        """mean_base, std_base: the marginal at t_max (the loaded buffers when a reference state was loaded)."""
        if getattr(self, "_base", None) is not None:
            return tuple(b.to(self.o.mean_0) for b in self._base)
        t = torch.tensor([self.t_max], dtype=self.o.mean_0.dtype, device=self.o.mean_0.device)
        return self.marginal(t)

    # ------------------------------------------------------------------ estimator interface
    def score(self, theta_t: Tensor, x: Tensor, t: Tensor) -> Tensor:
        """theta_t (N, D), x (N, C) or (1, C), t (N,)."""
        n = theta_t.shape[0]
        mean, std = self.marginal(t)
        pred = self.o.net((theta_t - mean) / std, self.o.embed(x).expand(n, -1), self.std_t(t))
        scale = (self.mean_t(t) / self.std_t(t))[:, None]
        return -scale * pred - (theta_t - mean) / std**2

    def ode_fn(self, theta_t: Tensor, x: Tensor, t: Tensor) -> Tensor:
        return self.drift(theta_t, t) - 0.5 * self.diffusion(t)[:, None] ** 2 * self.score(theta_t, x, t)

    def loss(self, theta: Tensor, x: Tensor, times: Tensor, eps: Tensor, control_variate: bool = True,
             control_variate_threshold: float = 0.3) -> Tensor:
        mean = self.mean_t(times)[:, None] * theta
        std = self.std_t(times)[:, None]
        target = -eps / std
        pred = self.score(mean + std * eps, x, times)
        loss = torch.sum((pred - target) ** 2.0, dim=-1)
        if control_variate:
            s = std[:, 0]
            pred_mean = self.score(mean, x, times)
            term1 = 2 / s * torch.sum(eps * pred_mean, dim=-1)
            term2 = torch.sum(eps**2, dim=-1) / s**2
            term3 = self.D / s**2
            cv = term3 - term1 - term2
            loss = loss + torch.where(s < control_variate_threshold, cv, torch.zeros_like(cv))
        return self.weight_fn(times) * loss

    @torch.no_grad()
    def sample_sde(self, x: Tensor, ts: Tensor, noise: Optional[Tensor], eta: float = 1.0, n: int = 0) -> Tensor:
        """Euler-Maruyama replay: noise (len(ts), N, D) holds the initial draw and one draw per step; None draws n rows
        with torch.randn as the reference does (the eager baseline of tools/bench_npse.py)."""
        mean_b, std_b = self.base()
        if noise is None:
            noise = _Draws((n, self.D), mean_b)
        theta = mean_b + std_b * noise[0]
        n = theta.shape[0]
        for k in range(1, ts.numel()):
            t1, t0 = ts[k - 1], ts[k]
            dt = t1 - t0
            tt = t1.expand(n)
            g = self.diffusion(tt)[:, None]
            fb = self.drift(theta, tt) - (1 + eta**2) / 2 * g**2 * self.score(theta, x, tt)
            theta = theta - fb * dt + eta * g * noise[k] * torch.sqrt(dt)
        return theta


class _Draws:
    def __init__(self, shape, like):
        self.shape, self.like = shape, like

    def __getitem__(self, k):
        return torch.randn(self.shape, dtype=self.like.dtype, device=self.like.device)


def flat_grad(oracle: NPSEOracle, slices) -> Tensor:
    """Gradients of the trunk parameters in the flat order of `VectorFieldMLPParams.slices()`."""
    chunks = [oracle.o.p[("net." + key).replace(".", "/")].grad.reshape(-1) for key, _, _, _ in slices]
    return torch.cat(chunks)


class OracleScoreField(nn.Module):
    """The oracle behind the estimator surface the NPSE trainer uses (loss, solve_schedule, t_min, t_max), for host
    logic without a GPU.  Times and eps are deterministic functions of the row."""

    def __init__(self, theta, x, sde="vp", **kw):
        super().__init__()
        self.o = NPSEOracle(theta.shape[1], x.shape[1], sde=sde, **kw)
        with torch.no_grad():
            self.o.o.mean_0.copy_(theta.mean(0))
            self.o.o.std_0.copy_(theta.std(0))
            self.o.o.x_mean.copy_(x.mean(0))
            self.o.o.x_std.copy_(x.std(0))
        self.input_shape, self.condition_shape = theta[0].shape, x[0].shape
        self.t_min, self.t_max = self.o.t_min, self.o.t_max

    def solve_schedule(self, steps, t_min=None, t_max=None):
        return torch.linspace(self.t_max if t_max is None else t_max, self.t_min if t_min is None else t_min, steps)

    def loss(self, input, condition, times=None, **kwargs):
        key = input.sum(-1, keepdim=True)
        if times is None:
            times = self.t_min + (self.t_max - self.t_min) * torch.frac(key[:, 0].abs() * 7.31)
        eps = torch.sin(key * torch.arange(1, input.shape[1] + 1) * 3.7) * 1.3
        return self.o.loss(input, condition, times, eps)


def oracle_score_build_fn(**kw):
    def build(theta, x):
        return OracleScoreField(theta, x, **kw)

    return build
