"""What MCABC and SMCABC share (sbi/inference/abc/abc_base.py): the distance, the batched simulator, and the two
regressions -- linear regression adjustment (Beaumont et al. 2002) and semi-automatic summary statistics (Fearnhead &
Prangle 2012) -- solved with torch.linalg on the host in fp64 (no scikit-learn at run time)."""

from __future__ import annotations

import itertools
import logging
from typing import Callable, Dict, Optional, Union

import torch
from torch import Tensor

from sbi_amd.simulators.simutils import simulate_in_batches
from sbi_amd.utils.metrics import Distance


def fit_linear(x: Tensor, y: Tensor, sample_weight: Optional[Tensor] = None):
    """Least squares with an intercept, y ~ intercept + x @ coef, optionally weighted: (coef (features, targets),
    intercept (targets,)), fp64 on the host.  The minimum-norm solution when x is rank deficient."""
    x64, y64 = x.detach().double().cpu(), y.detach().double().cpu()
    design = torch.cat((torch.ones(x64.shape[0], 1, dtype=torch.float64), x64), dim=1)
    if sample_weight is not None:
        root = sample_weight.detach().double().cpu().reshape(-1, 1).sqrt()
        design, y64 = design * root, y64 * root
    sol = torch.linalg.lstsq(design, y64, driver="gelsd").solution
    return sol[1:], sol[0]


def polynomial_features(x: Tensor, degree: int) -> Tensor:
    """All monomials of the columns of x of total degree 1 .. degree, without the constant: degree by degree, each in
    the order of combinations with replacement of the column indices."""
    cols = []
    for deg in range(1, degree + 1):
        for combo in itertools.combinations_with_replacement(range(x.shape[1]), deg):
            cols.append(x[:, list(combo)].prod(dim=1))
    return torch.stack(cols, dim=1)


class ABCBASE:
    """Base class of the Approximate Bayesian Computation samplers."""

    def __init__(self, simulator: Callable, prior, distance: Union[str, Callable] = "l2",
                 requires_iid_data: Optional[bool] = None, distance_kwargs: Optional[Dict] = None,
                 num_workers: int = 1, simulation_batch_size: int = 1, distance_batch_size: int = -1,
                 show_progress_bars: bool = True) -> None:
        if num_workers != 1:
            raise NotImplementedError("sbi_amd: ABC simulates in one process (num_workers=1): worker processes forked "
                                      "from a process that holds the GPU are not started here.")
        self.prior = prior
        self._simulator = simulator
        self._show_progress_bars = show_progress_bars
        self.x_o = None
        self.x_shape = None
        self.distance = Distance(distance, requires_iid_data, distance_kwargs, batch_size=distance_batch_size)

        def batched_simulator(theta: Tensor) -> Tensor:
            x = simulate_in_batches(self._simulator, theta, simulation_batch_size, num_workers,
                                    show_progress_bars=self._show_progress_bars)
            return torch.as_tensor(x, dtype=torch.float32).to(theta.device)      # (data live where the prior samples)

        self._batched_simulator = batched_simulator
        self.logger = logging.getLogger(__name__)

    @staticmethod
    def _get_sass_transform(theta: Tensor, x: Tensor, expansion_degree: int = 1,
                            sample_weight: Optional[Tensor] = None) -> Callable[[Tensor], Tensor]:
        """The semi-automatic summary statistics x -> expansion(x) @ coef of the regression of theta on the polynomial
        expansion of x (no bias column; the intercept is fitted and dropped)."""
        coef, _ = fit_linear(polynomial_features(x.reshape(x.shape[0], -1), expansion_degree), theta, sample_weight)
        sumstats_map = coef.to(torch.float32)

        def sumstats_transform(data: Tensor) -> Tensor:
            data = torch.as_tensor(data, dtype=torch.float32)
            expanded = polynomial_features(data.reshape(data.shape[0], -1), expansion_degree)
            return expanded.mm(sumstats_map.to(expanded.device))

        return sumstats_transform

    @staticmethod
    def _run_lra(theta: Tensor, x: Tensor, observation: Tensor, sample_weight: Optional[Tensor] = None) -> Tensor:
        """theta + m(x_o) - m(x) with m the (weighted) linear regression of theta on x."""
        xf = x.reshape(x.shape[0], -1)
        coef, intercept = fit_linear(xf, theta, sample_weight)
        pred_obs = observation.detach().double().cpu().reshape(1, -1) @ coef + intercept
        pred_sim = xf.detach().double().cpu() @ coef + intercept
        return theta + (pred_obs - pred_sim).to(dtype=theta.dtype, device=theta.device)
