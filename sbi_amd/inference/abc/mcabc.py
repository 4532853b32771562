"""Monte-Carlo (rejection) Approximate Bayesian Computation (sbi/inference/abc/mcabc.py)."""

from __future__ import annotations

from typing import Any, Callable, Dict, Optional, Union

import torch
from torch import Tensor

from sbi_amd.inference.abc.abc_base import ABCBASE
from sbi_amd.utils.kde import get_kde
from sbi_amd.utils.sbiutils import assert_all_finite, process_x


class MCABC(ABCBASE):
    """Rejection ABC: simulate from the prior, keep the parameters whose data lie closest to the observation."""

    def __init__(self, simulator: Callable, prior, distance: Union[str, Callable] = "l2",
                 requires_iid_data: Optional[bool] = None, distance_kwargs: Optional[Dict] = None,
                 num_workers: int = 1, simulation_batch_size: int = 1, distance_batch_size: int = -1,
                 show_progress_bars: bool = True):
        super().__init__(simulator=simulator, prior=prior, distance=distance, requires_iid_data=requires_iid_data,
                         distance_kwargs=distance_kwargs, num_workers=num_workers,
                         simulation_batch_size=simulation_batch_size, distance_batch_size=distance_batch_size,
                         show_progress_bars=show_progress_bars)

    def __call__(self, x_o, num_simulations: int, eps: Optional[float] = None, quantile: Optional[float] = None,
                 lra: bool = False, sass: bool = False, sass_fraction: float = 0.25, sass_expansion_degree: int = 1,
                 kde: bool = False, kde_kwargs: Optional[Dict[str, Any]] = None, return_summary: bool = False,
                 num_iid_samples: int = 1):
        """Accepted parameters (or a KDE fitted on them, with `kde`), and with `return_summary` a dict of the accepted
        `distances` and `x` (and `theta` when `kde`).  Exactly one of `eps` (accept distance < eps) and `quantile`
        (keep the int(num_simulations * quantile) closest, in ascending order) is given."""
        assert (eps is not None) ^ (quantile is not None), "Eps or quantile must be passed, but not both."
        kde_kwargs = {} if kde_kwargs is None else kde_kwargs

        if sass:      # a pilot run fits the summary statistics; simulator and x_o go through them from here on
            num_pilot_simulations = int(sass_fraction * num_simulations)
            self.logger.info("Running SASS with %s pilot samples.", num_pilot_simulations)
            num_simulations -= num_pilot_simulations
            pilot_theta = self.prior.sample((num_pilot_simulations,))
            pilot_x = self._batched_simulator(pilot_theta)
            sass_transform = self._get_sass_transform(pilot_theta, pilot_x, sass_expansion_degree)

            def simulator(theta):
                return sass_transform(self._batched_simulator(theta))

            x_o = sass_transform(process_x(x_o).to(pilot_x.device))
        else:
            simulator = self._batched_simulator

        theta = self.prior.sample((num_simulations,))
        x = simulator(theta.repeat_interleave(num_iid_samples, dim=0))
        x = x.reshape((num_simulations, num_iid_samples, -1))
        if not self.distance.requires_iid_data:
            x = x.squeeze(1)
            self.x_shape = x[0].shape
        else:
            self.x_shape = x[0, 0].shape
        self.x_o = process_x(x_o, self.x_shape).to(x.device)
        assert_all_finite(self.x_o, "Observed data x_o")
        distances = self.distance(self.x_o, x)

        if eps is not None:
            is_accepted = distances < eps
            num_accepted = is_accepted.sum().item()
            assert num_accepted > 0, f"No parameters accepted, eps={eps} too small"
            theta_accepted, distances_accepted, x_accepted = theta[is_accepted], distances[is_accepted], x[is_accepted]
        else:
            num_top_samples = int(num_simulations * quantile)
            sort_idx = torch.argsort(distances, stable=True)[:num_top_samples]     # (ties: simulation order)
            theta_accepted, distances_accepted, x_accepted = theta[sort_idx], distances[sort_idx], x[sort_idx]

        if lra:
            self.logger.info("Running Linear regression adjustment.")
            final_theta = self._run_lra(theta_accepted, x_accepted, observation=self.x_o)
        else:
            final_theta = theta_accepted

        if kde:
            self.logger.info("KDE on %s samples with bandwidth option %s. Beware that KDE can give unreliable results "
                             "when used with too few samples and in high dimensions.", final_theta.shape[0],
                             kde_kwargs.get("bandwidth", "cv"))
            kde_dist = get_kde(final_theta, **kde_kwargs)
            if return_summary:
                return kde_dist, dict(theta=final_theta, distances=distances_accepted, x=x_accepted)
            return kde_dist
        if return_summary:
            return final_theta, dict(distances=distances_accepted, x=x_accepted)
        return final_theta
