"""Sequential Monte-Carlo Approximate Bayesian Computation (sbi/inference/abc/smcabc.py), variants A (Toni et al. 2010),
B (Sisson et al. 2007, with resampling on a low effective sample size) and C (Beaumont et al. 2009: the kernel
covariance is the weighted covariance of the previous population).

The weight update -- for every new particle a log-sum-exp over all old particles of log w_j + log K(new_i; old_j),
a Python loop over particles in the reference -- is one call of `sbi_amd.utils.kde.mixture_lse` per population (and
per fill-up / LRA recomputation): one kernel launch on a ROCm device."""

from __future__ import annotations

import math
from typing import Any, Callable, Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from sbi_amd.inference.abc.abc_base import ABCBASE
from sbi_amd.utils.kde import get_kde, mixture_lse
from sbi_amd.utils.sbiutils import assert_all_finite, process_x, within_support


def weighted_covariance(particles: Tensor, weights: Tensor) -> Tensor:
    """np.cov(particles, rowvar=False, aweights=weights): (D, D), in fp64.  Mean and scatter are weighted by w; the
    normalisation is sum w - sum w^2 / sum w."""
    x, w = particles.double(), weights.double()
    total = w.sum()
    centred = x - (w[:, None] * x).sum(0) / total
    return (centred * w[:, None]).T @ centred / (total - (w * w).sum() / total)


class SMCABC(ABCBASE):
    """Sequential Monte-Carlo ABC."""

    def __init__(self, simulator: Callable, prior, distance: Union[str, Callable] = "l2",
                 requires_iid_data: Optional[bool] = None, distance_kwargs: Optional[Dict] = None,
                 num_workers: int = 1, simulation_batch_size: int = 1, distance_batch_size: int = -1,
                 show_progress_bars: bool = True, kernel: Optional[str] = "gaussian", algorithm_variant: str = "C"):
        super().__init__(simulator=simulator, prior=prior, distance=distance, requires_iid_data=requires_iid_data,
                         distance_kwargs=distance_kwargs, num_workers=num_workers,
                         simulation_batch_size=simulation_batch_size, distance_batch_size=distance_batch_size,
                         show_progress_bars=show_progress_bars)
        kernels = ("gaussian", "uniform")
        assert kernel in kernels, f"Kernel '{kernel}' not supported. Choose one from {kernels}."
        self.kernel = kernel
        algorithm_variants = ("A", "B", "C")
        assert algorithm_variant in algorithm_variants, (
            f"SMCABC variant '{algorithm_variant}' not supported, choose one from {algorithm_variants}.")
        self.algorithm_variant = algorithm_variant
        self.distance_to_x0 = None
        self.simulation_counter = 0
        self.num_simulations = 0
        self.kernel_variance = None
        self.num_resamples = 0           # populations resampled because of a low effective sample size

        def simulate_with_budget(theta):
            self.simulation_counter += theta.shape[0]
            return self._batched_simulator(theta)

        self._simulate_with_budget = simulate_with_budget

    def __call__(self, x_o, num_particles: int, num_initial_pop: int, num_simulations: int, epsilon_decay: float,
                 distance_based_decay: bool = False, ess_min: Optional[float] = None,
                 kernel_variance_scale: float = 1.0, use_last_pop_samples: bool = True, return_summary: bool = False,
                 kde: bool = False, kde_kwargs: Optional[Dict[str, Any]] = None, kde_sample_weights: bool = False,
                 lra: bool = False, lra_with_weights: bool = False, sass: bool = False, sass_fraction: float = 0.25,
                 sass_expansion_degree: int = 1, num_iid_samples: int = 1):
        """The last population's particles (or a KDE fitted on them, with `kde`), and with `return_summary` a dict of
        every population's `particles`, log-`weights`, `epsilons`, `distances` and `xs`."""
        pop_idx = 0
        self.num_simulations = num_simulations * num_iid_samples
        kde_kwargs = {} if kde_kwargs is None else kde_kwargs
        assert isinstance(epsilon_decay, float) and epsilon_decay > 0.0
        assert not (self.distance.requires_iid_data and lra), "Currently there is no support to run inference "
        assert not (self.distance.requires_iid_data and sass), "Currently there is no support to run inference "

        if sass:
            num_pilot_simulations = int(sass_fraction * num_simulations)
            self.logger.info("Running SASS with %s pilot samples.", num_pilot_simulations)
            sass_transform = self._run_sass_set_xo(num_particles, num_pilot_simulations, x_o, num_iid_samples, lra,
                                                   sass_expansion_degree)
            x_o = sass_transform(self.x_o)

            def sass_simulator(theta):
                self.simulation_counter += theta.shape[0]
                return sass_transform(self._batched_simulator(theta))

            self._simulate_with_budget = sass_simulator

        particles, epsilon, distances, x = self._set_xo_and_sample_initial_population(
            x_o, num_particles, num_initial_pop, num_iid_samples)
        log_weights = torch.full((num_particles,), -math.log(num_particles), device=particles.device)
        self.logger.info("population=%s, eps=%s, ess=%s, num_sims=%s", pop_idx, epsilon, 1.0, num_initial_pop)

        all_particles, all_log_weights, all_distances = [particles], [log_weights], [distances]
        all_epsilons, all_x = [epsilon], [x]

        while self.simulation_counter < self.num_simulations:
            pop_idx += 1
            if distance_based_decay:      # a quantile of the previous population's distances
                epsilon = self._get_next_epsilon(all_distances[pop_idx - 1], epsilon_decay)
            else:
                epsilon *= epsilon_decay
            self.kernel_variance = self._get_kernel_variance(
                all_particles[pop_idx - 1], torch.exp(all_log_weights[pop_idx - 1]), samples_per_dim=500,
                kernel_variance_scale=kernel_variance_scale)
            particles, log_weights, distances, x = self._sample_next_population(
                particles=all_particles[pop_idx - 1], log_weights=all_log_weights[pop_idx - 1],
                distances=all_distances[pop_idx - 1], epsilon=epsilon, x=all_x[pop_idx - 1],
                num_iid_samples=num_iid_samples, use_last_pop_samples=use_last_pop_samples)
            if ess_min is not None:
                particles, log_weights = self._resample_if_ess_too_small(particles, log_weights, ess_min, pop_idx)
            self.logger.info("population=%s done: eps=%.6f, num_sims=%s.", pop_idx, epsilon, self.simulation_counter)
            all_particles.append(particles)
            all_log_weights.append(log_weights)
            all_distances.append(distances)
            all_epsilons.append(epsilon)
            all_x.append(x)

        if lra:
            self.logger.info("Running Linear regression adjustment.")
            final_particles, _ = self._run_lra_update_weights(
                particles=all_particles[-1], xs=all_x[-1], observation=process_x(x_o),
                log_weights=all_log_weights[-1], lra_with_weights=lra_with_weights)
        else:
            final_particles = all_particles[-1]

        summary = dict(particles=all_particles, weights=all_log_weights, epsilons=all_epsilons,
                       distances=all_distances, xs=all_x)
        if kde:
            self.logger.info("KDE on %s samples with bandwidth option %s. Beware that KDE can give unreliable results "
                             "when used with too few samples and in high dimensions.", final_particles.shape[0],
                             kde_kwargs.get("bandwidth", "cv"))
            if kde_sample_weights:
                kde_kwargs["sample_weights"] = all_log_weights[-1].exp()
            kde_dist = get_kde(final_particles, **kde_kwargs)
            return (kde_dist, summary) if return_summary else kde_dist
        return (final_particles, summary) if return_summary else final_particles

    def _set_xo_and_sample_initial_population(self, x_o, num_particles: int, num_initial_pop: int,
                                              num_iid_samples: int) -> Tuple[Tensor, float, Tensor, Tensor]:
        """Particles, epsilon, distances and data of the initial population: the `num_particles` closest of
        `num_initial_pop` prior simulations; epsilon is the last accepted distance (1e8 if that is not finite)."""
        assert num_particles <= num_initial_pop, (
            "number of initial round simulations must be greater than population size")
        x_o = torch.as_tensor(x_o, dtype=torch.float32)
        assert (x_o.shape[0] == 1) or self.distance.requires_iid_data, (
            "Your data contain iid data-points, but the choice of your distance does not allow multiple conditioning "
            "observations.")
        theta = self.prior.sample((num_initial_pop,))
        x = self._simulate_with_budget(theta.repeat_interleave(num_iid_samples, dim=0))
        x = x.reshape((num_initial_pop, num_iid_samples, -1))
        if not self.distance.requires_iid_data:
            x = x.squeeze(1)
            self.x_shape = x[0].shape
        else:
            self.x_shape = x[0, 0].shape
        self.x_o = process_x(x_o, self.x_shape).to(x.device)
        assert_all_finite(self.x_o, "Observed data x_o")

        distances = self.distance(self.x_o, x)
        sortidx = torch.argsort(distances, stable=True)[:num_particles]          # (ties: simulation order)
        initial_epsilon = distances[sortidx[num_particles - 1]].item()
        if not math.isfinite(initial_epsilon):
            initial_epsilon = 1e8
        return theta[sortidx], initial_epsilon, distances[sortidx], x[sortidx]

    def _sample_next_population(self, particles: Tensor, log_weights: Tensor, distances: Tensor, epsilon: float,
                                x: Tensor, num_iid_samples: int,
                                use_last_pop_samples: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """Particles, normalised log-weights, distances and data of the next population, sorted by distance."""
        new_particles, new_log_weights, new_distances, new_x = [], [], [], []
        num_accepted_particles = 0
        num_particles = particles.shape[0]

        while num_accepted_particles < num_particles:
            # never more candidates than the budget has simulations left
            num_batch = min(num_particles - num_accepted_particles, self.num_simulations - self.simulation_counter)
            particle_candidates = self._sample_and_perturb(particles, torch.exp(log_weights), num_samples=num_batch)
            x_candidates = self._simulate_with_budget(particle_candidates.repeat_interleave(num_iid_samples, dim=0))
            x_candidates = x_candidates.reshape((num_batch, num_iid_samples, -1))
            if not self.distance.requires_iid_data:
                x_candidates = x_candidates.squeeze(1)
            dists = self.distance(self.x_o, x_candidates)
            is_accepted = dists <= epsilon
            num_accepted_batch = int(is_accepted.sum().item())
            if num_accepted_batch > 0:
                new_particles.append(particle_candidates[is_accepted])
                new_log_weights.append(
                    self._calculate_new_log_weights(particle_candidates[is_accepted], particles, log_weights))
                new_distances.append(dists[is_accepted])
                new_x.append(x_candidates[is_accepted])
                num_accepted_particles += num_accepted_batch

            if self.simulation_counter >= self.num_simulations and num_accepted_particles < num_particles:
                if use_last_pop_samples:
                    num_remaining = num_particles - num_accepted_particles
                    self.logger.info("Simulation Budget exceeded, filling up with %s samples from last population.",
                                     num_remaining)
                    # the best of the old population fill the gap; all weights are recomputed on the joint set
                    new_particles.append(particles[:num_remaining, :])
                    new_log_weights = [
                        self._calculate_new_log_weights(torch.cat(new_particles), particles, log_weights)]
                    new_distances.append(distances[:num_remaining])
                    new_x.append(x[:num_remaining])
                else:
                    self.logger.info("Simulation Budget exceeded, returning previous population.")
                    new_particles, new_log_weights, new_distances, new_x = [particles], [log_weights], [distances], [x]
                break

        new_particles, new_log_weights = torch.cat(new_particles), torch.cat(new_log_weights)
        new_distances, new_x = torch.cat(new_distances), torch.cat(new_x)
        new_log_weights = new_log_weights - torch.logsumexp(new_log_weights, dim=0)
        sort_idx = torch.argsort(new_distances, stable=True)
        return new_particles[sort_idx], new_log_weights[sort_idx], new_distances[sort_idx], new_x[sort_idx]

    def _get_next_epsilon(self, distances: Tensor, quantile: float) -> float:
        """The `quantile` of the previous population's UNIQUE distances, with their normalised cumulative sum as the
        cdf: the first distance whose "cdf" reaches the quantile (the last one if none does)."""
        distances = torch.unique(distances)
        distances_cdf = torch.cumsum(distances, dim=0) / distances.sum()
        hits = torch.where(distances_cdf >= quantile)[0]
        if hits.numel() == 0:
            self.logger.warning("Accepted unique distances=%s don't match quantile=%s. Selecting last distance.",
                                distances, quantile)
            return distances[-1].item()
        return distances[hits[0]].item()

    def kernel_log_mixture(self, new_particles: Tensor, old_particles: Tensor, old_log_weights: Tensor,
                           force_fallback: bool = False) -> Tensor:
        """log sum_j w_j K(new_i; old_j) for every new particle, K the perturbation kernel centred on old particle j:
        one `mixture_lse` call (whitened by the inverse Cholesky factor of the Gaussian kernel's covariance, or the
        box test of the uniform kernel) plus the kernel's normalising constant."""
        assert self.kernel_variance is not None, "get kernel variance first."
        D = old_particles.shape[1]
        if self.kernel == "gaussian":
            assert self.kernel_variance.ndim == 2
            chol = torch.linalg.cholesky(self.kernel_variance.double())
            whiten = torch.linalg.solve_triangular(chol, torch.eye(D, dtype=torch.float64, device=chol.device),
                                                   upper=False)
            const = -torch.log(torch.diagonal(chol)).sum() - 0.5 * D * math.log(2.0 * math.pi)      # (stays on the device)
            lse = mixture_lse(new_particles, old_particles, log_w=old_log_weights, whiten=whiten.float(),
                              scale=torch.ones(1, device=new_particles.device), force_fallback=force_fallback)[0]
        else:
            half_width = self.kernel_variance.reshape(-1).expand(D) if self.kernel_variance.numel() == 1 \
                else self.kernel_variance.reshape(D)
            const = -torch.log(2.0 * half_width.double()).sum()
            lse = mixture_lse(new_particles, old_particles, log_w=old_log_weights, half_width=half_width,
                              force_fallback=force_fallback)[0]
        return (lse.double() + const).to(torch.float32)

    def _calculate_new_log_weights(self, new_particles: Tensor, old_particles: Tensor,
                                   old_log_weights: Tensor) -> Tensor:
        """Unnormalised new log-weights of the three publications: prior density over the kernel mixture."""
        return self.prior.log_prob(new_particles) - self.kernel_log_mixture(new_particles, old_particles,
                                                                            old_log_weights)

    @staticmethod
    def sample_from_population_with_weights(particles: Tensor, weights: Tensor, num_samples: int = 1) -> Tensor:
        """`num_samples` particles drawn with replacement with probabilities proportional to the weights."""
        return particles[torch.multinomial(weights, num_samples, replacement=True)]

    def _sample_and_perturb(self, particles: Tensor, weights: Tensor, num_samples: int = 1) -> Tensor:
        """Resample from the population and perturb with the kernel; proposals outside the prior are redrawn."""
        num_accepted = 0
        parameters = []
        while num_accepted < num_samples:
            parms = self.sample_from_population_with_weights(particles, weights, num_samples=num_samples - num_accepted)
            parms_perturbed = self._perturb(parms)
            is_within_prior = within_support(self.prior, parms_perturbed)
            num_accepted += int(is_within_prior.sum().item())
            if num_accepted > 0:
                parameters.append(parms_perturbed[is_within_prior])
        return torch.cat(parameters)

    def _perturb(self, thetas: Tensor) -> Tensor:
        """One draw from the perturbation kernel around every row of `thetas`."""
        assert self.kernel_variance is not None, "get kernel variance first."
        if self.kernel == "gaussian":
            chol = torch.linalg.cholesky(self.kernel_variance)
            return thetas + torch.randn_like(thetas) @ chol.T
        return thetas + (2.0 * torch.rand_like(thetas) - 1.0) * self.kernel_variance

    def _get_kernel_variance(self, particles: Tensor, weights: Tensor, samples_per_dim: int = 100,
                             kernel_variance_scale: float = 1.0) -> Tensor:
        """The perturbation kernel's variance from a population: variant C its weighted covariance (the identity if
        that is not positive definite), variants A and B the diagonal of the ranges of a weighted resample; the
        uniform kernel's half widths are those ranges."""
        if self.kernel == "gaussian":
            if self.algorithm_variant == "C":
                population_cov = weighted_covariance(particles, weights).to(torch.float32)
                _, info = torch.linalg.cholesky_ex(kernel_variance_scale * population_cov)
                if int(info) != 0 or not bool(torch.isfinite(population_cov).all()):
                    self.logger.warning("Singular particle covariance, using unit covariance.")
                    population_cov = torch.eye(particles.shape[1], device=particles.device)
                return kernel_variance_scale * population_cov
            particle_ranges = self._get_particle_ranges(particles, weights, samples_per_dim=samples_per_dim)
            return kernel_variance_scale * torch.diag(particle_ranges)
        return kernel_variance_scale * self._get_particle_ranges(particles, weights, samples_per_dim=samples_per_dim)

    def _resample_if_ess_too_small(self, particles: Tensor, log_weights: Tensor, ess_min: float,
                                   pop_idx: int) -> Tuple[Tensor, Tensor]:
        """Resampled particles with uniform weights when the relative effective sample size (ESS / N, in (0, 1]) is
        below `ess_min` (Sisson et al. 2007); otherwise the population as it is."""
        num_particles = particles.shape[0]
        weights = torch.exp(log_weights)
        ess = float(((torch.sum(weights) ** 2) / torch.sum(weights**2)) / num_particles)
        if ess < ess_min:
            self.logger.info("ESS=%s too low, resampling pop %s...", ess, pop_idx)
            self.num_resamples += 1
            particles = self.sample_from_population_with_weights(particles, weights, num_samples=num_particles)
            log_weights = torch.full((num_particles,), -math.log(num_particles), device=particles.device)
        return particles, log_weights

    def _run_lra_update_weights(self, particles: Tensor, xs: Tensor, observation: Tensor, log_weights: Tensor,
                                lra_with_weights: bool) -> Tuple[Tensor, Tensor]:
        """Particles adjusted by the (weighted) linear regression of particles on xs, and their recomputed weights."""
        adjusted_particles = self._run_lra(theta=particles, x=xs, observation=observation,
                                           sample_weight=log_weights.exp() if lra_with_weights else None)
        adjusted_log_weights = self._calculate_new_log_weights(adjusted_particles, particles, log_weights)
        return adjusted_particles, adjusted_log_weights

    def _run_sass_set_xo(self, num_particles: int, num_pilot_simulations: int, x_o, num_iid_samples: int,
                         lra: bool = False, sass_expansion_degree: int = 1) -> Callable:
        """The summary-statistics transform from one rejection round of `num_pilot_simulations` that keeps
        `num_particles`; sets self.x_o on the way."""
        pilot_particles, _, _, pilot_xs = self._set_xo_and_sample_initial_population(
            x_o, num_particles, num_pilot_simulations, num_iid_samples)
        assert self.x_o is not None, "x_o not set yet."
        if lra:
            pilot_particles = self._run_lra(pilot_particles, pilot_xs, self.x_o)
        return self._get_sass_transform(pilot_particles, pilot_xs, expansion_degree=sass_expansion_degree,
                                        sample_weight=None)

    def _get_particle_ranges(self, particles: Tensor, weights: Tensor, samples_per_dim: int = 100) -> Tensor:
        """max - min per dimension of `samples_per_dim * D` particles resampled with their weights."""
        samples = self.sample_from_population_with_weights(particles, weights,
                                                           num_samples=samples_per_dim * particles.shape[1])
        particle_ranges = samples.max(0).values - samples.min(0).values
        assert particle_ranges.ndim < 2
        return particle_ranges
