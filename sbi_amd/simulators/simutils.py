"""Batched simulation for the ABC samplers (sbi/simulators/simutils.py `simulate_in_batches`), in one process."""

from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import Tensor


def simulate_in_batches(simulator: Callable[[Tensor], Tensor], theta: Tensor, sim_batch_size: Optional[int] = 1,
                        num_workers: int = 1, seed: Optional[int] = None, show_progress_bars: bool = True) -> Tensor:
    """Simulations x for the parameters theta, `sim_batch_size` rows per simulator call (None: all at once).

    `num_workers != 1` is refused: worker processes forked from a process that holds the GPU are not something this
    package starts.  Parallelise inside the simulator instead."""
    if num_workers != 1:
        raise NotImplementedError("sbi_amd: simulate_in_batches runs in one process (num_workers=1): worker processes "
                                  "forked from a process that holds the GPU are not started here.")
    if seed is not None:
        torch.manual_seed(seed)
    num_sims = theta.shape[0]
    if num_sims == 0:
        return torch.tensor([])
    if sim_batch_size is None or sim_batch_size >= num_sims:
        return simulator(theta)
    batches = torch.split(theta, sim_batch_size, dim=0)
    bar = None
    if show_progress_bars:
        try:
            from tqdm.auto import tqdm

            bar = tqdm(total=num_sims, desc=f"Running {num_sims} simulations.")
        except ImportError:
            bar = None
    outputs = []
    for batch in batches:
        outputs.append(simulator(batch))
        if bar is not None:
            bar.update(batch.shape[0])
    if bar is not None:
        bar.close()
    return torch.cat(outputs, dim=0)
