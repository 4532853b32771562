"""A recording simulator for the end-to-end ABC tests (TEST INFRASTRUCTURE: only tests import this).

x = round8(theta) + table[k]: the parameters are rounded to a 1/8 grid inside the simulator, the noise table lies on that
grid and so does the observation, so every l1 / mse / squared-l2 distance is an exact fp32 number (and the square root
of one correctly rounded).  Every (theta, x) the simulator is handed is stored; a test then recomputes on the host, in
fp64, what must have been accepted.  Ranking ties are broken by simulation order on both sides (a stable sort)."""
import torch


class RecordingSimulator:
    def __init__(self, dim: int = 2, table_rows: int = 4099, seed: int = 5, noise: float = 0.5):
        g = torch.Generator().manual_seed(seed)
        self.table = torch.round(noise * torch.randn(table_rows, dim, generator=g) * 8) / 8
        self.k = 0
        self.thetas, self.xs = [], []

    def __call__(self, theta: torch.Tensor) -> torch.Tensor:
        n = theta.shape[0]
        rows = (self.k + torch.arange(n)) % self.table.shape[0]
        self.k += n
        x = torch.round(theta * 8) / 8 + self.table[rows].to(theta.device)
        self.thetas.append(theta.detach().cpu())
        self.xs.append(x.detach().cpu())
        return x

    def recorded(self):
        return torch.cat(self.thetas), torch.cat(self.xs)


def exact_distances(x_o: torch.Tensor, x: torch.Tensor, name: str) -> torch.Tensor:
    """The distance in fp64 from grid data: exact for l1 and mse, the fp64 square root of an exact number for l2."""
    d = (x.double() - x_o.double().reshape(1, -1))
    if name == "l1":
        return d.abs().mean(-1)
    if name == "mse":
        return (d**2).mean(-1)
    return (d**2).sum(-1).sqrt()
