"""Eager-torch restatement of the mixture-density-network posterior estimator, written from the formulas (DESIGN.md
section 7g), in fp32 or fp64.  Its ``state_dict`` keys are the reference's (``net._hidden_net.0.weight`` ...,
``_transform_shift``, ``_transform_scale``, ``_embedding_net.0._mean`` / ``_std``), so a reference checkpoint loads
strictly.  The tests use it as the parity oracle of the HIP kernels and check it against recorded outputs of the real
classes (tests/golden/mdn_reference.pt)."""

import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F


class _Standardize(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.register_buffer("_mean", torch.zeros(C))
        self.register_buffer("_std", torch.ones(C))

    def forward(self, t):
        return (t - self._mean) / self._std


class _Heads(nn.Module):
    def __init__(self, D, C, H, K, eps):
        super().__init__()
        self.D, self.C, self.H, self.K, self.eps = D, C, H, K, eps
        self.U = D * (D - 1) // 2
        self._hidden_net = nn.Sequential(nn.Linear(C, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU())
        self._logits_layer = nn.Linear(H, K)
        self._means_layer = nn.Linear(H, K * D)
        self._unconstrained_diagonal_layer = nn.Linear(H, K * D)
        if self.U:
            self._upper_layer = nn.Linear(H, K * self.U)
        with torch.no_grad():      # the initialisation build_mdn always asks for
            self._logits_layer.weight.normal_(0.0, eps)
            self._logits_layer.bias.normal_(0.0, eps)
            self._unconstrained_diagonal_layer.weight.normal_(0.0, eps)
            self._unconstrained_diagonal_layer.bias.fill_(math.log(math.exp(1.0 - eps) - 1.0))
            if self.U:
                self._upper_layer.weight.normal_(0.0, eps)
                self._upper_layer.bias.zero_()


class MDNOracle(nn.Module):
    def __init__(self, D, C, H=50, K=10, eps=1e-4, z_score_theta=True, z_score_x=True):
        super().__init__()
        self.net = _Heads(D, C, H, K, eps)
        self.D, self.C, self.H, self.K, self.U, self.eps = D, C, H, K, self.net.U, eps
        self.z_score_theta = z_score_theta
        if z_score_theta:
            self.register_buffer("_transform_shift", torch.zeros(D))
            self.register_buffer("_transform_scale", torch.ones(D))
        self._embedding_net = nn.Sequential(_Standardize(C), nn.Identity()) if z_score_x else nn.Identity()
        self._rows, self._cols = np.triu_indices(D, 1)

    # -- mixture parameters of condition rows (n, C): raw logits, means, upper-triangular factors
    def components(self, x):
        n, D, K = x.shape[0], self.D, self.K
        h = self.net._hidden_net(self._embedding_net(x))
        logits = self.net._logits_layer(h)
        means = self.net._means_layer(h).reshape(n, K, D)
        diag = F.softplus(self.net._unconstrained_diagonal_layer(h).reshape(n, K, D))
        A = torch.zeros(n, K, D, D, dtype=x.dtype, device=x.device)
        idx = torch.arange(D)
        A[..., idx, idx] = diag
        if self.U:
            A[..., self._rows, self._cols] = self.net._upper_layer(h).reshape(n, K, self.U)
        return logits, means, A

    def precisions(self, A):
        return A.transpose(-1, -2) @ A + self.eps * torch.eye(self.D, dtype=A.dtype, device=A.device)

    def _z(self, theta):
        return (theta - self._transform_shift) / self._transform_scale if self.z_score_theta else theta

    def _log_scale(self):
        return torch.log(self._transform_scale).sum() if self.z_score_theta else 0.0

    def log_prob(self, theta, x):
        """theta (S, B, D) or (B, D); x (B, C) or (1, C) -> (S, B) or (B,)."""
        squeeze = theta.dim() == 2
        if squeeze:
            theta = theta[None]
        logits, means, A = self.components(x)
        d = self._z(theta)[:, :, None, :] - means[None]                 # (S, B, K, D)
        y = torch.einsum("bkij,sbkj->sbki", A, d)
        quad = (y * y).sum(-1) + self.eps * (d * d).sum(-1)
        logdet = torch.log(torch.diagonal(A, dim1=-2, dim2=-1)).sum(-1)   # no epsilon here, as the reference
        log_n = -0.5 * self.D * math.log(2 * math.pi) + logdet[None] - 0.5 * quad
        lp = torch.logsumexp(torch.log_softmax(logits, -1)[None] + log_n, -1) - self._log_scale()
        return lp[0] if squeeze else lp

    def loss(self, theta, x):
        return -self.log_prob(theta, x)

    def sample_given(self, comp, zeta, x):
        """theta (n, D) for rows paired with x[i % x_rows]: component comp[i], normal draw zeta[i]."""
        n = zeta.shape[0]
        _, means, A = self.components(x)
        r = torch.arange(n, device=zeta.device) % x.shape[0]
        mu, Ak = means[r, comp], A[r, comp]
        z = mu + torch.linalg.solve_triangular(Ak, zeta[..., None], upper=True)[..., 0]
        return z * self._transform_scale + self._transform_shift if self.z_score_theta else z

    def cumulative_weights(self, x):
        logits, _, _ = self.components(x)
        return torch.cumsum(torch.softmax(logits, -1), -1)

    def set_zstats(self, zstats):
        """zstats = [shift (D) | scale (D) | mean_x (C) | std_x (C)]: the kernels' buffer."""
        D, C = self.D, self.C
        with torch.no_grad():
            if self.z_score_theta:
                self._transform_shift.copy_(zstats[:D])
                self._transform_scale.copy_(zstats[D : 2 * D])
            if not isinstance(self._embedding_net, nn.Identity):
                self._embedding_net[0]._mean.copy_(zstats[2 * D : 2 * D + C])
                self._embedding_net[0]._std.copy_(zstats[2 * D + C :])

    def param_shapes(self):
        """(reference key, shape) in the flat order of include/sbi_amd_mdn.h."""
        out = []
        for key in ("_hidden_net.0", "_hidden_net.2", "_logits_layer", "_means_layer",
                    "_unconstrained_diagonal_layer") + (("_upper_layer",) if self.U else ()):
            m = self.net.get_submodule(key)
            out += [(f"net.{key}.weight", tuple(m.weight.shape)), (f"net.{key}.bias", tuple(m.bias.shape))]
        return out

    def flat_params(self):
        sd = self.state_dict()
        return torch.cat([sd[k].reshape(-1) for k, _ in self.param_shapes()])

    def flat_grads(self):
        named = dict(self.named_parameters())
        return torch.cat([named[k].grad.reshape(-1) for k, _ in self.param_shapes()])
