"""Eager-torch restatement (fp32 or fp64) of sbi's mixed neural likelihood estimator for x = [one continuous column, V
categorical columns] -- TEST INFRASTRUCTURE, never the product path.

  * ``ResidualMADE``: nflows' ``MADE(use_residual_blocks=True, random_mask=False, activation=relu)`` built from the
    ``MaskedLinear`` of oracle/maf_oracle.py (its degree and mask rules).  PARITY UNPINNED at the nflows boundary
    (nflows is not importable here); recalled: ``h = initial(x); h += relu(context_layer(c))``; per block
    ``t = L1(relu(L0(relu(h)))); t = glu(cat(t, block.context_layer(c)))``; ``h = h + t``; ``final(h)`` with no
    activation in front; every block's L1 initialised uniform(-1e-3, 1e-3).
  * ``CategoricalMADE``: sbi's class (estimators/categorical_net.py) on ``MADEWrapper`` (utils/nn_utils.py): a zero
    dummy input in front, the dummy's outputs dropped, logits beyond num_categories[v] set to -inf, the input mapped
    from raw values to indices by searchsorted in the sorted training values.
  * ``MixedOracle``: sbi's ``MixedDensityEstimator`` with ``NSFOracle`` (oracle/nsf_oracle.py, D = 1: context-only
    spline conditioner) behind the trainable combined embedding ``Linear, ReLU, Linear, ReLU``.

``state_dict()`` keys are the reference's (the theta standardisation is registered once, under
``condition_embedding.0``; the reference registers the same module a second time inside the categorical net)."""

import math

import torch
from torch import nn
from torch.nn import functional as F

from oracle.maf_oracle import MaskedLinear, _get_input_degrees
from oracle.nsf_oracle import NSFOracle, Standardize


class MaskedResidualBlock(nn.Module):
    def __init__(self, in_degrees, autoregressive_features, context_features):
        super().__init__()
        features = len(in_degrees)
        self.context_layer = nn.Linear(context_features, features)
        l0 = MaskedLinear(in_degrees, features, autoregressive_features, is_output=False)
        l1 = MaskedLinear(l0.degrees, features, autoregressive_features, is_output=False)
        self.linear_layers = nn.ModuleList([l0, l1])
        self.degrees = l1.degrees
        nn.init.uniform_(l1.weight, -1e-3, 1e-3)
        nn.init.uniform_(l1.bias, -1e-3, 1e-3)

    def forward(self, inputs, context):
        t = self.linear_layers[0](F.relu(inputs))
        t = self.linear_layers[1](F.relu(t))
        t = F.glu(torch.cat((t, self.context_layer(context)), dim=1), dim=1)
        return inputs + t


class ResidualMADE(nn.Module):
    def __init__(self, features, hidden_features, context_features, num_blocks, output_multiplier):
        super().__init__()
        self.initial_layer = MaskedLinear(_get_input_degrees(features), hidden_features, features, is_output=False)
        self.context_layer = nn.Linear(context_features, hidden_features)
        blocks, prev = [], self.initial_layer.degrees
        for _ in range(num_blocks):
            blocks.append(MaskedResidualBlock(prev, features, context_features))
            prev = blocks[-1].degrees
        self.blocks = nn.ModuleList(blocks)
        self.final_layer = MaskedLinear(prev, features * output_multiplier, features, is_output=True)

    def forward(self, inputs, context):
        h = self.initial_layer(inputs)
        h = h + F.relu(self.context_layer(context))
        for block in self.blocks:
            h = block(h, context)
        return self.final_layer(h)


class CategoricalMADE(ResidualMADE):
    def __init__(self, num_categories, categorical_values, hidden_features, context_features, num_blocks=2):
        self.num_variables = len(num_categories)
        self.max_num_categories = int(max(num_categories))
        super().__init__(self.num_variables + 1, hidden_features, context_features, num_blocks,
                         self.max_num_categories)
        self.num_categories = [int(c) for c in num_categories]
        mask = torch.zeros(self.num_variables, self.max_num_categories)
        lookup = torch.zeros(self.num_variables, self.max_num_categories)
        for i, c in enumerate(self.num_categories):
            mask[i, :c] = 1
            lookup[i, :c] = torch.sort(torch.as_tensor(categorical_values[i], dtype=torch.float32)).values
        self.register_buffer("mask", mask)
        self.register_buffer("values_lookup", lookup)

    def map_values_to_indices(self, values):
        mapped = values.clone()
        for i, c in enumerate(self.num_categories):
            uniq = self.values_lookup[i, :c].contiguous()
            col = values[..., i].contiguous()
            idx = torch.searchsorted(uniq, col)
            clamped = idx.clamp(0, c - 1)
            if not (idx == clamped).all():
                bad = idx != clamped
                raise ValueError(f"Variable {i} contains values not seen during training: "
                                 f"{col[bad].unique().tolist()}. Valid values are: {uniq.tolist()}")
            mapped[..., i] = idx
        return mapped

    def map_indices_to_values(self, indices):
        return torch.gather(self.values_lookup, 1, indices.long().t()).t()

    def logits(self, idx, context):
        """(n, V, Kmax) from category INDICES (n, V) (as floats) and the standardised context."""
        dummy = torch.zeros(idx.shape[:-1] + (1,), dtype=context.dtype)
        out = ResidualMADE.forward(self, torch.cat((dummy, idx.to(context.dtype)), -1), context)
        out = out[..., self.max_num_categories:]
        out = out.masked_fill(~self.mask.bool().flatten(), float("-inf"))
        return out.reshape(idx.shape[0], self.num_variables, self.max_num_categories)

    def log_prob_idx(self, idx, context):
        lg = torch.log_softmax(self.logits(idx, context), -1)
        return torch.gather(lg, 2, idx.long()[..., None])[..., 0].sum(-1)


class _Net(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net


class MixedOracle(nn.Module):
    def __init__(self, num_categories, categorical_values, C, discrete_hidden=50, discrete_blocks=2, embedding=50,
                 hidden=50, num_bins=10, num_transforms=5, context_layers=1, tail_bound=10.0, log_transform=False):
        super().__init__()
        V = len(num_categories)
        self.V, self.C, self.log_transform = V, C, log_transform
        self.L, self.T, self.NB = context_layers, num_transforms, discrete_blocks
        self.discrete_net = _Net(CategoricalMADE(num_categories, categorical_values, discrete_hidden, C,
                                                 discrete_blocks))
        flow = NSFOracle(torch.randn(8, 1), torch.zeros(8, embedding), z_score_theta="independent", z_score_x="none",
                         hidden_features=hidden, num_transforms=num_transforms, num_bins=num_bins,
                         tail_bound=tail_bound, hidden_layers_spline_context=context_layers)
        flow.net._embedding_net = nn.Sequential(nn.Linear(V + C, embedding), nn.ReLU(),
                                                nn.Linear(embedding, embedding), nn.ReLU())
        self.continuous_net = flow
        self.condition_embedding = nn.Sequential(Standardize(torch.zeros(C), torch.ones(C)), nn.Identity())

    # -- the kernels' buffers
    def set_zstats(self, zstats):
        C = self.C
        aff = self.continuous_net.net._transform._transforms[0]
        with torch.no_grad():
            aff._shift.copy_(zstats[0:1])
            aff._scale.copy_(zstats[1:2])
            self.condition_embedding[0]._mean.copy_(zstats[2: 2 + C])
            self.condition_embedding[0]._std.copy_(zstats[2 + C: 2 + 2 * C])

    def param_keys(self):
        """Reference keys in the flat order of include/sbi_amd_mnle.h."""
        d, c = "discrete_net.net.", "continuous_net.net."
        keys = [d + "initial_layer", d + "context_layer"]
        for b in range(self.NB):
            keys += [d + f"blocks.{b}.linear_layers.0", d + f"blocks.{b}.linear_layers.1",
                     d + f"blocks.{b}.context_layer"]
        keys += [d + "final_layer", c + "_embedding_net.0", c + "_embedding_net.2"]
        for t in range(self.T):
            p = c + f"_transform._transforms.{t + 1}.transform_net.spline_predictor."
            keys += [p + "0"] + ([p + "2"] if self.L > 0 else []) + [p + str(2 + 2 * self.L)]
        return [k + s for k in keys for s in (".weight", ".bias")]

    def flat_params(self):
        sd = self.state_dict()
        return torch.cat([sd[k].reshape(-1) for k in self.param_keys()])

    def flat_grads(self):
        named = dict(self.named_parameters())
        return torch.cat([named[k].grad.reshape(-1) for k in self.param_keys()])

    def flat_mask(self):
        """0/1 mask of the flat buffer (MADE masks; 1 elsewhere)."""
        sd = self.state_dict()
        out = []
        for k in self.param_keys():
            mk = k[: -len("weight")] + "mask" if k.endswith(".weight") else None
            out.append((sd[mk] if mk in sd else torch.ones_like(sd[k])).reshape(-1).float())
        return torch.cat(out)

    # -- densities of paired rows: x (n, 1 + V) raw values, theta (n, C)
    def parts(self, x, theta):
        cz = self.condition_embedding(theta)
        vals = x[:, 1:]
        idx = self.discrete_net.net.map_values_to_indices(vals)
        lp_d = self.discrete_net.net.log_prob_idx(idx, cz)
        xc = x[:, :1]
        xl = torch.log(xc) if self.log_transform else xc
        lp_c = self.continuous_net.net.log_prob(xl, torch.cat((vals, cz), -1))
        if self.log_transform:
            lp_c = lp_c - xl[:, 0]
        return lp_d, lp_c

    def log_prob(self, x, theta):
        lp_d, lp_c = self.parts(x, theta)
        return lp_d + lp_c

    def loss(self, x, theta):
        return -self.log_prob(x, theta)

    def logits(self, x, theta):
        idx = self.discrete_net.net.map_values_to_indices(x[:, 1:])
        return self.discrete_net.net.logits(idx, self.condition_embedding(theta))

    def sample_given(self, u, noise, theta):
        """Inverse-CDF categorical draws (first k with cumulative softmax >= u) and the inverse flow for `noise`.
        Returns (indices (n, V), x (n, 1 + V), distance of u to the nearest cumulative boundary (n,))."""
        made = self.discrete_net.net
        cz = self.condition_embedding(theta)
        n = u.shape[0]
        idx = torch.zeros(n, self.V, dtype=cz.dtype)
        gap = torch.full((n,), float("inf"), dtype=cz.dtype)
        for v in range(self.V):
            c = made.num_categories[v]
            cum = torch.cumsum(torch.softmax(made.logits(idx, cz)[:, v, :c], -1), -1)
            pick = (cum < u[:, v: v + 1].to(cz.dtype)).sum(-1).clamp(max=c - 1)
            gap = torch.minimum(gap, (cum[:, : c - 1] - u[:, v: v + 1]).abs().min(-1).values if c > 1 else gap)
            idx[:, v] = pick.to(cz.dtype)
        vals = made.map_indices_to_values(idx).to(cz.dtype)
        z, _ = self.continuous_net.net.inverse_from_noise(noise[:, None].to(cz.dtype), torch.cat((vals, cz), -1))
        xc = z.exp() if self.log_transform else z
        return idx.long(), torch.cat((xc, vals), -1), gap


# ------------------------------------------------------------------ the end-to-end toy task (analytic likelihood)
def toy_simulator(theta, g=None):
    """choice ~ Bernoulli(sigmoid(2 theta_1)), rt = exp(0.5 theta_2 + 0.3 (2c - 1) + 0.25 eps); x = [rt, choice]."""
    c = (torch.rand(theta.shape[0], generator=g) < torch.sigmoid(2 * theta[:, 0])).float()
    rt = torch.exp(0.5 * theta[:, 1] + 0.3 * (2 * c - 1) + 0.25 * torch.randn(theta.shape[0], generator=g))
    return torch.stack([rt, c], 1)


def toy_log_likelihood(theta, x):
    c, rt = x[:, 1], x[:, 0]
    p = torch.sigmoid(2 * theta[:, 0])
    lp_c = torch.where(c > 0.5, torch.log(p), torch.log1p(-p))
    mu = 0.5 * theta[:, 1] + 0.3 * (2 * c - 1)
    lp_rt = -0.5 * ((torch.log(rt) - mu) / 0.25) ** 2 - math.log(0.25 * math.sqrt(2 * math.pi)) - torch.log(rt)
    return lp_c + lp_rt


def toy_sets():
    g = torch.Generator().manual_seed(2024)
    lo, hi = torch.tensor([-2.0, -1.0]), torch.tensor([2.0, 1.0])
    theta = lo + (hi - lo) * torch.rand(2000, 2, generator=g)
    x = toy_simulator(theta, g)
    theta_t = lo + (hi - lo) * torch.rand(1000, 2, generator=g)
    x_t = toy_simulator(theta_t, g)
    return theta, x, theta_t, x_t
