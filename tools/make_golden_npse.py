#!/usr/bin/env python
"""Generate tests/golden/npse_reference.pt and npse_reference_default.pt from the REAL sbi classes (build container
only): `build_vector_field_estimator(..., estimator_type="score")` -> VE / VP / SubVP score estimators on VectorFieldMLP
(sbi/neural_nets/estimators/score_estimator.py, net_builders/vector_field_nets.py:136-339) and the real `Diffuser` with
its Euler-Maruyama predictor (sbi/samplers/score/diffuser.py, predictors.py).

Per case: the state_dict (all parameters perturbed so the zero-initialised output layer is exercised), inputs, `times`
(uniform draws with one row pinned to t_min and one to t_max, so rows fall on both sides of the control variate's 0.3
threshold) and the `eps` the loss drew; per-row losses in fp32 and from `est.double()`, with and without the control
variate; d mean-loss / d parameters from `est.double()` next to the fp32 run's own distance from it (the yardstick the
kernels are held to: the loss cancels catastrophically in fp32 at small std); `forward()` and `ode_fn()` at a few
(theta_t, t) including t_min and t_max in both precisions; the schedule functions on a grid; one 50-step
Euler-Maruyama run of 32 rows with the normal draws recorded, in both precisions.

Two files because a committed file may not exceed 1 MiB: the default-size net's state and fp64 gradient fill one alone
(its fp32 gradient is kept as per-block distances from the fp64 one, not as a tensor)."""

import os
import sys

import torch


def record_run(est, x_o, ts, n, draws=None):
    """One `Diffuser.run` on the real classes.  draws None: record every normal draw; else replay them."""
    from sbi.samplers.score.diffuser import Diffuser

    class Potential:      # what Diffuser / EulerMaruyama read of a VectorFieldBasedPotential for one observation
        vector_field_estimator = est
        device = "cpu"
        x_is_iid = False
        iid_method = None

        def __init__(self):
            self.x_o = x_o

        def gradient(self, theta, time=None, track_gradients=False):
            return est.score(input=theta, condition=self.x_o, t=time)

    log, it = [], iter(draws or [])
    real_randn, real_like = torch.randn, torch.randn_like

    def randn(*shape, **kw):
        if draws is None:
            out = real_randn(*shape, **{k: v for k, v in kw.items() if k != "device"})
            log.append(out.clone())
            return out
        return next(it).to(x_o.dtype)

    def randn_like(t, **kw):
        if draws is None:
            out = real_like(t)
            log.append(out.clone())
            return out
        return next(it).to(t.dtype)

    torch.randn, torch.randn_like = randn, randn_like
    try:
        out = Diffuser(Potential(), predictor="euler_maruyama").run(n, ts, show_progress_bars=False)
    finally:
        torch.randn, torch.randn_like = real_randn, real_like
    return out, log


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # third-party stubs + the reference tree on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib", "tqdm", "tqdm.auto"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.neural_nets.net_builders.vector_field_nets import build_vector_field_estimator

    small = dict(hidden_features=48, num_layers=2)
    specs = {
        "ve_default_D5_C3": (5, 3, "ve", {}, "max_likelihood"),
        "vp_H48_L2_D3_C4": (3, 4, "vp", small, "max_likelihood"),
        "subvp_H48_L2_D3_C4": (3, 4, "subvp", small, "max_likelihood"),
        "ve_variance_H48_L2_D3_C4": (3, 4, "ve", small, "variance"),
    }
    files = {"npse_reference_default.pt": {}, "npse_reference.pt": {}}

    class fp64:      # est.double() plus float64 as the default dtype: the time embedding allocates with the default
        def __init__(self, est):
            self.est = est

        def __enter__(self):
            self.est.double()
            torch.set_default_dtype(torch.float64)

        def __exit__(self, *exc):
            torch.set_default_dtype(torch.float32)
            self.est.float()

    for name, (D, C, sde, kw, weight) in specs.items():
        torch.manual_seed(7)
        theta = torch.randn(300, D) * torch.linspace(0.5, 3.0, D) + torch.linspace(-2.0, 2.0, D)
        x = theta[:, :1] * torch.ones(1, C) + torch.randn(300, C) * 0.3 + 1.5
        est = build_vector_field_estimator(theta, x, estimator_type="score", sde_type=sde, **kw)
        est._set_weight_fn(weight)
        with torch.no_grad():
            for p in est.parameters():
                p.add_(0.05 * torch.randn_like(p))
        n = 64
        times = torch.rand(n) * (est.t_max - est.t_min) + est.t_min
        times[0], times[1] = est.t_min, est.t_max
        torch.manual_seed(11)
        eps = torch.randn_like(theta[:n])
        state = {k: v.clone() for k, v in est.state_dict().items()}
        default = name == "ve_default_D5_C3"
        g = dict(D=D, C=C, sde=sde, kw=kw, weight=weight, state=state, theta=theta[:n].clone(), x=x[:n].clone(),
                 times=times, eps=eps, t_min=est.t_min, t_max=est.t_max)

        def run_loss(e, dt, cv):
            # the loss draws eps = randn_like(input) as its only random call: hand it the recorded draw (float64 draws
            # of the same seed are different numbers)
            real_like = torch.randn_like
            torch.randn_like = lambda t, **k: eps.to(t.dtype)
            try:
                e.zero_grad()
                losses = e.loss(theta[:n].to(dt), x[:n].to(dt), times=times.to(dt), control_variate=cv)
            finally:
                torch.randn_like = real_like
            if losses.dim() == 2:
                # weight_fn="variance" returns std_fn(times)**2 with a trailing unit axis, so the reference's
                # `weights * loss` is the (N, N) outer product; row i's own weighted loss is its diagonal
                losses = losses.diagonal()
            losses.mean().backward()
            return losses.detach().clone(), {k: p.grad.clone() for k, p in e.named_parameters()}

        for cv in (True, False):
            tag = "" if cv else "_nocv"
            l32, g32 = run_loss(est, torch.float32, cv)
            with fp64(est):
                l64, g64 = run_loss(est, torch.float64, cv)
            g["losses" + tag], g["losses64" + tag] = l32, l64
            if cv or sde == "vp":
                g["grads64" + tag] = g64
                g["grads32_err" + tag] = {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}
                if not default:
                    g["grads" + tag] = g32
            print(name, "cv" if cv else "nocv", "loss", l32[:3].tolist(), "fp32 loss err",
                  float((l32.double() - l64).abs().max()), "of", float(l64.abs().max()), "rows under 0.3:",
                  int((est.std_fn(times).reshape(-1) < 0.3).sum()))

        tq = torch.tensor([est.t_min, 0.05, 0.3, 0.5, 0.77, est.t_max]).repeat_interleave(4)
        theta_q = torch.randn(tq.shape[0], D) * 1.5
        with torch.no_grad():
            g.update(tq=tq, theta_q=theta_q, score=est(theta_q, x[:1], tq), ode=est.ode_fn(theta_q, x[:1], tq))
        with torch.no_grad(), fp64(est):
            g.update(score64=est(theta_q.double(), x[:1].double(), tq.double()),
                     ode64=est.ode_fn(theta_q.double(), x[:1].double(), tq.double()))
            grid = torch.linspace(est.t_min, est.t_max, 17, dtype=torch.float64)
            ones = torch.ones(1, D, dtype=torch.float64)
            g["schedule"] = dict(
                t=grid, mean_t=est.mean_t_fn(grid).reshape(-1), std=est.std_fn(grid).reshape(-1),
                drift=torch.stack([torch.broadcast_to(est.drift_fn(ones, t.reshape(1)), (1, D))[0] for t in grid]),
                diffusion=est.diffusion_fn(ones, grid).reshape(-1), solve=est.solve_schedule(9).double(),
                w_identity=torch.ones_like(grid), w_max_likelihood=est._max_likelihood_weight_fn(grid).reshape(-1),
                w_variance=est._variance_weight_fn(grid).reshape(-1),
                mean_base=est.mean_base.clone(), std_base=est.std_base.clone())
        with torch.no_grad():
            # one Euler-Maruyama run of the real Diffuser: 50 steps, 32 rows, the draws recorded and replayed in fp64
            ts = est.solve_schedule(51)
            torch.manual_seed(23)
            out32, draws = record_run(est, x[:1], ts, 32)
            with fp64(est):
                out64, _ = record_run(est, x[:1].double(), ts.double(), 32, draws)
            g["em"] = dict(ts=ts, noise=torch.stack([d.reshape(32, D) for d in draws]), out=out32.reshape(32, D),
                            out64=out64.reshape(32, D))
            print(name, "EM fp32 vs fp64", float((out32.double() - out64).abs().max()), "max", float(out64.abs().max()))
        files["npse_reference_default.pt" if default else "npse_reference.pt"][name] = g
    for fn, cases in files.items():
        path = os.path.join(make_golden.OUT, fn)
        torch.save(cases, path)
        print(fn, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
