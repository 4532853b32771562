#!/usr/bin/env python
"""Generate tests/golden/npse_iid_reference.pt from the REAL sbi classes (build container only): the iid score functions
`FactorizedNPEScoreFunction`, `GaussCorrectedScoreFn`, `AutoGaussCorrectedScoreFn`
(sbi/inference/potentials/vector_field_adaptor.py) on VE / VP score estimators built by `build_vector_field_estimator`,
and the real `Diffuser` (sbi/samplers/score/diffuser.py) driven by an iid potential stub.

Per case (sde in ve / vp, prior = MultivariateNormal with a non-diagonal covariance / Independent(Normal); net H = 48,
L = 2, D = 3, C = 4, N = 5 observations) and per method: the composed score at t in {t_min, 0.05, 0.5, t_max} for 7
inputs in fp32 and fp64, the per-observation scores in fp64, and one 20-step Euler-Maruyama run of 32 rows with the
normal draws recorded, in both precisions (fnpe's 1 / sqrt(N) initial scale comes from the reference's own
`Diffuser.initialize`).  Also, in fp64 only, the composed score of gauss with `enable_lam_psd=True` (scale 0.5) and of
auto_gauss with diagonal precisions (`precision_est_only_diag`): sbi's element-wise PSD branch under the diagonal prior.

auto_gauss: `estimate_posterior_precision` is replaced by recorded dense precisions (its own sampler cannot run under
the zuko stub); they are chosen so that `ensure_lam_positive_definite` fires at t_max and not at t_min (asserted)."""

import os
import sys

import torch

N_OBS, N_IN, EM_STEPS, EM_ROWS = 5, 7, 20, 32
METHODS = ("fnpe", "gauss", "auto_gauss")


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden  # third-party stubs + the reference tree on sys.path

    for mod in ["matplotlib", "matplotlib.pyplot", "matplotlib.axes", "matplotlib.figure", "joblib", "tqdm", "tqdm.auto"]:
        try:
            __import__(mod)
        except Exception:
            make_golden.stub(mod)
    from sbi.inference.potentials import vector_field_adaptor as A
    from sbi.neural_nets.net_builders.vector_field_nets import build_vector_field_estimator
    from sbi.samplers.score.diffuser import Diffuser
    from torch.distributions import Independent, MultivariateNormal, Normal

    D, C = 3, 4
    small = dict(hidden_features=48, num_layers=2)

    class fp64:
        def __init__(self, est):
            self.est = est

        def __enter__(self):
            self.est.double()
            torch.set_default_dtype(torch.float64)

        def __exit__(self, *exc):
            torch.set_default_dtype(torch.float32)
            self.est.float()

    def make_prior(kind, spec, dt):
        if kind == "mvn":
            return MultivariateNormal(spec["loc"].to(dt), covariance_matrix=spec["cov"].to(dt))
        return Independent(Normal(spec["loc"].to(dt), spec["scale"].to(dt)), 1)

    def iid_fn(method, est, prior, prec, dt, **kw):
        cls = A.get_iid_method(method)
        if method == "gauss":
            # `estimate_prior_precision` is lru_cached on the prior OBJECT: a float64 prior allocated where a collected
            # float32 one lived would be handed the float32 precision
            cls.__dict__["estimate_prior_precision"].__func__.cache_clear()
        if method == "auto_gauss":
            cls.estimate_posterior_precision = classmethod(lambda c, *a, **k: prec[None].to(dt))
        return cls(est, prior, **kw)

    def run_em(method, est, prior, prec, xs, ts, dt, draws):
        fn = iid_fn(method, est, prior, prec, dt)

        class Potential:      # what Diffuser / EulerMaruyama read of a VectorFieldBasedPotential with iid observations
            vector_field_estimator = est
            device = "cpu"
            x_is_iid = True
            iid_method = method
            x_o = xs

            def gradient(self, theta, time=None, track_gradients=False):
                return fn(theta, xs, time)

        log, it = [], iter(draws or [])
        real_randn, real_like = torch.randn, torch.randn_like

        def randn(*shape, **kw):
            if draws is None:
                out = real_randn(*shape, **{k: v for k, v in kw.items() if k != "device"})
                log.append(out.clone())
                return out
            return next(it).to(dt)

        def randn_like(t, **kw):
            if draws is None:
                out = real_like(t)
                log.append(out.clone())
                return out
            return next(it).to(t.dtype)

        torch.randn, torch.randn_like = randn, randn_like
        try:
            out = Diffuser(Potential(), predictor="euler_maruyama").run(EM_ROWS, ts, show_progress_bars=False)
        finally:
            torch.randn, torch.randn_like = real_randn, real_like
        return out.reshape(EM_ROWS, D), log

    cases = {}
    for sde in ("ve", "vp"):
        torch.manual_seed(7)
        theta = torch.randn(300, D) * torch.linspace(0.5, 2.0, D) + torch.linspace(-1.0, 1.0, D)
        x = theta[:, :1] * torch.ones(1, C) + torch.randn(300, C) * 0.3 + 1.5
        est = build_vector_field_estimator(theta, x, estimator_type="score", sde_type=sde, **small)
        with torch.no_grad():
            for p in est.parameters():
                p.add_(0.05 * torch.randn_like(p))
        state = {k: v.clone() for k, v in est.state_dict().items()}
        for kind in ("mvn", "indep"):
            torch.manual_seed(13)
            B = torch.randn(D, D) * 0.5
            spec = dict(loc=torch.linspace(-0.5, 0.7, D), cov=B @ B.T + torch.eye(D), scale=torch.linspace(0.8, 1.6, D))
            xs = x[100 : 100 + N_OBS].clone()
            # dense recorded precisions of auto_gauss: weak in one direction, so that (1 - N) P0 + sum_i P_i is
            # indefinite once m^2 / s^2 is small (t_max) and positive definite at t_min
            Q, _ = torch.linalg.qr(torch.randn(D, D))
            prec = torch.stack([(Q * torch.tensor([0.05, 1.5, 3.0]) * (1 + 0.2 * i)) @ Q.T + 0.02 * (i + 1) * torch.eye(D)
                                for i in range(N_OBS)])
            prec = 0.5 * (prec + prec.transpose(1, 2))
            tq = torch.tensor([est.t_min, 0.05, 0.5, est.t_max])
            theta_q = torch.randn(N_IN, 1, D) * 1.5
            g = dict(D=D, C=C, sde=sde, kw=small, weight="max_likelihood", state=state, theta=theta[:64].clone(),
                     x=x[:64].clone(), prior_kind=kind, prior=spec, xs=xs, tq=tq, theta_q=theta_q.reshape(N_IN, D),
                     prec=prec.double(), N=N_OBS, t_min=est.t_min, t_max=est.t_max, methods={})
            # the PSD correction must fire at t_max and stay off at t_min
            with torch.no_grad(), fp64(est):
                p64 = make_prior(kind, spec, torch.float64)
                sig0 = p64.covariance_matrix if kind == "mvn" else torch.diag(p64.base_dist.scale**2)
                for t, want_negative in ((est.t_min, False), (est.t_max, True)):
                    tt = torch.tensor([t], dtype=torch.float64)
                    c = float((est.mean_t_fn(tt) ** 2 / est.std_fn(tt) ** 2).reshape(-1)[0])
                    lam_unc = (1 - N_OBS) * (torch.linalg.inv(sig0) + c * torch.eye(D)) + N_OBS * c * torch.eye(D) + \
                        prec.double().sum(0)
                    ev = torch.linalg.eigvalsh(lam_unc)
                    print(sde, kind, "t", t, "eigenvalues of the uncorrected Lam", ev.tolist())
                    assert (ev.min() < 0) == want_negative, (t, ev)
            for method in METHODS:
                rec = {}
                with torch.no_grad():
                    fn = iid_fn(method, est, make_prior(kind, spec, torch.float32), prec, torch.float32)
                    rec["score"] = torch.stack([fn(theta_q, xs, t.reshape(1)).reshape(N_IN, D) for t in tq])
                with torch.no_grad(), fp64(est):
                    p64 = make_prior(kind, spec, torch.float64)
                    fn = iid_fn(method, est, p64, prec, torch.float64)
                    rec["score64"] = torch.stack([fn(theta_q.double(), xs.double(), t.double().reshape(1)).reshape(N_IN, D)
                                                  for t in tq])
                    rec["s64"] = torch.stack([est.score(theta_q.double(), xs.double(), t.double().reshape(1))
                                              for t in tq])          # (4, 7, N, D)
                    assert rec["s64"].shape == (4, N_IN, N_OBS, D), rec["s64"].shape
                with torch.no_grad():
                    ts = est.solve_schedule(EM_STEPS + 1)
                    torch.manual_seed(23)
                    out32, draws = run_em(method, est, make_prior(kind, spec, torch.float32), prec, xs, ts,
                                          torch.float32, None)
                    with fp64(est):
                        out64, _ = run_em(method, est, make_prior(kind, spec, torch.float64), prec, xs.double(),
                                          ts.double(), torch.float64, draws)
                    rec["em"] = dict(ts=ts, noise=torch.stack([d.reshape(EM_ROWS, D) for d in draws]), out=out32,
                                     out64=out64)
                assert len(draws) == EM_STEPS + 1
                print(sde, kind, method, "score fp32 vs fp64", float((rec["score"].double() - rec["score64"]).abs().max()),
                      "of", float(rec["score64"].abs().max()), "| EM fp32 vs fp64",
                      float((out32.double() - out64).abs().max()), "of", float(out64.abs().max()))
                g["methods"][method] = rec
            # the diagonal branches: gauss with the PSD fix on (scale 0.5, so that it fires) and diagonal estimated
            # precisions; under Independent(Normal) both take the element-wise correction, under the dense prior eigh
            diag_prec = torch.diagonal(prec, dim1=1, dim2=2).contiguous() * 0.3
            g["diag_prec"] = diag_prec.double()
            with torch.no_grad(), fp64(est):
                p64 = make_prior(kind, spec, torch.float64)
                for tag, method, pr, kw in (("gauss_psd", "gauss", prec, dict(enable_lam_psd=True, scale_from_prior_precision=0.5)),
                                            ("auto_gauss_diag", "auto_gauss", diag_prec, dict(precision_est_only_diag=True))):
                    fn = iid_fn(method, est, p64, pr, torch.float64, **kw)
                    g[tag + "_score64"] = torch.stack([fn(theta_q.double(), xs.double(), t.double().reshape(1))
                                                       .reshape(N_IN, D) for t in tq])
            cases[f"{sde}_{kind}"] = g
    path = os.path.join(make_golden.OUT, "npse_iid_reference.pt")
    torch.save(cases, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
