"""Host-side pieces of the NPSE path that need no GPU: schedule functions against outputs of the real sbi classes
(tests/golden/npse_reference*.pt), parameter layout and state-dict exchange, refusals, the trainer's constructor rules
and loop bookkeeping, pickling -- and the CPU restatement tests/npse_oracle.py against the same fixture (in fp64 it must
reproduce the fp64 records to 1e-9, which is what makes it a yardstick for shapes the fixture does not hold)."""

import os
import pickle
import re
import warnings

import pytest
import torch

from tests.npse_oracle import NPSEOracle, flat_grad, oracle_score_build_fn

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["ve_default_D5_C3", "vp_H48_L2_D3_C4", "subvp_H48_L2_D3_C4", "ve_variance_H48_L2_D3_C4"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_case(name):
    fn = "npse_reference_default.pt" if name == "ve_default_D5_C3" else "npse_reference.pt"
    return torch.load(os.path.join(GOLD_DIR, fn), weights_only=False)[name]


def estimator_of(g):
    from sbi_amd.neural_nets import build_score_matching_estimator

    kw = g["kw"]
    est = build_score_matching_estimator(g["theta"], g["x"], sde_type=g["sde"], weight_fn=g["weight"],
                                         hidden_features=kw.get("hidden_features", 100),
                                         num_layers=kw.get("num_layers", 5))
    est.load_reference_state_dict(g["state"])
    return est


def oracle_of(g, double=False):
    kw = g["kw"]
    o = NPSEOracle(g["D"], g["C"], sde=g["sde"], H=kw.get("hidden_features", 100), L=kw.get("num_layers", 5),
                   weight=g["weight"])
    if double:
        o = o.double()
    o.load_reference_state_dict(g["state"])
    return o


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", CASES)
def test_schedule_functions_match_the_reference(name):
    g = load_case(name)
    est, s = estimator_of(g), g["schedule"]
    t = s["t"]
    ones = torch.ones(1, g["D"], dtype=torch.float64)
    assert type(est).__name__ == {"ve": "VEScoreEstimator", "vp": "VPScoreEstimator", "subvp": "SubVPScoreEstimator"}[g["sde"]]
    assert est.t_min == pytest.approx(g["t_min"]) and est.t_max == pytest.approx(g["t_max"])
    assert est.mean_t_fn(t).shape == (t.numel(), 1)
    assert rel(est.mean_t_fn(t).reshape(-1), s["mean_t"]) < 1e-12
    assert rel(est.std_fn(t).reshape(-1), s["std"]) < 1e-12
    assert rel(est.diffusion_fn(ones, t).reshape(-1), s["diffusion"]) < 1e-12
    drift = torch.stack([torch.broadcast_to(est.drift_fn(ones, tt.reshape(1)), (1, g["D"]))[0] for tt in t])
    assert (drift - s["drift"]).abs().max() < 1e-12
    assert torch.allclose(est.solve_schedule(9).double(), s["solve"], atol=1e-6)
    for w in ("identity", "max_likelihood", "variance"):
        est._set_weight_fn(w)
        assert rel(est.weight_fn(t).reshape(-1), s["w_" + w]) < 1e-12
    assert torch.allclose(est.mean_base, s["mean_base"].float(), atol=1e-6)
    assert torch.allclose(est.std_base, s["std_base"].float(), rtol=1e-6)
    assert torch.allclose(est.approx_marginal_std(torch.tensor([est.t_max])), est.std_base)
    assert torch.allclose(est.noise_schedule(t), est.std_fn(t).reshape(-1) if g["sde"] == "ve" else 0.01 + 9.99 * t)
    # schedules stay inside [t_min, t_max] and run from t_max down to t_min
    tr = est.train_schedule(1000)
    assert tr.shape == (1000,) and tr.min() >= est.t_min and tr.max() <= est.t_max
    sol = est.solve_schedule(50)
    assert sol[0] == pytest.approx(est.t_max) and sol[-1] == pytest.approx(est.t_min) and (sol[1:] < sol[:-1]).all()


def test_ve_lognormal_and_power_law_schedules():
    from sbi_amd.neural_nets import build_score_matching_estimator

    theta, x = torch.randn(40, 3), torch.randn(40, 2)
    est = build_score_matching_estimator(theta, x, sde_type="ve", train_schedule="lognormal", solve_schedule="power_law")
    tr = est.train_schedule(2000)
    assert tr.min() >= est.t_min and tr.max() <= est.t_max and 0.2 < float(tr.mean()) < 0.8
    sol = est.solve_schedule(30)
    assert sol[0] == est.t_max and sol[-1] == est.t_min and (sol[1:] < sol[:-1]).all()
    # power law: equal steps in sigma^(1/rho) -- up to the rescaling of the unit interval onto [t_min, t_max], which moves
    # a time by at most t_min = 1e-3, i.e. ln sigma by 1e-3 ln(1e5) = 0.0115 and sigma^(1/7) by a factor 1.0016
    sig = est.std_fn(sol.double()).reshape(-1) ** (1 / 7.0)
    assert (sig[1:-1] - sig[:-2] - (sig[1] - sig[0])).abs().max() < 1e-2 * float(sig[0] - sig[1])
    with pytest.raises(ValueError):
        build_score_matching_estimator(theta, x, sde_type="ve", sigma_min=0.0)
    with pytest.raises(ValueError):
        build_score_matching_estimator(theta, x, sde_type="ve", solve_schedule="cosine")
    with pytest.raises(ValueError):
        build_score_matching_estimator(theta, x, sde_type="edm")
    assert build_score_matching_estimator(theta, x, sde_type="subvp").t_min == 1e-2


def test_layout_is_the_fmpe_layout_with_reference_key_names():
    from sbi_amd import _lib
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import build_flow_matching_estimator
    from sbi_amd.neural_nets.estimators.score_estimator import _cfg

    lib = _lib.load()
    for name in CASES[:2]:
        g = load_case(name)
        est = estimator_of(g)
        fm = build_flow_matching_estimator(g["theta"], g["x"], hidden_features=est.net.hyper.hidden_features,
                                           num_layers=est.net.hyper.num_layers)
        assert [e for e in est.net.hyper.entries()] == [e for e in fm.net.hyper.entries()]
        keys = ["net." + k for k, _ in est.net.hyper.entries()]
        assert all(k in g["state"] for k in keys)
        assert {k for k in g["state"] if k.startswith("net.") and "time_emb" not in k} == set(keys)
        assert {"mean_0", "std_0", "_mean_base", "_std_base"} <= set(g["state"])
        cfg = _cfg(est, 0.3)
        assert lib.sbi_amd_fmpe_param_count(cfg.net) == est.net.hyper.param_count() == est.net.flat_params.numel()
        # two columns per row with the control variate, one without: the FMPE workspace of 2n / n rows
        assert lib.sbi_amd_npse_train_workspace_floats(cfg, 200) == \
            lib.sbi_amd_fmpe_train_workspace_floats(cfg.net, 400)
        assert lib.sbi_amd_npse_train_workspace_floats(_cfg(est, 0.0), 200) == \
            lib.sbi_amd_fmpe_train_workspace_floats(cfg.net, 200)
    assert load_case(CASES[0])["state"]["net.input_layer.weight"].shape == (100, 5)
    assert estimator_of(load_case(CASES[0])).net.hyper.param_count() == 76405
    bad = _cfg(est, 0.3)
    bad.sde = 3
    assert lib.sbi_amd_npse_train_workspace_floats(bad, 64) == _lib.E_UNSUPPORTED
    bad = _cfg(est, 0.3)
    bad.net.H = 200
    assert lib.sbi_amd_npse_train_workspace_floats(bad, 64) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_npse_score(bad, None, None, None, None, 1, None, 1, 4, 0, None, None) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_npse_score(cfg, None, None, None, None, 1, None, 1, 4, 0, None, None) == _lib.E_BADARG
    assert lib.sbi_amd_npse_sample_sde(cfg, None, None, None, None, 1, None, 5, 1.0, None, 0, 0, 4, None, None) == \
        _lib.E_BADARG


def test_header_and_binding_agree():
    import ctypes

    from sbi_amd import _build, _lib

    text = open(os.path.join(ROOT, "include", "sbi_amd_npse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(sbi_amd_npse_\w+)\s*\(", text))
    assert len(syms) == 5 and syms == set(_lib.exported_symbols_npse())
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/sbi_amd_npse.h but not exported"


@pytest.mark.parametrize("name", CASES[1:3])
def test_state_dict_round_trip(name):
    from sbi_amd.neural_nets import build_score_matching_estimator

    g = load_case(name)
    est = estimator_of(g)
    sd = est.reference_state_dict()
    for k, v in sd.items():
        assert torch.equal(v.reshape(-1), g["state"][k].reshape(-1).float()), k
    est2 = build_score_matching_estimator(g["theta"] + 1.0, g["x"], sde_type=g["sde"], hidden_features=48, num_layers=2)
    est2.load_reference_state_dict(sd)
    assert torch.equal(est2.net.flat_params, est.net.flat_params) and torch.equal(est2.net.zstats, est.net.zstats)
    assert torch.equal(est2.mean_base, est.mean_base)
    est3 = build_score_matching_estimator(g["theta"] * 2.0, g["x"], sde_type=g["sde"], hidden_features=48, num_layers=2)
    est3.load_state_dict(est.state_dict())
    assert torch.equal(est3.std_base, est.std_base) and torch.equal(est3.net.zstats, est.net.zstats)
    o = oracle_of(g)                       # the oracle reads the estimator's own export
    o.load_reference_state_dict(sd)


def test_refusals_name_what_runs():
    from sbi_amd.inference import NPSE, posterior_score_nn
    from sbi_amd.inference.posteriors.vector_field_posterior import VectorFieldPosterior
    from sbi_amd.neural_nets import build_score_matching_estimator
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import build_flow_matching_estimator

    theta, x = torch.randn(32, 3), torch.randn(32, 2)
    for model in ("ada_mlp", "transformer", "transformer_cross_attn"):
        with pytest.raises(NotImplementedError, match="mlp"):
            posterior_score_nn(model=model)
        with pytest.raises(NotImplementedError, match="mlp"):
            build_score_matching_estimator(theta, x, net=model)
    with pytest.raises(NotImplementedError, match="mlp"):
        build_score_matching_estimator(theta, x, net=torch.nn.Linear(3, 3))
    with pytest.raises(NotImplementedError):
        build_score_matching_estimator(theta, x, compose_standardization=True)
    with pytest.raises(NotImplementedError, match="max_likelihood"):
        build_score_matching_estimator(theta, x, weight_fn=lambda t: t)
    with pytest.raises(ValueError):
        build_score_matching_estimator(theta, x, weight_fn="linear")
    with pytest.raises(NotImplementedError):
        build_score_matching_estimator(theta, torch.randn(32, 3, 3))
    with pytest.raises(NotImplementedError):
        build_score_matching_estimator(theta, x, embedding_net=torch.nn.Linear(2, 2))
    est = build_score_matching_estimator(theta, x, sde_type="vp")
    with pytest.raises(RuntimeError, match="no CPU fallback|ROCm"):
        est.loss(theta, x)
    with pytest.raises(RuntimeError, match="no CPU fallback|ROCm"):
        est(theta, x, torch.rand(32))
    prior = torch.distributions.Independent(torch.distributions.Normal(torch.zeros(3), torch.ones(3)), 1)
    post = VectorFieldPosterior(est, prior, device="cpu", sample_with="sde").set_default_x(x[0])
    with pytest.raises(NotImplementedError, match="corrector"):
        post.sample((4,), corrector="langevin")
    with pytest.raises(NotImplementedError, match="euler_maruyama"):
        post.sample((4,), predictor="ddim")
    with pytest.raises(NotImplementedError, match="iid"):
        post.sample((4,), x=x[:5])
    with pytest.raises(NotImplementedError, match="iid"):
        post.sample((4,), iid_method="fnpe")
    with pytest.raises(NotImplementedError, match="log_prob"):
        post.log_prob(theta)
    with pytest.raises(TypeError):
        post.sample((4,), predictor_params={"eta": 1.0, "foo": 2})
    with pytest.raises(ValueError):
        VectorFieldPosterior(est, prior, device="cpu", sample_with="vi")
    # a flow-matching estimator keeps refusing "sde", with the words it used before
    fm = build_flow_matching_estimator(theta, x)
    pf = VectorFieldPosterior(fm, prior, device="cpu").set_default_x(x[0])
    with pytest.raises(NotImplementedError, match="probability-flow ODE only"):
        pf.sample((4,), sample_with="sde")
    with pytest.raises(NotImplementedError):
        NPSE(prior=prior).append_simulations(theta, x, proposal=object())
    with pytest.raises(RuntimeError, match="ROCm"):
        NPSE(prior=None, device="cpu").append_simulations(theta, x).train(max_num_epochs=1)


def test_constructor_rules_of_the_trainer():
    from sbi_amd.inference import NPSE, posterior_score_nn

    theta, x = torch.randn(64, 3), torch.randn(64, 2)

    def built(inf):
        return inf._build_neural_net(theta, x)

    assert built(NPSE()).sde_type == "ve"                                   # None resolves to "ve"
    assert built(NPSE(sde_type="subvp")).sde_type == "subvp"
    assert built(NPSE(vf_estimator=posterior_score_nn(sde_type="vp"))).sde_type == "vp"
    assert built(NPSE(vf_estimator=posterior_score_nn(sde_type="vp"), sde_type="vp")).sde_type == "vp"
    with pytest.raises(ValueError, match="Conflicting `sde_type`"):
        NPSE(vf_estimator=posterior_score_nn(sde_type="vp"), sde_type="ve")
    with pytest.warns(FutureWarning, match="score_estimator"):
        assert built(NPSE(score_estimator=posterior_score_nn(sde_type="vp"))).sde_type == "vp"
    with pytest.warns(FutureWarning, match="density_estimator"):
        NPSE(density_estimator=posterior_score_nn())
    with pytest.warns(FutureWarning, match="string"):
        assert built(NPSE(vf_estimator="mlp", sde_type="vp")).sde_type == "vp"
    with pytest.raises(ValueError, match="Cannot pass both"):
        NPSE(vf_estimator=posterior_score_nn(), score_estimator=posterior_score_nn())
    with pytest.raises(ValueError, match="Cannot pass both"):
        NPSE(vf_estimator=posterior_score_nn(), density_estimator=posterior_score_nn())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError):
            NPSE(vf_estimator="transformer")
    inf = NPSE()
    inf._neural_net = built(inf)
    with pytest.raises(ValueError):
        inf.build_posterior(sample_with="vi")
    assert inf.build_posterior().sample_with == "sde"
    assert inf.build_posterior(sample_with="ode").sample_with == "ode"


def test_trainer_loop_bookkeeping_with_oracle_backed_estimator():
    """Epoch loop of the trainer on a CPU stand-in estimator: EMA-smoothed summaries, validation at fixed times between
    t_min + nugget and t_max - nugget, resume_training, calibration kernel."""
    from sbi_amd.inference import NPSE
    from tests.helpers import linear_gaussian_data

    theta, x = linear_gaussian_data(300, 3, 2)
    torch.manual_seed(0)
    inf = NPSE(vf_estimator=oracle_score_build_fn(sde="vp", H=16, L=1, E=8), show_progress_bars=False)
    inf.append_simulations(theta, x)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inf.train(training_batch_size=64, max_num_epochs=3, validation_times=torch.tensor([0.2, 0.5, 0.8]),
                  ema_loss_decay=0.25)
        s = inf.summary
        assert len(s["training_loss"]) == len(s["validation_loss"]) == 4 and s["epochs_trained"] == [4]
        assert all(torch.isfinite(torch.tensor(s["validation_loss"])))
        split = inf.train_indices.clone()
        inf.train(training_batch_size=64, max_num_epochs=5, resume_training=True, validation_times=3,
                  calibration_kernel=lambda xx: torch.ones(xx.shape[0]) * 2.0)
        assert torch.equal(split, inf.train_indices) and inf.epoch == 6
    inf._summary["validation_loss"] = [1.0, 0.9, 1.1, 1.0] * 3
    inf._best_val_loss, inf._val_loss, inf._epochs_since_last_improvement = 0.5, 2.0, 0
    inf._converged(epoch=8, stop_after_epochs=4)
    assert inf._epochs_since_last_improvement == 1


def test_estimator_and_posterior_pickle_round_trip():
    from copy import deepcopy

    from sbi_amd.inference.posteriors.vector_field_posterior import VectorFieldPosterior
    from sbi_amd.neural_nets import build_score_matching_estimator

    theta, x = torch.randn(40, 3), torch.randn(40, 2)
    for sde in ("ve", "vp", "subvp"):
        est = build_score_matching_estimator(theta, x, sde_type=sde, hidden_features=32, num_layers=2,
                                             weight_fn="variance")
        est2 = pickle.loads(pickle.dumps(est))
        assert type(est2) is type(est) and est2.weight_fn_name == "variance" and est2.t_min == est.t_min
        assert torch.equal(est2.net.flat_params, est.net.flat_params) and torch.equal(est2.std_base, est.std_base)
        assert torch.equal(deepcopy(est).net.zstats, est.net.zstats)
    prior = torch.distributions.Independent(torch.distributions.Normal(torch.zeros(3), torch.ones(3)), 1)
    post = VectorFieldPosterior(est, prior, device="cpu", sample_with="sde")
    post2 = pickle.loads(pickle.dumps(post))
    assert post2.sample_with == "sde"
    assert torch.equal(post2.vector_field_estimator.net.flat_params, est.net.flat_params)


@pytest.mark.parametrize("name", CASES)
def test_oracle_restatement_in_fp64_reproduces_the_fp64_records(name):
    g = load_case(name)
    o = oracle_of(g, double=True)
    th, x, t, eps = g["theta"].double(), g["x"].double(), g["times"].double(), g["eps"].double()
    for tag, cv in (("", True), ("_nocv", False)):
        o.zero_grad()
        losses = o.loss(th, x, t, eps, control_variate=cv)
        assert rel(losses.detach(), g["losses64" + tag]) < 1e-9
        if "grads64" + tag in g:
            losses.mean().backward()
            for k, ref in g["grads64" + tag].items():
                got = o.o.p[k.replace(".", "/")].grad
                assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max()) + 1e-300, (k, tag)
    with torch.no_grad():
        assert rel(o.score(g["theta_q"].double(), x[:1], g["tq"].double()), g["score64"]) < 1e-9
        assert rel(o.ode_fn(g["theta_q"].double(), x[:1], g["tq"].double()), g["ode64"]) < 1e-9
        s = g["em"]
        assert rel(o.sample_sde(x[:1], s["ts"].double(), s["noise"].double()), s["out64"]) < 1e-9
        mb, sb = o.base()
        assert torch.allclose(mb.float(), g["schedule"]["mean_base"].float(), atol=1e-6)
        assert torch.allclose(sb.float(), g["schedule"]["std_base"].float(), rtol=1e-6)


@pytest.mark.parametrize("name", CASES[1:])
def test_oracle_in_fp32_is_as_close_to_fp64_as_the_reference_is(name):
    """The fp32 restatement follows the reference's arithmetic, so its distance from the fp64 record is of the size of
    the reference's own (recorded per block in the fixture): within 4 x + a 1e-6 floor."""
    g = load_case(name)
    o = oracle_of(g)
    losses = o.loss(g["theta"], g["x"], g["times"], g["eps"])
    ref_err = float((g["losses"].double() - g["losses64"]).abs().max())
    assert float((losses.detach().double() - g["losses64"]).abs().max()) <= 4 * ref_err + 1e-6 * float(g["losses64"].abs().max())
    losses.mean().backward()
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import FMPEHyper

    kw = g["kw"]
    hyper = FMPEHyper(D=g["D"], C=g["C"], hidden_features=kw.get("hidden_features", 100), num_layers=kw.get("num_layers", 5))
    slices, off = [], 0
    for key, shape in hyper.entries():
        slices.append((key, off, 0, shape))
    got = flat_grad(o, slices)
    ref64 = torch.cat([g["grads64"]["net." + k].reshape(-1) for k, _ in hyper.entries()])
    ref_err = max(g["grads32_err"].values())
    assert float((got.double() - ref64).abs().max()) <= 4 * ref_err + 1e-6 * float(ref64.abs().max())
