"""Host side of NPSE with iid observations, no GPU needed: the fp64 tables of
sbi_amd.inference.potentials.vector_field_adaptor against outputs of the real sbi classes
(tests/golden/npse_iid_reference.pt, written by tools/make_golden_npse_iid.py), the diagonal branches against the
per-call restatement tests/npse_iid_oracle.py (itself pinned to the same fixture), constructor defaults, names and
refusals."""

import inspect
import math

import pytest
import torch

from tests.npse_iid_oracle import IID_CASES, METHODS, compose, iid_score, load_iid_case, make_prior, random_prior_spec
from tests.test_npse_host_cpu import estimator_of, oracle_of

# 1e-10 of max|ref|: the formula was measured at 3.1e-14 against the real classes (D = 3, N = 5, three SDE families); the
# allowance covers the conditioning of other seeds
TABLE_TOL = 1e-10


def score_fn(g, method, est=None, **kw):
    from sbi_amd.inference.potentials.vector_field_adaptor import get_iid_method

    est = estimator_of(g) if est is None else est
    fn = get_iid_method(method)(est, make_prior(g["prior_kind"], g["prior"]), **kw)
    if method == "auto_gauss":
        fn.posterior_precision_est_fn = lambda conditions: g["prec"]      # the fixture's recorded precisions
    return fn


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", IID_CASES)
def test_tables_reproduce_the_real_classes_in_fp64(name, method):
    g = load_iid_case(name)
    rec = g["methods"][method]
    fn = score_fn(g, method)
    tb = fn.tables(g["tq"].double(), g["xs"])
    D, N = g["D"], g["N"]
    assert tb.mats.shape == (4, 3, D, D) and tb.vecs.shape == (4, D) and tb.mats.dtype == torch.float64
    assert (tb.lam is None) == (method == "fnpe") and (tb.lam is None or tb.lam.shape == (N, D, D))
    for k in range(4):
        got = compose(tb, k, rec["s64"][k], g["theta_q"].double())
        ref = rec["score64"][k]
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"{name} {method} t={float(g['tq'][k]):.3g}: {err:.3e} of max|ref|")
        assert err <= TABLE_TOL
    if method == "auto_gauss":      # the PSD correction is active at t_max and idle at t_min: C - c I = corr
        eye = torch.eye(D, dtype=torch.float64)
        m, s = fn._ms(g["tq"].double())
        corr = tb.mats[:, 1] - (m**2 / s**2)[:, None, None] * eye
        assert float((corr[0] - 0.01 * eye).abs().max()) < 1e-9 * float(tb.mats[0, 1].abs().max())   # nugget only
        assert float(torch.linalg.eigvalsh(corr[3]).max()) > 0.1


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", IID_CASES)
def test_the_per_call_oracle_reproduces_the_real_classes_in_fp64(name, method):
    g = load_iid_case(name)
    rec = g["methods"][method]
    o = oracle_of(g, double=True)
    with torch.no_grad():
        for k in range(4):
            got = iid_score(o, method, g["prior_kind"], g["prior"], g["theta_q"].double(), g["xs"].double(),
                            float(g["tq"][k].double()), prec=g["prec"])
            ref = rec["score64"][k]
            assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
            s = o.score(g["theta_q"].double().repeat_interleave(g["N"], 0), g["xs"].double().repeat(7, 1),
                        g["tq"][k].double().expand(7 * g["N"])).reshape(7, g["N"], g["D"])
            assert float((s - rec["s64"][k]).abs().max()) <= 1e-9 * float(rec["s64"][k].abs().max())


@pytest.mark.parametrize("name", IID_CASES)
def test_diagonal_branches_reproduce_the_real_classes_in_fp64(name):
    """gauss with enable_lam_psd=True and auto_gauss with precision_est_only_diag against the fixture's records of the
    real classes: sbi's element-wise correction under Independent(Normal), the eigendecomposition under the dense prior."""
    g = load_iid_case(name)
    est = estimator_of(g)
    s64 = g["methods"]["gauss"]["s64"]           # the per-observation scores do not depend on the method
    fired = 0
    for tag, method, kw in (("gauss_psd", "gauss", dict(enable_lam_psd=True, scale_from_prior_precision=0.5)),
                            ("auto_gauss_diag", "auto_gauss", dict(precision_est_only_diag=True))):
        fn = score_fn(g, method, est=est, **kw)
        if method == "auto_gauss":
            fn.posterior_precision_est_fn = lambda conditions: g["diag_prec"]
        tb = fn.tables(g["tq"].double(), g["xs"])
        m, sd = fn._ms(g["tq"].double())
        for k in range(4):
            got = compose(tb, k, s64[k], g["theta_q"].double())
            ref = g[tag + "_score64"][k]
            err = float((got - ref).abs().max() / ref.abs().max())
            print(f"{name} {tag} t={float(g['tq'][k]):.3g}: {err:.3e} of max|ref|")
            assert err <= TABLE_TOL
            corr = tb.mats[k, 1] - (m[k] ** 2 / sd[k] ** 2) * torch.eye(g["D"], dtype=torch.float64)
            fired += int(float(corr.abs().max()) > 0.011)
            if g["prior_kind"] == "indep":      # all diagonal: the element-wise variant keeps every table diagonal
                assert float((tb.mats[k] - torch.diag_embed(torch.diagonal(tb.mats[k], dim1=1, dim2=2))).abs().max()) == 0
    assert fired >= 2       # beyond the nugget at the late times


@pytest.mark.parametrize("name", ["ve_indep", "vp_indep", "vp_mvn"])
def test_diagonal_branches_match_the_per_call_restatement(name):
    """precision_est_only_diag (diagonal estimated precisions) and gauss with enable_lam_psd=True: with a diagonal prior
    both take sbi's element-wise correction, with the dense prior the eigendecomposition."""
    g = load_iid_case(name)
    est = estimator_of(g)
    o = oracle_of(g, double=True)
    th, xs = g["theta_q"].double(), g["xs"].double()
    diag_prec = torch.diagonal(g["prec"], dim1=1, dim2=2).contiguous() * 0.3      # (N, D): weak, so the fix fires
    fired = 0
    for method, kw, okw in (("auto_gauss", dict(precision_est_only_diag=True), dict(prec=diag_prec)),
                            ("gauss", dict(enable_lam_psd=True, scale_from_prior_precision=0.5),
                             dict(psd=True, scale=0.5))):
        fn = score_fn(g, method, est=est, **kw)
        if method == "auto_gauss":
            fn.posterior_precision_est_fn = lambda conditions: diag_prec
        tb = fn.tables(g["tq"].double(), g["xs"])
        for k in range(4):
            t = float(g["tq"][k].double())
            with torch.no_grad():
                s = o.score(th.repeat_interleave(g["N"], 0), xs.repeat(7, 1), torch.full((35,), t, dtype=torch.float64))
                s = s.reshape(7, g["N"], g["D"])
                ref = iid_score(o, method, g["prior_kind"], g["prior"], th, xs, t, s=s, **okw)
            got = compose(tb, k, s, th)
            assert float((got - ref).abs().max()) <= TABLE_TOL * float(ref.abs().max()), (method, k)
            m, sd = fn._ms(g["tq"].double())
            corr = tb.mats[k, 1] - (m[k] ** 2 / sd[k] ** 2) * torch.eye(g["D"], dtype=torch.float64)
            fired += int(float(corr.abs().max()) > 0.011)
            if g["prior_kind"] == "indep":      # all diagonal: the element-wise variant keeps every table diagonal
                assert float((tb.mats[k] - torch.diag_embed(torch.diagonal(tb.mats[k], dim1=1, dim2=2))).abs().max()) == 0
    assert fired >= 2       # beyond the nugget at the late times


def test_constructor_defaults_and_method_names():
    from sbi_amd.inference.potentials import vector_field_adaptor as A

    assert A.get_iid_method("fnpe") is A.FactorizedNPEScoreFunction
    assert A.get_iid_method("gauss") is A.GaussCorrectedScoreFn
    assert A.get_iid_method("auto_gauss") is A.AutoGaussCorrectedScoreFn

    def defaults(cls):
        return {k: v.default for k, v in inspect.signature(cls.__init__).parameters.items()
                if v.default is not inspect.Parameter.empty}

    assert defaults(A.FactorizedNPEScoreFunction) == dict(device="cpu", prior_score_weight=None)
    assert defaults(A.GaussCorrectedScoreFn) == dict(posterior_precision=None, scale_from_prior_precision=2.0,
                                                     enable_lam_psd=False, lam_psd_nugget=0.01, device="cpu")
    assert defaults(A.AutoGaussCorrectedScoreFn) == dict(enable_lam_psd=True, lam_psd_nugget=0.01,
                                                         precision_est_only_diag=False, precision_est_budget=None,
                                                         precision_initial_sampler_steps=100, device="cpu")
    sample = inspect.signature(__import__("sbi_amd.inference.posteriors.vector_field_posterior", fromlist=["x"])
                               .VectorFieldPosterior.sample).parameters
    assert sample["iid_method"].default is None and sample["iid_params"].default is None


def test_refusals_name_what_runs():
    from sbi_amd.inference.posteriors.vector_field_posterior import VectorFieldPosterior
    from sbi_amd.inference.potentials import vector_field_adaptor as A
    from sbi_amd.inference.potentials.vector_field_potential import (VectorFieldBasedPotential,
                                                                     vector_field_estimator_based_potential)
    from sbi_amd.neural_nets.estimators.flowmatching_estimator import build_flow_matching_estimator
    from sbi_amd.utils.torchutils import BoxUniform

    g = load_iid_case("vp_indep")
    est = estimator_of(g)
    prior = make_prior("indep", g["prior"])
    box = BoxUniform(-2 * torch.ones(3), 2 * torch.ones(3))
    with pytest.raises(NotImplementedError, match="fnpe.*gauss"):
        A.get_iid_method("jac_gauss")
    with pytest.raises(NotImplementedError):
        A.get_iid_method("nope")
    for cls in (A.GaussCorrectedScoreFn, A.AutoGaussCorrectedScoreFn):
        with pytest.raises(NotImplementedError, match="fnpe"):
            cls(est, box)
        with pytest.raises(NotImplementedError, match="fnpe"):
            cls(est, torch.distributions.Independent(torch.distributions.Exponential(torch.ones(3)), 1))
    with pytest.raises(NotImplementedError, match="BoxUniform"):
        A.FactorizedNPEScoreFunction(est, torch.distributions.Independent(torch.distributions.Exponential(torch.ones(3)), 1))
    fm = build_flow_matching_estimator(g["theta"], g["x"], hidden_features=32, num_layers=1)
    with pytest.raises((NotImplementedError, ValueError)):
        A.FactorizedNPEScoreFunction(fm, prior)
    with pytest.raises(NotImplementedError, match="score"):
        VectorFieldBasedPotential(fm, prior)
    with pytest.raises(NotImplementedError, match="iid"):
        VectorFieldPosterior(fm, prior, device="cpu").sample((2,), x=g["xs"])
    pot, _ = vector_field_estimator_based_potential(est, prior, g["xs"][:1])
    with pytest.raises(NotImplementedError, match="log_prob"):
        pot(g["theta_q"])
    with pytest.raises(NotImplementedError, match="guidance"):
        pot.set_x(g["xs"][:1], guidance_method="affine_classifier_free")
    with pytest.raises(NotImplementedError, match="jac_gauss"):
        pot.set_x(g["xs"], x_is_iid=True, iid_method="jac_gauss")
    pot.set_x(g["xs"], x_is_iid=True, iid_method="gauss")
    assert pot.x_is_iid and pot.x_o.shape == (5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback|ROCm"):      # the composition is a kernel: no host path
        pot.gradient(g["theta_q"], torch.tensor([0.5]))
    # a posterior that does not live on a ROCm device keeps refusing iid observations, and says why
    post = VectorFieldPosterior(est, prior, device="cpu", sample_with="sde").set_default_x(g["xs"][0])
    with pytest.raises(NotImplementedError, match="iid.*device only"):
        post.sample((4,), x=g["xs"])
    with pytest.raises(NotImplementedError, match="iid.*device only"):
        post.sample((4,), iid_method="gauss")
    with pytest.raises(NotImplementedError, match="jac_gauss"):
        post.sample((4,), iid_method="jac_gauss")
    with pytest.raises(NotImplementedError, match="guidance"):
        post.sample((4,), guidance_method="universal")
    with pytest.raises(NotImplementedError, match="corrector"):
        post.sample((4,), x=g["xs"], corrector="langevin")
    with pytest.raises(NotImplementedError, match="log_prob"):
        post.log_prob(g["theta_q"], x=g["xs"])


def test_fnpe_base_scale_box_uniform_and_single_observation():
    from sbi_amd.inference.potentials import vector_field_adaptor as A
    from sbi_amd.utils.torchutils import BoxUniform

    g = load_iid_case("ve_mvn")
    est = estimator_of(g)
    ts = est.solve_schedule(6).double()
    eye = torch.eye(3, dtype=torch.float64)
    fn = A.FactorizedNPEScoreFunction(est, make_prior("mvn", g["prior"]))
    tb = fn.tables(ts, g["xs"])
    assert tb.base_scale == pytest.approx(1 / math.sqrt(5)) and tb.lam is None
    assert torch.equal(tb.mats[:, 0], eye.expand(6, 3, 3)) and torch.equal(tb.mats[:, 1], eye.expand(6, 3, 3))
    w = (est.t_max - ts) / est.t_max
    assert torch.allclose(tb.mats[:, 2], 4 * w[:, None, None] * torch.linalg.inv(g["prior"]["cov"].double()), rtol=1e-12)
    assert float(tb.mats[0, 2].abs().max()) == 0 and float(tb.mats[-1, 2].abs().max()) > 0      # w(t_max) = 0
    box = A.FactorizedNPEScoreFunction(est, BoxUniform(-2 * torch.ones(3), 2 * torch.ones(3))).tables(ts, g["xs"])
    assert float(box.mats[:, 2].abs().max()) == 0 and float(box.vecs.abs().max()) == 0
    assert box.base_scale == pytest.approx(1 / math.sqrt(5))
    # one observation composes to the plain score for every method
    for method in METHODS:
        one = score_fn(g, method, est=est).tables(ts, g["xs"][:1])
        assert one.lam is None and torch.equal(one.mats[:, 0], eye.expand(6, 3, 3))
        assert torch.equal(one.mats[:, 1], eye.expand(6, 3, 3))
        assert float(one.mats[:, 2].abs().max()) == 0 and float(one.vecs.abs().max()) == 0
    lam, mats, vecs = tb.on("cpu")
    assert lam is None and mats.dtype == torch.float32 and mats.is_contiguous() and vecs.shape == (6, 3)


def test_header_and_binding_agree_for_the_iid_entry_points():
    import ctypes
    import os
    import re

    from sbi_amd import _build, _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sbi_amd_npse_iid.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(sbi_amd_npse_\w+)\s*\(", text))
    assert len(syms) == 5 and syms == set(_lib.exported_symbols_npse_iid())
    assert not syms & set(_lib.exported_symbols_npse())
    _build.build()
    lib = ctypes.CDLL(str(_build.LIB_PATH))
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/sbi_amd_npse_iid.h but not exported"


def test_envelope_and_bad_arguments_are_refused_on_the_host():
    """Nothing is launched: the pointers below are not device memory."""
    import ctypes

    from sbi_amd import _lib
    from sbi_amd.neural_nets import build_score_matching_estimator
    from sbi_amd.neural_nets.estimators.score_estimator import _cfg, iid_fused_supported

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    small = build_score_matching_estimator(torch.randn(40, 3), torch.randn(40, 2), sde_type="vp", hidden_features=32,
                                           num_layers=1)
    wide = build_score_matching_estimator(torch.randn(40, 17), torch.randn(40, 2), sde_type="vp", hidden_features=32,
                                          num_layers=1)
    assert lib.sbi_amd_npse_iid_workspace_floats(_cfg(small), 5) == 5 * 128
    assert lib.sbi_amd_npse_iid_workspace_floats(_cfg(small), 1025) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_npse_iid_workspace_floats(_cfg(wide), 5) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_npse_iid_workspace_floats(_cfg(small), 0) == _lib.E_BADARG
    assert iid_fused_supported(small, 1024) and not iid_fused_supported(small, 1025)
    assert not iid_fused_supported(wide, 5) and not iid_fused_supported(small, 5, steps=65536)
    sample = lambda cfg, N, steps: lib.sbi_amd_npse_sample_sde_iid(cfg, p, p, p, p, N, p, steps, 1.0, None, p, p, None,
                                                                    0, 0, 8, p, p, None)
    assert sample(_cfg(wide), 5, 10) == _lib.E_UNSUPPORTED
    assert sample(_cfg(small), 1025, 10) == _lib.E_UNSUPPORTED
    assert sample(_cfg(small), 5, 65536) == _lib.E_UNSUPPORTED
    assert sample(_cfg(small), 0, 10) == _lib.E_BADARG
    assert lib.sbi_amd_npse_sde_normals(1, 0, -1, 8, 3, p, None) == _lib.E_BADARG
    assert lib.sbi_amd_npse_compose_iid(p, p, None, p, p, 8, 0, 3, p, None) == _lib.E_BADARG
    assert lib.sbi_amd_npse_compose_iid(p, p, None, p, p, 8, 5, 129, p, None) == _lib.E_BADARG
    assert lib.sbi_amd_npse_sde_normals(1, -1, 0, 8, 3, p, None) == _lib.E_BADARG
    assert lib.sbi_amd_npse_score_iid(_cfg(wide), p, p, p, p, 5, p, None, p, p, 8, p, p, None) == _lib.E_UNSUPPORTED
    assert lib.sbi_amd_npse_score_iid(_cfg(small), p, p, p, p, 5, p, None, None, p, 8, p, p, None) == _lib.E_BADARG
