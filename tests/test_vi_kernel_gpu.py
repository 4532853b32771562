"""The Gaussian-q kernels through the C ABI (include/sbi_amd_vi.h) against tests/vi_oracle.py in fp64, at the
project's row bound |d| <= 1e-5 (1 + |ref|): draw (theta, log q, the exported eps, row independence, the interval
link at |z| = 50), log_prob on the draw's output, and step -- the gradient of every method and flag combination over
D in {1, 2, 5, 16}, n in {1, 63, 64, 65, 257, 4 097}, both families and every link kind, bit-identity of two launches,
bit-identity of the update with sbi_amd_adam_clip_step when the clip is inactive, the clipped update against the
oracle, the non-finite guard -- and the plan's refusals.

Inputs: r is correlated with eps (r = 0.5 + B eps + noise) so that no gradient entry is small by cancellation; the
oracle's gradient entries outside the structurally-zero upper triangle are asserted to be >= 1e-3 in magnitude (the
seed is advanced until the ORACLE says so; the kernels are not consulted).  phi and the link ranges keep |z| within a
few units, where theta (fp32) still determines z to ~1e-6: the round trip of log_prob depends on it."""
import itertools
from ctypes import byref, c_int64

import pytest
import torch

from sbi_amd import _lib
from sbi_amd._lib import VIConfigC
from sbi_amd.utils.parity import row_parity
from tests import vi_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METHOD = {"rKL": 0, "IW": 1, "alpha": 2, "fKL": 3}
LINKS = ["none", "affine", "interval", "lower", "upper", "mix"]
RING = 8


def within(got, ref, what):
    rp = row_parity(got.detach().cpu(), ref.detach().cpu())
    print(f"{what}: worst {rp['worst_scaled']:.3f} x bound (|d| = {rp['worst_abs']:.2e} at ref {rp['worst_ref']:.3g})")
    assert rp["worst_scaled"] <= 1.0, (what, rp)


def make_link(kind, D, g):
    if kind == "none":
        return None
    kinds = {"affine": [0], "interval": [1], "lower": [2], "upper": [3], "mix": [1, 0, 2, 3]}[kind]
    t = torch.zeros(4, D)
    for d in range(D):
        k = kinds[d % len(kinds)]
        t[0, d] = k
        a = float(torch.randn((), generator=g))
        if k == 0:
            t[1, d], t[2, d] = a, (0.5 + float(torch.rand((), generator=g))) * (1 if d % 2 == 0 else -1)
        elif k == 1:
            width = 2.0 + 2.0 * float(torch.rand((), generator=g))
            t[1, d], t[2, d] = a, width
            t[3, d] = t[1, d] + t[2, d]
        else:
            t[1, d], t[2, d] = a, 1.0 if k == 2 else -1.0
    return t


def make_phi(D, full, g):
    loc = 0.3 * torch.randn(D, generator=g)
    if full:
        L = torch.diag(0.5 + 0.3 * torch.rand(D, generator=g)) + 0.15 * torch.randn(D, D, generator=g).tril(-1)
        L = L + torch.randn(D, D, generator=g).triu(1)              # junk above the diagonal: must never be read
        return torch.cat([loc, L.reshape(-1)])
    return torch.cat([loc, 0.3 * torch.randn(D, generator=g) - 0.5])


def lib():
    return _lib.load()


def draw(D, full, phi, link, n, seed, step, row_offset=0, want_eps=True):
    theta = torch.empty(n, D, device=DEV)
    log_q = torch.empty(n, device=DEV)
    eps = torch.empty(n, D, device=DEV) if want_eps else None
    rc = lib().sbi_amd_vi_gauss_draw(D, int(full), _lib.ptr(phi), _lib.ptr(link), n, seed, step, row_offset,
                                     _lib.ptr(theta), _lib.ptr(log_q), _lib.ptr(eps), _lib.current_stream(phi.device))
    assert rc == 0
    return theta, log_q, eps


class StepState:
    def __init__(self, phi, m=None, v=None):
        self.phi = phi.clone()
        self.m = torch.zeros_like(phi) if m is None else m.clone()
        self.v = torch.zeros_like(phi) if v is None else v.clone()
        self.snap = phi.clone() + 0.125
        self.ring = torch.full((RING,), -7.0, device=DEV)
        self.status = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.grad = torch.full_like(phi, -9.0)


def step(cfg, st, p, r, n, link, clip, lr, t, seed, stp, want_grad=True):
    need = c_int64(0)
    assert lib().sbi_amd_vi_gauss_plan(cfg.D, n, byref(need)) == 0
    ws = torch.empty((need.value + 3) // 4, device=DEV)
    rc = lib().sbi_amd_vi_gauss_step(byref(cfg), _lib.ptr(p), _lib.ptr(r), n, _lib.ptr(st.phi), _lib.ptr(st.m),
                                     _lib.ptr(st.v), _lib.ptr(st.snap), _lib.ptr(link), clip, lr, 0.9, 0.999, 1e-8, t,
                                     seed, stp, _lib.ptr(ws), _lib.ptr(st.ring), RING, _lib.ptr(st.status),
                                     _lib.ptr(st.grad) if want_grad else None, _lib.current_stream(st.phi.device))
    assert rc == 0
    torch.cuda.synchronize()


def build_case(D, n, full, link_kind, method, kw, base_seed):
    """Inputs whose ORACLE gradient has no entry below 1e-3 outside the upper triangle."""
    for attempt in range(40):
        g = torch.Generator().manual_seed(1000 * base_seed + attempt)
        phi = make_phi(D, full, g).to(DEV)
        link = make_link(link_kind, D, g)
        link_dev = None if link is None else link.to(DEV).contiguous()
        seed, stp = 1234567 + attempt, 3 + attempt
        theta, log_q, eps = draw(D, full, phi, link_dev, n, seed, stp)
        B = 0.7 * torch.randn(D, D, generator=g) + torch.eye(D)
        e = eps.cpu()
        r = (0.5 + e @ B.T + 0.3 * torch.randn(n, D, generator=g)).contiguous()
        p = (log_q.cpu() + 0.2 * e.sum(-1) + 0.3 * torch.randn(n, generator=g)).contiguous()
        g64, loss64 = O.gradient(method, phi, link, eps, p, None if method == "fKL" else r, D, full, **kw)
        live = torch.ones(phi.numel(), dtype=torch.bool)
        if full:
            live[D:] = torch.ones(D, D).tril().bool().reshape(-1)
        if bool((g64[live].abs() >= 1e-3).all()) and bool(torch.isfinite(g64).all()):
            return dict(phi=phi, link=link, link_dev=link_dev, seed=seed, stp=stp, theta=theta, log_q=log_q, eps=eps,
                        p=p.to(DEV), r=None if method == "fKL" else r.to(DEV), g64=g64, loss64=loss64, live=live)
    raise AssertionError("no seed gave an oracle gradient with every entry >= 1e-3")


def config(D, full, method, kw):
    stl = bool(kw.get("stick_the_landing", False) or kw.get("dreg", False))
    return VIConfigC(D=D, full_cov=int(full), method=METHOD[method], K=kw.get("K", 1), stick_the_landing=int(stl),
                     dreg=int(kw.get("dreg", False)), unbiased=int(kw.get("unbiased", False)),
                     alpha=float(kw.get("alpha", 0.0)))


# ---- draw / log_prob ------------------------------------------------------------------------------------------------
DRAW_CASES = [(1, 1, True, "interval"), (2, 63, False, "affine"), (5, 64, True, "mix"), (16, 65, True, "interval"),
              (16, 257, False, "lower"), (5, 4097, True, "upper"), (2, 257, True, "none"), (16, 4097, True, "mix")]


@pytest.mark.parametrize("D,n,full,link_kind", DRAW_CASES)
def test_draw_and_log_prob_against_the_oracle(D, n, full, link_kind):
    g = torch.Generator().manual_seed(D * 100 + n)
    phi = make_phi(D, full, g).to(DEV)
    link = make_link(link_kind, D, g)
    link_dev = None if link is None else link.to(DEV)
    seed, stp = 2**40 + 17 * n, 5
    theta, log_q, eps = draw(D, full, phi, link_dev, n, seed, stp)
    within(eps, O.philox_normal(seed, stp, range(n), D), "eps vs the host Philox / Box-Muller")
    _, th64, lq64 = O.forward(phi.cpu().double(), link, eps.cpu().double(), D, full)
    within(theta, th64, "theta")
    within(log_q, lq64, "log q")
    back = torch.empty(n, device=DEV)
    assert lib().sbi_amd_vi_gauss_log_prob(D, int(full), _lib.ptr(phi), _lib.ptr(link_dev), _lib.ptr(theta), n,
                                           _lib.ptr(back), _lib.current_stream(phi.device)) == 0
    within(back, log_q, "log_prob(draw's theta) vs draw's log q")


def test_rows_do_not_depend_on_the_batch_or_the_offset():
    D, full = 5, True
    g = torch.Generator().manual_seed(9)
    phi, link = make_phi(D, full, g).to(DEV), make_link("mix", D, g).to(DEV)
    th_a, lq_a, eps_a = draw(D, full, phi, link, 4097, 77, 2)
    th_b, lq_b, eps_b = draw(D, full, phi, link, 65, 77, 2, row_offset=300)
    th_c, lq_c, eps_c = draw(D, full, phi, link, 1, 77, 2, row_offset=4096)
    assert torch.equal(eps_b, eps_a[300:365]) and torch.equal(th_b, th_a[300:365]) and torch.equal(lq_b, lq_a[300:365])
    assert torch.equal(eps_c, eps_a[4096:]) and torch.equal(th_c, th_a[4096:])
    _, _, eps_d = draw(D, full, phi, link, 65, 77, 3, row_offset=300)
    assert not torch.equal(eps_d, eps_b)                                   # another step: another stream
    _, _, eps_big = draw(D, full, phi, link, 2, 77, 2, row_offset=2**32 + 5)
    within(eps_big, O.philox_normal(77, 2, [2**32 + 5, 2**32 + 6], D), "rows past 2^32")
    e = eps_a.double()
    assert abs(float(e.mean())) < 0.02 and abs(float(e.var()) - 1) < 0.03


@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_interval_link_stays_strictly_inside(sign):
    D = 4
    lo = torch.tensor([-2.0, 0.1, 1000.0, -1e-3])
    hi = torch.tensor([2.0, 0.4, 1000.5, 1e-3])
    link = torch.stack([torch.ones(D), lo, hi - lo, hi]).to(DEV)
    phi = torch.cat([torch.full((D,), 50.0 * sign), torch.full((D,), -7.0)]).to(DEV)       # z = +-50 +- 1e-3 eps
    theta, log_q, _ = draw(D, False, phi, link, 257, 5, 1)
    assert bool((theta > lo.to(DEV)).all()) and bool((theta < hi.to(DEV)).all())
    assert torch.isfinite(log_q).all()


def test_plan_envelope():
    need = c_int64(0)
    assert lib().sbi_amd_vi_gauss_plan(16, 65536, byref(need)) == 0 and need.value >= 65536 * 4
    assert lib().sbi_amd_vi_gauss_plan(17, 256, byref(need)) == _lib.E_UNSUPPORTED
    assert lib().sbi_amd_vi_gauss_plan(16, 65537, byref(need)) == _lib.E_UNSUPPORTED
    assert lib().sbi_amd_vi_gauss_plan(0, 256, byref(need)) == _lib.E_BADARG
    # D = 17 is refused by step / draw / log_prob as well (real, amply sized buffers: nothing here depends on the
    # refusal coming before a launch)
    D, n = 17, 8
    cfg = config(D, True, "rKL", {})
    phi = torch.cat([torch.zeros(D), torch.eye(D).reshape(-1)]).to(DEV)
    st = StepState(phi)
    p, r, ws = torch.zeros(n, device=DEV), torch.zeros(n, D, device=DEV), torch.zeros(4 * n, device=DEV)
    stream = _lib.current_stream(phi.device)
    assert lib().sbi_amd_vi_gauss_step(byref(cfg), _lib.ptr(p), _lib.ptr(r), n, _lib.ptr(st.phi), _lib.ptr(st.m),
                                       _lib.ptr(st.v), _lib.ptr(st.snap), None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1, 0, 0,
                                       _lib.ptr(ws), _lib.ptr(st.ring), RING, _lib.ptr(st.status), None,
                                       stream) == _lib.E_UNSUPPORTED
    theta, log_q = torch.zeros(n, D, device=DEV), torch.zeros(n, device=DEV)
    assert lib().sbi_amd_vi_gauss_draw(D, 1, _lib.ptr(phi), None, n, 0, 0, 0, _lib.ptr(theta), _lib.ptr(log_q), None,
                                       stream) == _lib.E_UNSUPPORTED
    assert lib().sbi_amd_vi_gauss_log_prob(D, 1, _lib.ptr(phi), None, _lib.ptr(theta), n, _lib.ptr(log_q),
                                           stream) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(st.phi, phi) and st.status.tolist() == [0, 0, 0, 0]


# ---- step ---------------------------------------------------------------------------------------------------------
METHODS = [("rKL", {}), ("rKL", {"stick_the_landing": True}),
           ("IW", {"K": 1}), ("IW", {"K": 3}), ("IW", {"K": 8}), ("IW", {"K": 3, "stick_the_landing": True}),
           ("IW", {"K": 8, "dreg": True}),
           ("alpha", {"alpha": 0.5}), ("alpha", {"alpha": 2.0}), ("alpha", {"alpha": 0.5, "stick_the_landing": True}),
           ("alpha", {"alpha": 2.0, "dreg": True}), ("alpha", {"alpha": 0.5, "unbiased": True}),
           ("alpha", {"alpha": 2.0, "unbiased": True, "stick_the_landing": True}),
           ("fKL", {})]
SHAPES = [(1, 1), (2, 63), (5, 64), (16, 65), (5, 257), (16, 4097), (2, 4097), (1, 257), (16, 1), (5, 65), (2, 64),
          (16, 63)]


def step_cases():
    """Every method / flag combination meets four shapes; the shapes, families and link kinds cycle so that every D, n,
    family and link kind meets several methods."""
    cases = []
    shape_it, link_it, fam_it = itertools.cycle(SHAPES), itertools.cycle(LINKS), itertools.cycle([True, False, True])
    for method, kw in METHODS:
        for _ in range(4):
            D, n = next(shape_it)
            K = kw.get("K", 1)
            rows = n if K == 1 else max(n // K, 1) * K          # IW: whole groups (K = 3: 63, 258, 4095, ... rows)
            if K == 3 and n == 64:
                rows = 129                                       # 43 groups of 3: groups straddle the wave boundary
            cases.append(pytest.param(method, kw, D, rows, next(fam_it), next(link_it),
                                      id=f"{method}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'plain'}-D{D}-n{rows}"))
    return cases


@pytest.mark.parametrize("method,kw,D,n,full,link_kind", step_cases())
def test_step_gradient_determinism_and_update(method, kw, D, n, full, link_kind):
    c = build_case(D, n, full, link_kind, method, kw, base_seed=D * 7 + n)
    assert bool((c["g64"][c["live"]].abs() >= 1e-3).all())
    cfg = config(D, full, method, kw)
    g = torch.Generator().manual_seed(n + D)
    P = c["phi"].numel()
    m0 = (0.05 * torch.randn(P, generator=g)).to(DEV)
    v0 = (0.01 * torch.rand(P, generator=g)).to(DEV)
    lr, t = 3e-3 * 0.999**4, 7
    runs = []
    for _ in range(2):
        st = StepState(c["phi"], m0, v0)
        step(cfg, st, c["p"], c["r"], n, c["link_dev"], 1e9, lr, t, c["seed"], c["stp"])
        runs.append(st)
    a, b = runs
    for x, y in ((a.grad, b.grad), (a.phi, b.phi), (a.m, b.m), (a.v, b.v), (a.ring, b.ring)):
        assert torch.equal(x, y)                                           # two launches: the same bits
    within(a.grad, c["g64"], "gradient vs autograd in fp64")
    if full:
        assert bool((a.grad[~c["live"].to(DEV)] == 0).all())              # the strict upper triangle: exactly 0
    within(a.ring[t % RING], c["loss64"], "displayed loss")
    assert a.status.tolist() == [0, 0, t, 0] and bool((a.ring[torch.arange(RING) != t % RING] == -7.0).all())
    assert torch.equal(a.snap, c["phi"] + 0.125)
    # the clip coefficient is exactly 1: the same bits as the stand-alone clip + Adam on the exported gradient
    p_ref, m_ref, v_ref = c["phi"].clone(), m0.clone(), v0.clone()
    scratch = torch.zeros(256, device=DEV)
    assert lib().sbi_amd_adam_clip_step(_lib.ptr(p_ref), _lib.ptr(a.grad), _lib.ptr(m_ref), _lib.ptr(v_ref), P, t, lr,
                                        0.9, 0.999, 1e-8, 1e9, _lib.ptr(scratch),
                                        _lib.current_stream(p_ref.device)) == 0
    torch.cuda.synchronize()
    assert torch.equal(a.phi, p_ref) and torch.equal(a.m, m_ref) and torch.equal(a.v, v_ref)


@pytest.mark.parametrize("method,kw,D,n,full,link_kind", [
    ("rKL", {}, 5, 257, True, "interval"), ("IW", {"K": 8}, 16, 64, True, "mix"),
    ("alpha", {"alpha": 0.5}, 2, 65, False, "affine"), ("fKL", {}, 16, 4097, False, "lower")])
def test_clipped_update_against_the_oracle(method, kw, D, n, full, link_kind):
    c = build_case(D, n, full, link_kind, method, kw, base_seed=D + n + 1)
    norm = float(c["g64"].norm())
    clip = 0.25 * norm                                                     # active
    lr, gamma, sched = 1e-2, 0.999, 3
    st = StepState(c["phi"])
    step(config(D, full, method, kw), st, c["p"], c["r"], n, c["link_dev"], clip, lr * gamma**sched, 1, c["seed"],
         c["stp"])
    want = O.update(c["phi"], c["g64"], clip, lr, gamma=gamma, sched_steps=sched)
    within(st.phi, want, "phi after a clipped step")
    assert float((st.phi - c["phi"]).abs().max()) > 1e-3                   # (it moved)
    # t = 50: the snapshot is refreshed with the new phi
    st50 = StepState(c["phi"])
    step(config(D, full, method, kw), st50, c["p"], c["r"], n, c["link_dev"], clip, lr, 50, c["seed"], c["stp"])
    assert torch.equal(st50.snap, st50.phi) and st50.status.tolist() == [0, 1, 50, 0]


@pytest.mark.parametrize("method,kw", [("rKL", {}), ("IW", {"K": 8}), ("alpha", {"alpha": 0.5}), ("fKL", {})])
def test_non_finite_guard(method, kw):
    D, n, full = 5, 64, True
    c = build_case(D, n, full, "interval", method, kw, base_seed=3)
    p = c["p"].clone()
    p[17] = float("nan")
    g = torch.Generator().manual_seed(4)
    m0, v0 = torch.randn(c["phi"].numel(), generator=g).to(DEV), torch.rand(c["phi"].numel(), generator=g).to(DEV)
    st = StepState(c["phi"], m0, v0)
    step(config(D, full, method, kw), st, p, c["r"], n, c["link_dev"], 10.0, 1e-3, 4, c["seed"], c["stp"])
    assert torch.equal(st.phi, c["phi"] + 0.125)                           # = the snapshot
    assert bool((st.m == 0).all()) and bool((st.v == 0).all())
    assert st.status.tolist() == [1, 0, 0, 0]
    assert bool((st.ring == -7.0).all()) and bool((st.grad == -9.0).all()) and torch.equal(st.snap, c["phi"] + 0.125)
    step(config(D, full, method, kw), st, p, c["r"], n, c["link_dev"], 10.0, 1e-3, 5, c["seed"], c["stp"])
    assert st.status.tolist() == [2, 0, 0, 0]
