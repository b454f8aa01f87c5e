"""CPU: the host side of tigar_amd/timeIntegration.py (parameters, the linear-combination expressions, the time
bookkeeping) against closed forms, and the dense reference of the GPU tests (tests/timeint_reference.py) against exact
solutions of the 1-D linear-FE pair (K, M) with 15 unknowns: convergence orders, energy conservation of the midpoint
rule, annihilation of the top mode at RHO_INF = 0."""
import numpy as np
import pytest
import scipy.linalg

import timeint_reference as R


class _V(object):
    """stand-in for a vector: the expressions only need identity"""

    def __init__(self, name):
        self.name = name


def _integrator(rho, order, dt=0.1, t=0.0, first=False):
    from tigar_amd import timeIntegration as TI
    x = _V("x")
    old = [_V("x_old"), _V("xdot_old"), _V("xddot_old")][:order + 1]
    return TI.GeneralizedAlphaIntegrator(rho, dt, x, old, t=t, useFirstOrderAlphaM=first), x, old


# (RHO_INF, order, useFirstOrderAlphaM) -> (alpha_m, alpha_f, gamma, beta), worked out by hand from
# alpha_m = (2 - rho) / (1 + rho) [first order: (3 - rho) / (2 (1 + rho))], alpha_f = 1 / (1 + rho),
# gamma = 1/2 + alpha_m - alpha_f, beta = (1 + alpha_m - alpha_f)^2 / 4
CLOSED = {
    (0.0, 2, False): (2.0, 1.0, 1.5, 1.0),
    (0.5, 2, False): (1.0, 2.0 / 3.0, 5.0 / 6.0, 4.0 / 9.0),
    (1.0, 2, False): (0.5, 0.5, 0.5, 0.25),
    (0.0, 1, False): (1.5, 1.0, 1.0, 0.5625),
    (0.5, 1, False): (5.0 / 6.0, 2.0 / 3.0, 2.0 / 3.0, 49.0 / 144.0),
    (1.0, 1, False): (0.5, 0.5, 0.5, 0.25),
    (0.0, 2, True): (1.5, 1.0, 1.0, 0.5625),
    (0.5, 2, True): (5.0 / 6.0, 2.0 / 3.0, 2.0 / 3.0, 49.0 / 144.0),
    (1.0, 2, True): (0.5, 0.5, 0.5, 0.25),
}


@pytest.mark.parametrize("rho,order,first", sorted(CLOSED))
def test_parameters_closed_form(rho, order, first):
    it, _, _ = _integrator(rho, order, first=first)
    assert it.systemOrder == order
    got = (it.ALPHA_M, it.ALPHA_F, it.GAMMA, it.BETA)
    # (gamma is a sum of three numbers of size <= 2 that cancel to ~0.5: two roundings of 2 eps absolute, 8 eps relative;
    #  beta squares such a sum: twice that)
    assert np.allclose(got, CLOSED[(rho, order, first)], rtol=16 * R.EPS, atol=0)
    assert np.allclose(got, R.parameters(rho, order, first), rtol=16 * R.EPS, atol=0)


def _coefs(expr, vectors):
    return [expr.coefficient(v) for v in vectors]


@pytest.mark.parametrize("rho", [0.0, 0.5, 1.0])
def test_rate_expressions_second_order(rho):
    dt = 0.05
    it, x, old = _integrator(rho, 2, dt=dt)
    g, b = it.GAMMA, it.BETA
    c, rest = it.xdot().split(x)
    assert np.isclose(c, g / (b * dt), rtol=1e-15)
    assert rest.coefficient(x) == 0 and len(rest.terms) == 3
    assert np.allclose(_coefs(rest, old), [-g / (b * dt), 1 - g / b, dt * (1 - g / (2 * b))], rtol=1e-14, atol=1e-16)
    c, rest = it.xddot().split(x)
    assert np.isclose(c, 1 / (b * dt * dt), rtol=1e-14)
    assert np.allclose(_coefs(rest, old), [-1 / (b * dt * dt), -1 / (b * dt), 1 - 1 / (2 * b)], rtol=1e-13, atol=1e-13)
    # alpha levels
    am, af = it.ALPHA_M, it.ALPHA_F
    assert np.allclose(_coefs(it.x_alpha(), [x] + old), [af, 1 - af, 0, 0])
    assert np.isclose(it.xdot_alpha().coefficient(x), af * g / (b * dt))
    assert np.isclose(it.xddot_alpha().coefficient(x), am / (b * dt * dt))
    assert np.isclose(it.xddot_alpha().coefficient(old[2]), am * (1 - 1 / (2 * b)) + 1 - am)
    # predictor: the x that makes xdot() equal xdot_old
    pred = it.sameVelocityPredictor()
    v = it.xdot()
    cx = v.coefficient(x)
    for k, w in enumerate(old):
        want = (1.0 if k == 1 else 0.0)
        assert np.isclose(cx * pred.coefficient(w) + v.coefficient(w), want, atol=1e-13)


@pytest.mark.parametrize("rho", [0.0, 0.5, 1.0])
def test_rate_expressions_first_order(rho):
    dt = 0.05
    it, x, old = _integrator(rho, 1, dt=dt)
    g = it.GAMMA
    c, rest = it.xdot().split(x)
    assert np.isclose(c, 1 / (g * dt))
    assert np.allclose(_coefs(rest, old), [-1 / (g * dt), (g - 1) / g])
    assert np.isclose(it.xdot_alpha().coefficient(x), it.ALPHA_M / (g * dt))
    pred = it.sameVelocityPredictor()
    assert pred.coefficient(old[0]) == 1.0 and len(pred.terms) == 1


def test_linear_combination_algebra():
    from tigar_amd.timeIntegration import LinearCombination as LC, x_alpha
    a, b, c = _V("a"), _V("b"), _V("c")
    e = 2.0 * LC.of(a) + b - 0.5 * (LC.of(a) - c) * 4.0
    assert [v.name for _, v in e.terms] == ["a", "b", "c"]          # merged, first appearance
    assert _coefs(e, [a, b, c]) == [0.0, 1.0, 2.0]
    k, rest = e.split(b)
    assert k == 1.0 and [v.name for _, v in rest.terms] == ["a", "c"]
    assert _coefs(-e / 2.0, [a, b, c]) == [-0.0, -0.5, -1.0]
    assert _coefs(a - LC.of(b), [a, b]) == [1.0, -1.0]
    assert _coefs(x_alpha(0.25, a, b), [a, b]) == [0.25, 0.75]
    with pytest.raises(TypeError):
        LC.of(a) * LC.of(b)


def test_backward_euler_expressions():
    from tigar_amd import timeIntegration as TI
    x, xo, vo = _V("x"), _V("xo"), _V("vo")
    it = TI.BackwardEulerIntegrator(0.25, x, [xo, vo], t=1.0)
    assert it.systemOrder == 2 and it.t == 1.25
    assert _coefs(it.xdot(), [x, xo, vo]) == [4.0, -4.0, 0.0]
    assert _coefs(it.xddot(), [x, xo, vo]) == [16.0, -16.0, -4.0]
    assert TI.BackwardEulerIntegrator(0.25, x, [xo]).systemOrder == 1


def test_time_bookkeeping(monkeypatch):
    from tigar_amd import timeIntegration as TI
    calls = []
    monkeypatch.setattr(TI._dev, "state_advance", lambda c, *vecs: calls.append((list(c), vecs)))
    it, x, old = _integrator(0.5, 2, dt=0.125, t=2.0)
    assert it.t == 2.125
    it.advance()
    it.advance()
    assert it.t == 2.375 and len(calls) == 2
    c, vecs = calls[0]
    assert len(c) == 7 and vecs == (x, old[0], old[1], old[2])
    assert np.allclose(c[:4], _coefs(it.xdot(), [x] + old))
    it1, x1, old1 = _integrator(0.5, 1, dt=0.125)
    it1.advance()
    assert len(calls[-1][1]) == 3 and calls[-1][0][3:] == [0.0, 0.0, 0.0, 0.0]
    ls = TI.LoadStepper(0.5, t=1.0)
    assert ls.t == 1.5 and ls.tval == 1.5
    ls.advance()
    assert ls.t == 2.0 and ls.tval == 2.0 and isinstance(ls.t, float)


# ---- the dense reference itself ---------------------------------------------------------------------------------------
N = 15


@pytest.fixture(scope="module")
def pair():
    K, M = R.fe_pair_1d(N)
    lam, Q = scipy.linalg.eigh(K, M)            # Q^T M Q = I
    return K, M, lam, Q


def test_reference_cholesky():
    K, M = R.fe_pair_1d(N)
    A = (K + 3.0 * M).astype(R.LD)
    L = R.cholesky(A)
    assert L.dtype == R.LD
    b = np.arange(1, N + 1, dtype=R.LD)
    x = R.cho_solve(L, b)
    assert float(np.max(np.abs(A @ x - b))) < 1e-15 * float(np.max(np.abs(b))) * np.linalg.cond(K + 3.0 * M)


@pytest.mark.parametrize("rho", [1.0, 0.5, 0.0])
def test_reference_wave_second_order(pair, rho):
    K, M, lam, Q = pair
    T = 0.5
    c = np.array([1.0, 0.5])
    x0 = Q[:, :2] @ c
    exact = Q[:, :2] @ (c * np.cos(np.sqrt(lam[:2]) * T))
    errs = []
    for steps in (100, 200, 400):
        out = R.integrate(K, M, T / steps, steps, order=2, rho_inf=rho, x0=x0)
        errs.append(np.linalg.norm(out["x"][-1] - exact))
    rates = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print("rho_inf %g: errors %s rates %s" % (rho, errs, rates))
    assert min(rates) >= 1.9


@pytest.mark.parametrize("rho", [1.0, 0.5, 0.0])
def test_reference_heat_second_order(pair, rho):
    K, M, lam, Q = pair
    T = 0.05
    c = np.array([1.0, 0.5])
    x0 = Q[:, :2] @ c
    exact = Q[:, :2] @ (c * np.exp(-lam[:2] * T))
    errs = []
    for steps in (40, 80, 160):
        out = R.integrate(K, M, T / steps, steps, order=1, rho_inf=rho, x0=x0)
        errs.append(np.linalg.norm(out["x"][-1] - exact))
    rates = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print("rho_inf %g: errors %s rates %s" % (rho, errs, rates))
    assert min(rates) >= 1.9


def test_reference_backward_euler_first_order_accurate(pair):
    K, M, lam, Q = pair
    T = 0.05
    x0 = Q[:, 0]
    for order in (1, 2):
        exact = x0 * (np.exp(-lam[0] * T) if order == 1 else np.cos(np.sqrt(lam[0]) * T))
        errs = []
        for steps in (80, 160, 320):
            out = R.integrate(K, M, T / steps, steps, order=order, scheme="backward_euler", x0=x0)
            errs.append(np.linalg.norm(out["x"][-1] - exact))
        rates = [np.log2(errs[i] / errs[i + 1]) for i in range(2)]
        assert 0.9 <= min(rates) and max(rates) <= 1.1


def test_reference_midpoint_conserves_energy(pair):
    K, M, lam, Q = pair
    rng = np.random.default_rng(5)
    x0, v0 = rng.standard_normal(N), rng.standard_normal(N) * 10.0
    out = R.integrate(K, M, 0.01, 200, order=2, rho_inf=1.0, x0=x0, v0=v0)
    e = np.array([R.energy(K, M, x, v) for x, v in zip(out["x"], out["v"])])
    drift = np.max(np.abs(e - e[0])) / e[0]
    print("relative energy drift over 200 steps: %.2e" % drift)
    assert drift <= 1e-12


def test_reference_top_mode_annihilated(pair):
    K, M, lam, Q = pair
    dt = 1e3 / np.sqrt(lam[-1])
    x0 = Q[:, -1]
    out = R.integrate(K, M, dt, 4, order=2, rho_inf=0.0, x0=x0)
    e = [R.energy(K, M, x, v) for x, v in zip(out["x"], out["v"])]
    print("energy of the top mode, RHO_INF = 0:", [v / e[0] for v in e])
    assert e[4] < 1e-6 * e[0]
    out = R.integrate(K, M, dt, 4, order=2, rho_inf=1.0, x0=x0)
    e1 = [R.energy(K, M, x, v) for x, v in zip(out["x"], out["v"])]
    assert np.allclose(np.array(e1) / e1[0], 1.0, rtol=1e-9)


def test_reference_longdouble_agrees(pair):
    K, M, lam, Q = pair
    rng = np.random.default_rng(6)
    x0 = rng.standard_normal(N)
    load = lambda t: np.sin(3.0 * t) * np.ones(N)
    for order, scheme in ((2, "generalized_alpha"), (1, "generalized_alpha"), (2, "backward_euler"), (1, "backward_euler")):
        kw = dict(order=order, scheme=scheme, rho_inf=0.5, load=load, x0=x0, damping=(0.1, 0.01) if order == 2 else None)
        a = R.integrate(K, M, 0.01, 20, dtype=np.float64, **kw)
        b = R.integrate(K, M, 0.01, 20, dtype=R.LD, **kw)
        assert b["x"][-1].dtype == R.LD
        err = max(float(np.linalg.norm(p - q)) for p, q in zip(a["x"], b["x"])) / max(float(np.linalg.norm(q)) for q in b["x"])
        assert 0 < err < 1e-12
