"""Host: pins tests/dynamics_reference.py before anything on the GPU is held against it (no GPU, no library call), and checks
the conditions under which the cases and flows of tests/test_gpu_dynamics.py were chosen.

Central differences follow the rule of tests/test_jet_reference_host.py: the truncation term is taken from the reference
itself (2 x the difference between the steps h and h/2), the rounding term is 8 eps_longdouble max|f| / h.
"""
import json
import os

import numpy as np
import pytest

import dynamics_reference as DR
from tigar_amd import timeIntegration as TI

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_cases_meet_their_conditions_and_tangent_against_differences(name):
    """in the reference between 20 % and 80 % of the points are active, no point has |g| below 1e-6 of the patch size, the law
    is admissible at y and y_alpha; away from g = 0 the tangent times w equals the central difference of the residual along w
    in longdouble"""
    c = DR.assembled_case(name, dtypes=(LD,))
    d, y, old = c["dyn"][0], c["y"], c["old"]
    ya = d.levels(y, old)[0]
    g = d.gap(ya)
    size = float(np.max(np.max(d.X, axis=0) - np.min(d.X, axis=0)))
    active = d.active(y, old)
    print("%s: %d of %d points active, min |g| / size %.2e" % (name, active, g.size, float(np.min(abs(g))) / size))
    assert 0.2 * g.size <= active <= 0.8 * g.size
    assert float(np.min(abs(g))) >= 1e-6 * size
    d.base.state(y, c["material"]), d.base.state(ya, c["material"])          # (an inadmissible state raises)
    rng = np.random.default_rng(3)
    w = (DR.CASE_NOISE * rng.standard_normal(y.size)).astype(LD)
    # the perturbation h w moves no point further than a quarter of the smallest |g|: the residual is smooth along it
    reach = d.alpha_f * float(np.max(np.sqrt(np.sum(d.values(w) ** 2, axis=1))))
    h = LD(min(1e-3, 0.25 * float(np.min(abs(g))) / reach))
    K = d.tangent(y, old)
    r = lambda s: d.residual(y.astype(LD) + s * w, old)
    R0 = r(LD(0))
    t1, t2 = (r(h) - r(-h)) / (2 * h), (r(h / 2) - r(-h / 2)) / h
    bound = 2 * float(np.max(np.abs(t1 - t2))) + 8 * EPS_LD * float(np.max(np.abs(R0))) / float(h)
    err = float(np.max(np.abs(t2 - K @ w)))
    print("%s: |K w - difference| %.2e, bound %.2e, max |K w| %.2e" % (name, err, bound, float(np.max(np.abs(K @ w)))))
    assert err <= bound
    assert bound <= 1e-6 * float(np.max(np.abs(K @ w)))                       # (the check has teeth)


class _V(object):
    """a host stand-in for a vector: the integrators only compare identities"""


@pytest.mark.parametrize("rho_inf", [0.0, 0.5, 1.0])
def test_coefficients_against_split(rho_inf):
    """c_a = alpha_m / (beta dt^2) and c_v = alpha_f gamma / (beta dt) typed in the reference equal the coefficients of the
    unknown in ``xddot_alpha()`` and ``xdot_alpha()`` of the integrator, and the reference's constants are the integrator's"""
    dt = 0.37
    y, old = _V(), [_V(), _V(), _V()]
    it = TI.GeneralizedAlphaIntegrator(rho_inf, dt, y, old)
    am, af, gamma, beta = DR.newmark(rho_inf)
    for mine, theirs in ((am, it.ALPHA_M), (af, it.ALPHA_F), (gamma, it.GAMMA), (beta, it.BETA)):
        assert abs(mine - theirs) <= 4 * np.finfo(float).eps * abs(theirs)
    c_a, rest = it.xddot_alpha().split(y)
    c_v = it.xdot_alpha().coefficient(y)
    assert abs(c_a - am / (beta * dt * dt)) <= 8 * np.finfo(float).eps * c_a
    assert abs(c_v - af * gamma / (beta * dt)) <= 8 * np.finfo(float).eps * c_v
    assert all(v is not y for _, v in rest.terms) and len(rest.terms) == 3
    be = TI.BackwardEulerIntegrator(dt, y, old[:2])
    assert abs(be.xddot().coefficient(y) - 1.0 / dt ** 2) <= 8 * np.finfo(float).eps / dt ** 2
    assert abs(be.xdot().coefficient(y) - 1.0 / dt) <= 8 * np.finfo(float).eps / dt


def _golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", DR.GOLDEN_FLOWS)) as f:
        return json.load(f)


def _same_flow(rec, got, steps):
    assert abs(got["dt"] - rec["dt"]) <= 1e-12 * rec["dt"]
    assert got["iterations"] == rec["iterations"][:steps] and got["active"] == rec["active"][:steps]
    for k, U in got["U"].items():
        want = np.asarray(rec["U"][k])
        assert np.max(np.abs(np.asarray(U) - want)) <= 1e-9 * np.max(np.abs(want)), k
    for a, b in zip(got["energy"], rec["energy"]):
        assert abs(a - b) <= 1e-9 * abs(b)


def test_linear_flow_conserves_energy():
    """``LinearElastic``, RHO_INF = 1, no damping, no contact: the total energy of the float64 flow over 20 steps is constant;
    its drift -- 3.7e-16 of the energy when recorded -- is the yardstick of the device flow.  Every step takes one Newton step:
    the second norm is a rounding error."""
    rec = _golden()["linear-p2"]
    got = DR.flow_record("linear", 2)
    _same_flow(rec, got, DR.FLOW_STEPS["linear"])
    e = np.asarray(got["energy"])
    drift = float(np.max(np.abs(e - e[0])) / e[0])
    print("linear flow: energy %.12e, drift over 20 steps %.2e" % (e[0], drift))
    assert drift <= 64 * np.finfo(float).eps
    assert got["iterations"] == [2] * 20 and max(got["second_norm"]) <= 1e-12


@pytest.mark.parametrize("kind,p,steps", [("vibration", 2, None), ("vibration", 3, 1), ("obstacle", 2, None), ("solid", 2, None),
                                          ("euler", 2, 2)])
def test_flows_meet_their_conditions_and_the_record(kind, p, steps):
    """the recorded flows (tests/golden/dynamics_flows.json) are what the reference computes (all steps, or the first ones of
    the slower flows), within their iteration limits; the obstacle flow has a non-empty active set in at least two steps"""
    rec = _golden()["%s-p%d" % (kind, p)]
    got = DR.flow_record(kind, p, steps)
    _same_flow(rec, got, DR.FLOW_STEPS[kind] if steps is None else steps)
    assert len(rec["iterations"]) == DR.FLOW_STEPS[kind] and max(rec["iterations"]) <= DR.FLOW_MAX_ITERS[kind]
    assert sorted(int(k) for k in rec["U"]) == list(DR.FLOW_RECORD[kind])
    if kind == "obstacle":
        assert sum(1 for a in rec["active"] if a > 0) >= 2
        s = DR.flow_setup(kind, p)
        Mc = np.asarray(s["pb"]["Mc"].todense())
        n, off, _ = s["plane"]
        tip = lambda U: float(np.min((s["dyn"].X + s["dyn"].values(Mc @ U)) @ n))
        import shell_reference as SR
        Us = SR.strip_flow(p, s["material"])[1]
        assert abs((tip(np.zeros_like(Us)) - off) - 0.5 * (tip(np.zeros_like(Us)) - tip(Us))) <= 1e-12
    else:
        assert not any(rec["active"])


def test_second_order_in_time():
    """the strip released from its static solution, RHO_INF = 0.5, with the compatible initial acceleration: the error of the
    dofs at a fixed time T against the same flow at T / 8, for the steps T and T / 2 -- the ratio lies in [3.5, 4.5] (second
    order and the finite reference step give 63 / 15 = 4.2).
    The first choice, the step of the free-vibration flow (1/20 of the lowest linearised period T_1), is NOT in the asymptotic
    range: the strip is stiff -- its membrane modes lie far above the lowest bending mode -- and the ratio rises slowly, 2.4,
    3.0, 3.5, 3.9 at T = T_1 / 20, / 80, / 640, / 2560 (measured on the CPU).  So T = T_1 / 2560, and the flow runs in longdouble:
    at such steps the first residual norm of a step is so small that the float64 flow cannot reduce it by 1e-10."""
    import shell_reference as SR
    s = DR.flow_setup("vibration", 2)
    pb = s["pb"]
    base = SR.ShellReference(pb["uks"], 2, pb["cp"], rational=True, dtype=LD)
    ends = {}
    for div in (1, 2, 8):
        d = DR.DynamicsReference(base, s["material"], s["density"], s["dt"] / 128 / div, 0.5)
        ends[div] = DR.flow(d, pb["Mc"], s["free"], s["U0"], A0=s["A0"], steps=div, tol=1e-13, max_iters=10, record=(div,))["U"][div]
    e1, e2 = (float(np.max(np.abs(ends[div] - ends[8]))) for div in (1, 2))
    print("second order in time: errors %.3e (T), %.3e (T / 2), ratio %.3f" % (e1, e2, e1 / e2))
    assert 3.5 <= e1 / e2 <= 4.5
