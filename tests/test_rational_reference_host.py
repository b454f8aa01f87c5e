"""CPU: the host reference of the rational forms (tests/rational_reference.py) against facts that do not depend on it.

In the rational space psi_a = phi_a / W_h the nodal field w (the weights themselves) is the constant 1 and w_i l(P_i) is
the linear function l(x) -- exactly, because W_h and W_h x are the interpolants of w and w P.  Hence K_rat w = 0,
w^T M_rat w = b_rat(1) . w = the measure of the patch, and the rational elasticity form annihilates the rigid motions.
The forms are homogeneous of degree -2 (matrices) and -1 (load) in the control functions.
"""
import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R
import rational_reference as RR

TOL = 1e-12


def _patch(name):
    if name == "annulus":
        uks, cp = R.annulus_patch(3)
        return uks, 2, [np.asarray(c) for c in cp]
    uks, cp = R.volume_patch(2, (2, 2, 2))
    return uks, 2, [np.asarray(c) for c in cp]


@pytest.fixture(scope="module", params=["annulus", "volume"])
def case(request):
    uks, p, cp = _patch(request.param)
    x = RR.physical_nodes(cp)
    fn = np.sin(2.0 * x[:, 0]) + x[:, -1] ** 2
    M, K, b, _ = RR.rational_fe_system(uks, p, cp, fnodal=fn)
    return {"uks": uks, "p": p, "cp": cp, "x": x, "fn": fn, "M": M, "K": K, "b": b, "w": cp[-1]}


def _close(A, B, tol=TOL):
    A, B = A.tocsr(), B.tocsr()
    return abs(A - B).max() <= tol * abs(B).max()


def _measure(c):
    return float(np.sum(R.Reference(c["uks"], c["p"], c["cp"]).wdet))


def test_weights_vary(case):
    assert case["w"].max() - case["w"].min() > 0.05


def test_unit_weights_reproduce_the_oracle(case):
    uks, p, cp = case["uks"], case["p"], case["cp"]
    one = [c / cp[-1] for c in cp]                                    # the same nodes, unit weights
    M, K, b, _ = RR.rational_fe_system(uks, p, one, fnodal=case["fn"])
    Mo, Ko, bo = O.mapped_fe_system(uks, p, one, fnodal=case["fn"])
    assert _close(M, Mo) and _close(K, Ko)
    assert np.max(abs(b - bo)) <= TOL * np.max(abs(bo))
    A = RR.rational_elasticity_fe_system(uks, p, one, 1.3, 0.7)
    assert _close(A, O.mapped_elasticity_fe_system(uks, p, one, 1.3, 0.7))


def test_stiffness_annihilates_the_weights(case):
    K, w = case["K"], case["w"]
    assert np.max(abs(K @ w)) <= TOL * abs(K).max()
    # ... which the un-rationalised matrix does not: the two spaces differ
    Ko = O.mapped_fe_system(case["uks"], case["p"], case["cp"])[1]
    assert np.max(abs(Ko @ w)) > 1e-4 * abs(Ko).max()


def test_mass_and_load_of_one_give_the_measure(case):
    w, vol = case["w"], _measure(case)
    assert abs(w @ (case["M"] @ w) - vol) <= TOL * vol
    b1 = RR.rational_fe_system(case["uks"], case["p"], case["cp"], fnodal=np.ones_like(w))[2]
    assert abs(b1 @ w - vol) <= TOL * vol


def test_symmetry(case):
    for A in (case["K"], case["M"]):
        T = A.T.tocsr()
        T.sort_indices()
        assert np.array_equal(T.indptr, A.indptr) and np.array_equal(T.indices, A.indices)
        assert np.max(abs(T.data - A.data)) <= TOL * abs(A).max()


def test_homogeneity_in_the_control_functions(case):
    uks, p, cp = case["uks"], case["p"], case["cp"]
    M2, K2, b2, _ = RR.rational_fe_system(uks, p, [2.0 * c for c in cp], fnodal=case["fn"])
    assert _close(M2, case["M"] / 4.0) and _close(K2, case["K"] / 4.0)
    assert np.max(abs(b2 - case["b"] / 2.0)) <= TOL * np.max(abs(case["b"]))


def test_linear_functions_are_reproduced(case):
    # U_i = w_i l(P_i) is l(x) in the rational space: its error sums vanish, those of the un-rationalised reading do not
    x, w = case["x"], case["w"]
    coef = np.array([2.0, -1.0, 0.5])[:x.shape[1]]
    U = w * (1.0 + x @ coef)
    pts = RR.RationalPoints(case["uks"], case["p"], case["cp"])
    xq = np.asarray(pts.x, dtype=np.float64)
    (s0, s1, e2), _ = pts.sums_rational(U, 1.0 + xq @ coef, np.tile(coef, (pts.npts, 1)))
    assert np.sqrt(float(s0 + s1)) <= 1e-13 * np.sqrt(float(e2))
    (t0, t1, _), _ = pts.sums(U, 1.0 + xq @ coef, np.tile(coef, (pts.npts, 1)))
    assert np.sqrt(float(t0 + t1)) > 1e-3 * np.sqrt(float(e2))


def test_elasticity_annihilates_the_rigid_motions(case):
    uks, p, cp, x, w = case["uks"], case["p"], case["cp"], case["x"], case["w"]
    d = len(uks)
    A = RR.rational_elasticity_fe_system(uks, p, cp, 1.3, 0.7)
    modes = []
    for i in range(d):                                                # translations
        r = np.zeros((d, len(w)))
        r[i] = 1.0
        modes.append(r)
    for i in range(d):                                                # rotations in the planes (i, j)
        for j in range(i + 1, d):
            r = np.zeros((d, len(w)))
            r[i], r[j] = -x[:, j], x[:, i]
            modes.append(r)
    assert len(modes) == (3 if d == 2 else 6)
    for r in modes:
        assert np.max(abs(A @ (w[None, :] * r).ravel())) <= TOL * abs(A).max()
    # the un-rationalised form does not hold the rotations
    Ao = O.mapped_elasticity_fe_system(uks, p, cp, 1.3, 0.7)
    assert np.max(abs(Ao @ (w[None, :] * modes[-1]).ravel())) > 1e-4 * abs(Ao).max()


def test_point_load_of_an_interpolant_is_the_nodal_load(case):
    pts = RR.RationalPoints(case["uks"], case["p"], case["cp"])
    fq = pts.eval(case["fn"])[0]
    b = pts.load_rational(fq).astype(np.float64)
    assert np.max(abs(b - case["b"])) <= TOL * np.max(abs(case["b"]))
    c = RR.rational_fe_system(case["uks"], case["p"], case["cp"], fq=np.asarray(fq, dtype=np.float64))[3]
    assert np.max(abs(c - case["b"])) <= TOL * np.max(abs(case["b"]))


def test_annulus_poisson_converges_in_the_rational_space():
    errs = [RR.solve_annulus_poisson(nel) for nel in (4, 8)]
    assert errs[0][0] / errs[1][0] >= 7.0 and errs[0][1] / errs[1][1] >= 3.5
