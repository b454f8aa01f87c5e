"""CPU: pins the longdouble reference of the point kernels (tests/sample_reference.py) against closed forms -- polynomial
fields of degree <= p come back at random points with their gradients, the quarter annulus has the radius 1 + xi_0 and the
radial direction as the exact normal of its circles, the closest-point iteration inverts the annulus (xi_0 = r - 1), projects
points off a lifted surface, and the location rule puts vertices where include/tigar_hip.h says."""
import numpy as np
import pytest

import postproc_reference as R
import sample_reference as S

LD = np.longdouble


def graded_patch(nels, p, seed=0):
    """an affine patch F = xi on graded element vertices: (vertices, control functions on the nodes, node coordinates)"""
    rng = np.random.default_rng(seed)
    uks = [np.concatenate([[0.0], np.cumsum(rng.uniform(0.3, 1.7, n))]) + 0.25 * k for k, n in enumerate(nels)]
    X = R.lagrange_nodes(uks, p)
    return uks, list(X) + [np.ones_like(X[0])], X


def lifted_annulus(nel):
    """the quarter annulus lifted into space: z = 0.4 x y (interpolated on the nodes)"""
    uks, cp = S.annulus_patch(nel)
    x, y = cp[0] / cp[2], cp[1] / cp[2]
    return uks, [cp[0], cp[1], 0.4 * x * y * cp[2], cp[2]]


@pytest.mark.parametrize("nels,p", [((5,), 3), ((3, 4), 2), ((2, 2), 5), ((2, 1, 3), 2), ((1, 2, 1), 4)])
def test_polynomials_are_reproduced(nels, p):
    d = len(nels)
    uks, cp, X = graded_patch(nels, p, seed=p)
    P = S.Patch(uks, p, cp)
    rng = np.random.default_rng(1)
    xi = np.stack([rng.uniform(u[0], u[-1], 40) for u in uks], axis=1)
    f = lambda x: np.prod([0.5 + (0.4 * x[k]) ** p - 0.2 * x[k] for k in range(d)], axis=0)
    out = P.eval(xi, [f(X)])
    exact = f([xi[:, k].astype(LD) for k in range(d)])
    # the nodal values and the node coordinates are doubles: eps / 2 each on sum_a |u_a phi_a|, and as much again through
    # f' times the shift of a node for a polynomial of degree p in each of d directions
    assert np.all(abs(out["val"][:, 0] - exact) <= (1 + p * d) * S.EPS * out["val_mag"][:, 0])
    h = 1e-6
    for k in range(d):                                 # the Cartesian gradient of an affine patch is the parametric one
        e = np.zeros(d)
        e[k] = h
        fd = (f((xi + e).T.astype(LD)) - f((xi - e).T.astype(LD))) / (2 * h)
        assert np.max(abs(out["grad"][:, 0, k] - fd)) < 1e-7 * (1 + np.max(abs(fd)))
    assert np.max(abs(out["x"] - xi)) <= S.EPS * np.max(abs(xi))       # (the node coordinates v + h a / p are rounded)
    assert np.all(out["val_mag"][:, 0] >= abs(out["val"][:, 0]) * (1 - 1e-15))


def test_rational_values_divide_by_the_weight():
    uks, cp = S.annulus_patch(4)
    P = S.Patch(uks, 2, cp)
    rng = np.random.default_rng(2)
    xi = rng.uniform(0, 1, (30, 2))
    u = rng.standard_normal(P.nnodes)
    plain, rat, w = P.eval(xi, [u]), P.eval(xi, [u], rational=True), P.eval(xi, [np.asarray(cp[2])])
    assert np.max(abs(rat["val"] - plain["val"] / w["val"])) < 1e-17
    # the weight function itself: u / W = 1 with zero gradient
    one = P.eval(xi, [np.asarray(cp[2])], rational=True)
    assert np.max(abs(one["val"] - 1)) < 1e-18 and np.max(abs(one["grad"])) < 1e-15


def test_annulus_radius_and_normals():
    uks, cp = S.annulus_patch(4)
    P = S.Patch(uks, 2, cp)
    rng = np.random.default_rng(3)
    xi = rng.uniform(0, 1, (50, 2))
    out = P.eval(xi)
    x = out["x"]
    r = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)
    # the control net is held in double (1 / sqrt(2), the refined net): a few eps / 2 on coordinates up to 2
    assert np.max(abs(r - (1 + xi[:, 0].astype(LD)))) <= 8 * S.EPS
    DF = out["DF"]
    n = x / r[:, None]
    # a perturbation eps of the nodal values passes into a derivative with the factor sum_a |l_a'| / h <= 2 p^2 nel = 32
    assert np.max(abs(DF[:, :, 0] - n)) < 32 * 8 * S.EPS               # d F / d xi_0 is the unit radial normal of the circles
    assert np.max(abs(np.einsum("qi,qi->q", DF[:, :, 1], n))) < 32 * 8 * S.EPS   # ... and the circles' tangent is orthogonal to it
    # the radial derivative of a function of r alone, by the Cartesian gradient
    X = np.stack([np.asarray(cp[i]) / np.asarray(cp[2]) for i in range(2)], axis=1)
    rn = np.hypot(X[:, 0], X[:, 1])
    g = P.eval(xi, [rn * np.asarray(cp[2])], rational=True)            # (r is linear in xi_0: exact in the rational space)
    assert np.max(abs(g["val"][:, 0] - r)) <= 8 * S.EPS
    assert np.max(abs(g["grad"][:, 0] - n)) < 32 * 16 * S.EPS


def test_location_rule_at_vertices():
    v = np.array([0.0, 0.25, 1.0, 1.5])
    inside, e = S.element_of(v, v)
    assert inside.all() and e.tolist() == [0, 1, 2, 2]                 # interior vertices: the upper element; the last: the last
    pts = np.array([np.nextafter(0.0, -1), np.nextafter(1.5, 2), np.nan, np.inf, -np.inf, np.nextafter(0.25, 0), np.nextafter(1.5, 0)])
    inside, e = S.element_of(v, pts)
    assert inside.tolist() == [False, False, False, False, False, True, True]
    assert e[5] == 0 and e[6] == 2
    uks, cp, _ = graded_patch((3, 2), 2)
    P = S.Patch(uks, 2, cp)
    out = P.eval(np.array([[uks[0][1], uks[1][2]], [uks[0][0], np.nan], [uks[0][3], uks[1][0]]]))
    assert out["inside"].tolist() == [True, False, True]
    assert np.all(np.isnan(out["x"][1])) and np.array_equal(out["x"][[0, 2]].astype(np.float64), [[uks[0][1], uks[1][2]], [uks[0][3], uks[1][0]]])


@pytest.mark.parametrize("nel,max_seeds,most", [(4, 32768, 5), (7, 32768, 5), (7, 7, 6), (7, 1, 8)])
def test_inverse_map_of_the_annulus(nel, max_seeds, most):
    uks, cp = S.annulus_patch(nel)
    P = S.Patch(uks, 2, cp)
    rng = np.random.default_rng(nel)
    xi = rng.uniform(0, 1, (60, 2))
    xi[::5, 0] = rng.integers(0, 2, 12)                                # a fifth of them on faces
    xi[2::10, 1] = 1.0
    x = P.eval(xi)["x"].astype(np.float64)
    res = P.locate(x, tol=1e-13, max_iter=50, max_seeds=max_seeds)
    assert all(r[3] == 0 for r in res)
    assert max(r[2] for r in res) <= most          # (one seed: the centre of the corner element, up to 8 steps away)
    got = np.array([r[0] for r in res], dtype=LD)
    assert np.max(abs(got - xi)) <= 1.3e-15
    assert np.max(abs(got[:, 0] - (np.hypot(x[:, 0], x[:, 1]) - 1))) <= 1e-15       # the closed form xi_0 = r - 1
    assert max(float(r[1]) for r in res) <= 1e-15


@pytest.mark.parametrize("offset,most", [(0.05, 17), (0.2, 27)])
def test_projection_onto_the_lifted_annulus(offset, most):
    uks, cp = lifted_annulus(4)
    P = S.Patch(uks, 2, cp)
    rng = np.random.default_rng(5)
    xi = rng.uniform(0.05, 0.95, (25, 2))
    out = P.eval(xi)
    DF = out["DF"]
    nrm = np.cross(DF[:, :, 0], DF[:, :, 1])
    nrm = nrm / np.sqrt(np.sum(nrm * nrm, axis=1))[:, None]
    x = (out["x"] + offset * nrm).astype(np.float64)
    res = P.locate(x, tol=1e-12, max_iter=50)
    assert all(r[3] == 0 for r in res), [r[3] for r in res]
    assert max(r[2] for r in res) <= most
    got = np.array([r[0] for r in res], dtype=LD)
    assert np.max(abs(got - xi)) <= 1e-9                               # (the foot of the normal, up to tol rho / (1 - rho))
    assert np.max(abs(np.array([float(r[1]) for r in res]) - offset)) <= 1e-12
    assert max(r[4] for r in res) <= 0.5


def test_points_outside_the_annulus_project_onto_its_boundary():
    uks, cp = S.annulus_patch(4)
    P = S.Patch(uks, 2, cp)
    th = np.linspace(0.1, 1.4, 8)
    x = np.concatenate([0.6 * np.stack([np.cos(th), np.sin(th)], axis=1), 2.4 * np.stack([np.cos(th), np.sin(th)], axis=1),
                        [[1.5 * np.cos(-0.2), 1.5 * np.sin(-0.2)], [1.5 * np.cos(1.8), 1.5 * np.sin(1.8)]]])
    res = P.locate(x, tol=1e-12, max_iter=50)
    assert all(r[3] == 0 for r in res), [(r[2], r[3]) for r in res]
    got = np.array([r[0] for r in res], dtype=np.float64)
    assert np.all(got[:8, 0] == 0.0) and np.all(got[8:16, 0] == 1.0)   # held at the bound
    assert got[16, 1] == 0.0 and got[17, 1] == 1.0
    assert np.max(abs(np.array([float(r[1]) for r in res[:16]]) - 0.4)) < 1e-12
    assert max(r[2] for r in res) <= 43


def test_statuses():
    uks, cp = S.annulus_patch(4)
    P = S.Patch(uks, 2, cp)
    x = P.eval(np.array([[0.3, 0.6]]))["x"].astype(np.float64)
    assert P.locate(x, max_iter=1, max_seeds=1)[0][3] == 1             # the iteration limit
    assert P.locate(np.array([[np.nan, 1.0]]))[0][3] == 2
    assert P.locate(x, guess=np.array([[np.inf, 0.5]]))[0][3] == 2
    # a collapsed edge (all nodes of xi_0 = 0 coincide), hit exactly: DF^T DF is singular there
    uks, cpa, X = graded_patch((2, 2), 2)
    P = S.Patch(uks, 2, [X[0] * np.cos(X[1]), X[0] * np.sin(X[1]), np.ones_like(X[0])])
    r = P.locate(np.array([[0.0, 0.0]]), guess=np.array([[0.0, 0.5]]))[0]
    assert r[3] == 3


def test_lattice_reference_is_the_point_reference_on_the_lattice():
    uks, cp = S.annulus_patch(3)
    t = np.array([0.0, 0.3, 1.0])
    ref = S.lattice_reference(uks, 2, cp, t)
    out = S.Patch(uks, 2, cp).eval(S.lattice_xi(uks, t))
    assert np.max(abs(out["x"] - ref.x)) < 1e-15
    assert R.gauss01(3)[0].shape == (3,) and abs(float(R.gauss01(3)[0][1]) - 0.5) < 1e-18      # (put back)
