"""Host: pins tests/jet_reference.py, tests/shell_reference.py and ``forms.KirchhoffLoveSVK.host`` before anything on the GPU
is held against them (no GPU, no library call).

Central differences: the error of (f(x + h) - f(x - h)) / 2h is h^2/6 |f'''| + eps |f| / h.  The truncation term is taken from
the reference itself -- the difference between the steps h and h/2 is 3/4 of the truncation error of h, so 2 x that difference
bounds it -- and the rounding term is 8 eps_longdouble max|f| / h; nothing in a bound comes from the law under test.
"""
import numpy as np
import pytest

import postproc_reference as R
import jet_reference as JR
import shell_reference as SR
from tigar_amd import forms as F

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
MAT = F.KirchhoffLoveSVK(SR.E_MOD, SR.NU, SR.THICKNESS)


def _point_parameters(uks, nq):
    """parametric coordinates [npts, d] of the quadrature points, element-major"""
    t, _ = R.gauss01(nq)
    d = len(uks)
    nel = [len(u) - 1 for u in uks]
    qs = np.array(np.unravel_index(np.arange(nq ** d), (nq,) * d, order="F")).T
    out = []
    for e in np.ndindex(*nel[::-1]):
        el = e[::-1]
        out.append(np.stack([LD(uks[k][el[k]]) + (LD(uks[k][el[k] + 1]) - LD(uks[k][el[k]])) * t[qs[:, k]] for k in range(d)], 1))
    return np.concatenate(out)


def _nodes_ld(uks, p):
    ax = []
    for u in uks:
        u = np.asarray(u).astype(LD)
        inner = u[:-1, None] + np.diff(u)[:, None] * (np.arange(1, p + 1).astype(LD) / LD(p))[None, :]
        ax.append(np.concatenate([[u[0]], inner.ravel()]))
    return [g.ravel(order="F") for g in np.meshgrid(*ax, indexing="ij")]


@pytest.mark.parametrize("d,nsd,p,nq", [(1, 2, 2, 3), (1, 3, 3, 2), (2, 2, 2, 3), (2, 3, 3, 4), (2, 3, 4, 1), (2, 2, 1, 2)])
def test_jets_of_polynomials_are_exact(d, nsd, p, nq):
    """a polynomial of degree <= p per direction in the parametric coordinates is in the space: its jet is its derivatives.  The
    rational space holds f = (W f) / W: the quotient rule gives the same jet back.  The coordinates of the polynomial map
    likewise.  Bound: nodal differences divided by h^2 lose (p / h_min)^2, so 64 (p / h_min)^2 eps_longdouble of the scale."""
    nels = (3,) if d == 1 else (3, 2)
    uks, cp = JR.polynomial_patch(nels, p, nsd, weighted=True)
    X = _nodes_ld(uks, p)
    xi = _point_parameters(uks, nq)
    a, b = xi[:, 0], xi[:, -1]
    if d == 1:
        f = lambda s, t: 1 + s - s ** p
        want = np.stack([1 + a - a ** p, 1 - p * a ** (p - 1), -p * (p - 1) * a ** max(p - 2, 0) * (p >= 2)], 1)
    else:
        q = min(p, 2)
        f = lambda s, t: 1 + s * t + s ** q - 2 * t ** q
        want = np.stack([f(a, b), b + q * a ** (q - 1), a - 2 * q * b ** (q - 1), q * (q - 1) * a ** 0 * (q == 2), a ** 0,
                         -2 * q * (q - 1) * a ** 0 * (q == 2)], 1)
    hmin = min(float(np.min(np.diff(u))) for u in uks)
    bound = 64 * (p / hmin) ** 2 * EPS_LD * float(np.max(np.abs(want)))
    ref = JR.JetReference(uks, p, cp, nq)
    err = float(np.max(np.abs(ref.jets(f(X[0], X[-1])) - want)))
    assert err <= bound, (err, bound)
    # rational: c W_h / W_h = c, and for a random nodal field v the jet of v_h / W_h times that of W_h gives the jet of v_h back
    # by the PRODUCT rule (the reference applies the quotient rule)
    rat = JR.JetReference(uks, p, cp, nq, rational=True)
    W = np.asarray(cp[-1]).astype(LD)
    Jc = rat.jets(3 * W)
    assert float(np.max(np.abs(Jc[:, 0] - 3))) <= bound and float(np.max(np.abs(Jc[:, 1:]))) <= bound
    v = np.random.default_rng(p + nq).standard_normal(W.size).astype(LD)
    Jr, Jv, JW = rat.jets(v), ref.jets(v), ref.jets(W)
    back = np.empty_like(Jv)
    back[:, 0] = Jr[:, 0] * JW[:, 0]
    for k in range(d):
        back[:, 1 + k] = Jr[:, 1 + k] * JW[:, 0] + Jr[:, 0] * JW[:, 1 + k]
    for s_, (k, m) in enumerate(JR.SLOTS[d]):
        back[:, 1 + d + s_] = Jr[:, 1 + d + s_] * JW[:, 0] + Jr[:, 1 + k] * JW[:, 1 + m] + Jr[:, 1 + m] * JW[:, 1 + k] + Jr[:, 0] * JW[:, 1 + d + s_]
    assert float(np.max(np.abs(back - Jv))) <= 64 * (p / hmin) ** 2 * EPS_LD * float(np.max(np.abs(Jv)))
    # the geometry of the unweighted patch is a polynomial map: x_0 = xi_0 + 0.1 xi_1^q (d = 2) -- first and second derivatives
    uks, cp = JR.polynomial_patch(nels, p, nsd, weighted=False)
    gj = JR.JetReference(uks, p, cp, nq).geometry_jets()
    q = 2 if p >= 2 else 1
    gb = 64 * (p / hmin) ** 2 * JR.EPS          # (the control functions are float64 data: their rounding is what is amplified)
    if d == 2:
        assert float(np.max(np.abs(gj[:, 0, 1] - 1))) <= gb and float(np.max(np.abs(gj[:, 0, 2] - 0.1 * q * b ** (q - 1)))) <= gb
        assert float(np.max(np.abs(gj[:, 0, 5] - 0.1 * q * (q - 1)))) <= gb and float(np.max(np.abs(gj[:, 0, 4]))) <= gb


def _random_jets(npts, seed, dtype=LD):
    """reference jets of a surface close to a stretched plane with curvature, displacement jets of a tenth of that"""
    rng = np.random.default_rng(seed)
    X = 0.3 * rng.standard_normal((npts, 3, 6))
    X[:, 0, 1] += 1.0
    X[:, 1, 2] += 1.2
    U = 0.05 * rng.standard_normal((npts, 3, 6))
    return X.astype(dtype), U.astype(dtype)


def test_demo_energy_is_the_curvilinear_energy():
    """psi as the demo writes it (Gram-Schmidt basis, Voigt D, curvature from -a_alpha . d_beta a_3) equals psi of the closed
    curvilinear form: two statements of one function, to 256 eps_longdouble of its size"""
    X, U = _random_jets(200, 1)
    psi = MAT.host(X, U)[0]
    demo = SR.demo_energy(X, U, MAT.E, MAT.nu, MAT.thickness)
    assert psi.dtype == LD
    assert float(np.max(np.abs(psi - demo))) <= 256 * EPS_LD * float(np.max(np.abs(demo)))


def _central(fun, U, i, a, h):
    dU = np.zeros_like(U)
    dU[:, i, a] = h
    return (fun(U + dU) - fun(U - dU)) / (2 * h)


def test_load_and_tangent_against_central_differences():
    """s = d psi / d jet(u) against differences of the DEMO's psi, T = d s / d jet(u) against differences of s, in longdouble"""
    X, U = _random_jets(50, 2)
    psi, s, T = MAT.host(X, U)
    demo = lambda V: SR.demo_energy(X, V, MAT.E, MAT.nu, MAT.thickness)
    load = lambda V: MAT.host(X, V)[1]
    h = LD(1e-5)
    worst = [0.0, 0.0]
    for i in range(3):
        assert float(np.max(np.abs(s[:, i, 0]))) == 0.0 and float(np.max(np.abs(T[:, i, 0]))) == 0.0       # the value slot
        for a in range(1, 6):
            d1, d2 = _central(demo, U, i, a, h), _central(demo, U, i, a, h / 2)
            bound = 2 * float(np.max(np.abs(d1 - d2))) + 8 * EPS_LD * float(np.max(np.abs(psi))) / float(h)
            err = float(np.max(np.abs(d2 - s[:, i, a])))
            worst[0] = max(worst[0], err / bound)
            assert err <= bound, ("s", i, a, err, bound)
            t1, t2 = _central(load, U, i, a, h), _central(load, U, i, a, h / 2)
            bound = 2 * float(np.max(np.abs(t1 - t2))) + 8 * EPS_LD * float(np.max(np.abs(s))) / float(h)
            err = float(np.max(np.abs(t2 - T[:, :, :, i, a])))
            worst[1] = max(worst[1], err / bound)
            assert err <= bound, ("T", i, a, err, bound)
    print("largest error / bound: s %.2e, T %.2e" % tuple(worst))


def test_tangent_has_major_symmetry():
    X, U = _random_jets(100, 3, np.float64)
    T = MAT.host(X, U)[2]
    assert T.dtype == np.float64
    assert float(np.max(np.abs(T - T.transpose(0, 3, 4, 1, 2)))) <= 64 * JR.EPS * float(np.max(np.abs(T)))


def _rotation(axis, angle):
    axis = np.asarray(axis, dtype=LD) / np.sqrt(np.sum(np.asarray(axis, dtype=LD) ** 2))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=LD)
    return np.eye(3, dtype=LD) + np.sin(LD(angle)) * K + (1 - np.cos(LD(angle))) * (K @ K)


def test_rigid_motion_costs_nothing():
    """u = (R - I) X + c: eps and kappa vanish to rounding.  eps is a difference of two numbers of size |X_,a|^2 and kappa of
    two of size |X_,ab|, each known to a few eps; n = h C eps and m = h^3/12 C kappa then reach s through x_,a and a_3: a
    bound of 1e3 eps_longdouble E h G^3 (1 + G), G = max |jet| -- and its square over E h for psi."""
    X, _ = _random_jets(100, 4)
    Rm = _rotation((1.0, 2.0, -0.5), 0.9)
    U = np.einsum("ij,qja->qia", Rm - np.eye(3, dtype=LD), X)
    U[:, :, 0] += np.array([0.3, -1.0, 2.0], dtype=LD)
    psi, s, T = MAT.host(X, U)
    G = float(np.max(np.abs(X)))
    bound = 1e3 * EPS_LD * MAT.E * MAT.thickness * G ** 3 * (1 + G)
    assert float(np.max(np.abs(s))) <= bound
    assert float(np.max(np.abs(psi))) <= bound * bound / (MAT.E * MAT.thickness)


def test_degenerate_points_are_counted():
    X, U = _random_jets(10, 5, np.float64)
    for q in (0, 4, 9):
        U[q, :, 2] = X[q, :, 1] + U[q, :, 1] - X[q, :, 2]           # x_,1 = x_,0
    assert int(np.sum(MAT.degenerate(X, U))) == 3
    with pytest.raises(RuntimeError, match="3 points"):
        MAT.host(X, U)


@pytest.mark.parametrize("surface", ["cylinder", "doubly_curved"])
def test_assembled_residual_and_tangent_against_differences(surface):
    """R . w against the difference of the assembled DEMO energy along w, K w against the difference of R, in longdouble"""
    hom = SR.cylinder_homogeneous() if surface == "cylinder" else SR.doubly_curved_homogeneous
    pb = SR.problem(2, (2, 2), hom)
    ref = SR.ShellReference(pb["uks"], 2, pb["cp"], rational=surface == "cylinder")
    rng = np.random.default_rng(6)
    u = (0.02 * rng.standard_normal(3 * ref.n)).astype(LD)
    w = rng.standard_normal(3 * ref.n).astype(LD)
    Rv, K = ref.residual(u, MAT), ref.tangent(u, MAT)
    assert float(np.max(np.abs(K - K.T))) <= 64 * EPS_LD * float(np.max(np.abs(K)))
    assert abs(ref.energy(u, MAT) - ref.law_energy(u, MAT)) <= 256 * EPS_LD * abs(ref.energy(u, MAT))
    h = LD(1e-5)
    e = lambda s: ref.energy(u + s * w, MAT)
    d1, d2 = (e(h) - e(-h)) / (2 * h), (e(h / 2) - e(-h / 2)) / h
    bound = 2 * abs(d1 - d2) + 8 * EPS_LD * abs(e(0)) / float(h)
    assert abs(d2 - Rv @ w) <= bound
    r = lambda s: ref.residual(u + s * w, MAT)
    t1, t2 = (r(h) - r(-h)) / (2 * h), (r(h / 2) - r(-h / 2)) / h
    bound = 2 * float(np.max(np.abs(t1 - t2))) + 8 * EPS_LD * float(np.max(np.abs(Rv))) / float(h)
    assert float(np.max(np.abs(t2 - K @ w))) <= bound


def test_body_force_enters_the_value_slot():
    pb = SR.problem(2, (2, 2), SR.cylinder_homogeneous())
    ref = SR.ShellReference(pb["uks"], 2, pb["cp"], rational=True, dtype=np.float64)
    u = np.zeros(3 * ref.n)
    f = np.array([0.5, -1.0, 2.0])
    r = ref.residual(u, MAT, f)
    # rational functions phi / W do not sum to one; the load of f against the function 1 = sum_a W_a phi_a / W does
    W = np.asarray(pb["cp"][3])
    got = -(r.reshape(3, ref.n) @ W)
    area = float(np.sum(ref.ref.wdet))
    assert np.allclose(got, f * area, rtol=1e-12)
    assert abs(area - 0.5 * np.pi * 1.5) <= 1e-6 * area           # a quarter cylinder of radius 1 and length 1.5
