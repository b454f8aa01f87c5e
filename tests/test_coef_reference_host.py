"""CPU: the host reference of the forms with point coefficients (tests/coef_reference.py) against facts that do not depend
on it -- the matrices of the references that came before it, the divergence theorem on a box, and the identity
R(u) = J u - load of a law that is linear in (u, grad u).
"""
import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R
import rational_reference as RR
import coef_reference as CR

TOL = 1e-12


def _dense_close(D, Ao, tol=TOL):
    Ao = np.asarray(Ao.todense())
    return np.max(np.abs(D.astype(np.float64) - Ao)) <= tol * np.max(np.abs(Ao))


@pytest.mark.parametrize("name", ["annulus", "volume"])
def test_constant_coefficients_reproduce_the_earlier_references(name):
    uks, cp = R.annulus_patch(3) if name == "annulus" else R.volume_patch(2, (2, 1, 2))
    p = 2
    cp = [np.asarray(c, dtype=np.float64) for c in cp]
    Mo, Ko, _ = O.mapped_fe_system(uks, p, cp)
    Mr, Kr, _, _ = RR.rational_fe_system(uks, p, cp)
    for dtype in (CR.LD, np.float64):
        plain = CR.CoefReference(uks, p, cp, dtype=dtype)
        assert _dense_close(plain.dense(1.0), Ko) and _dense_close(plain.dense(None, None, None, 1.0), Mo)
        nsd = len(cp) - 1
        eye = np.tile(np.eye(nsd), (plain.npts, 1, 1))
        assert _dense_close(plain.dense(eye), Ko)                     # the tensor route of the same form
        rat = CR.CoefReference(uks, p, cp, rational=True, dtype=dtype)
        assert _dense_close(rat.dense(1.0), Kr) and _dense_close(rat.dense(None, None, None, 1.0), Mr)
    # points and weights are those of the quadrature-point reference
    ref = R.Reference(uks, p, cp)
    assert np.max(np.abs(plain.x - ref.x.astype(np.float64))) <= 1e-14
    assert np.max(np.abs(plain.wdet() - ref.wdet.astype(np.float64))) <= 1e-14
    # the flux load of F = grad of a nodal field is the stiffness matrix times the field; the source load is the point load
    u = np.sin(np.arange(plain.nnodes, dtype=np.float64))
    _, g = plain.eval(u)
    assert np.max(np.abs(plain.load(None, g) - Ko @ u)) <= TOL * np.max(np.abs(Ko @ u))
    fq = np.cos(np.arange(plain.npts, dtype=np.float64))
    assert np.max(np.abs(plain.load(fq) - ref.load(fq)[0].astype(np.float64))) <= TOL * np.max(np.abs(fq))


@pytest.mark.parametrize("d", [1, 2, 3])
def test_advection_terms_cancel_inside_a_box(d):
    """B_ab = int (b . grad phi_a) phi_b, C_ab = int phi_a (b . grad phi_b) with one constant b on an affine box:
    (B + C)_ab = int b . grad(phi_a phi_b) = boundary integral of (b . n) phi_a phi_b, which vanishes when a or b is an
    interior node.  nq = p + 1 integrates the degree-2p integrand exactly."""
    p, nels = 2, (3, 2, 2)[:d]
    uks = [np.linspace(0.0, 1.0 + 0.5 * k, nels[k] + 1) ** 1.3 for k in range(d)]
    X = R.lagrange_nodes(uks, p)
    lin = np.array([[2.0, 0.3, -0.1], [0.2, 1.5, 0.4], [-0.3, 0.1, 0.8]])[:d, :d]      # an affine map
    cp = [sum(lin[i, k] * X[k] for k in range(d)) + 0.1 * i for i in range(d)] + [np.ones_like(X[0])]
    ref = CR.CoefReference(uks, p, cp, dtype=np.float64)
    bvec = np.array([0.7, -1.1, 0.4])[:d]
    S = ref.dense(None, bvec, bvec, None)
    n = [e * p + 1 for e in nels]
    idx = np.array(np.unravel_index(np.arange(ref.nnodes), n, order="F")).T
    interior = np.all((idx > 0) & (idx < np.array(n) - 1), axis=1)
    assert interior.any() and not interior.all()
    scale = np.max(np.abs(ref.dense(None, bvec, None, None)))
    assert np.max(np.abs(S[interior, :])) <= TOL * scale and np.max(np.abs(S[:, interior])) <= TOL * scale
    assert np.max(np.abs(S)) > 1e-3 * scale                             # ... and does not vanish on the boundary


@pytest.mark.parametrize("rational", [False, True])
def test_linear_law_residual_is_the_tangent_times_u_minus_the_load(rational):
    uks, cp = R.annulus_patch(2)
    cp = [np.asarray(c, dtype=np.float64) for c in cp]
    ref = CR.CoefReference(uks, 2, cp, rational=rational, dtype=np.float64)
    rng = np.random.default_rng(5)
    npts, nsd = ref.npts, ref.nsd
    A, b = rng.standard_normal((npts, nsd, nsd)), rng.standard_normal((npts, nsd))
    c, m, f = rng.standard_normal((npts, nsd)), rng.standard_normal(npts), rng.standard_normal(npts)
    u = rng.standard_normal(ref.nnodes)
    uq, gq = ref.eval(u)
    flux = np.einsum("qij,qj->qi", A, gq) + b * uq[:, None]
    source = np.einsum("qi,qi->q", c, gq) + m * uq
    Rv = ref.load(source - f, flux)
    want = ref.dense(A, b, c, m) @ u - ref.load(f)
    assert np.max(np.abs(Rv - want)) <= TOL * np.max(np.abs(want))


def test_host_newton_flow_converges_quadratically():
    """-div(grad u / sqrt(1 + |grad u|^2)) + u^3 = f on the quarter annulus, the problem of tests/test_gpu_coef.py"""
    import coef_problem as P
    U, hist, errs = P.host_flow(4)
    assert hist[-1] < 1e-10 and len(hist) <= 8
    assert hist[-1] <= 1e-3 * hist[-2]                                  # the last step is in the quadratic regime
    assert errs[0] < 2e-2 and errs[1] < 3e-1
