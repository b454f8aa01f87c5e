"""CPU: the host reference of finite-strain elasticity (tests/hyper_reference.py) and the host laws of
``forms.LinearElastic`` / ``StVenantKirchhoff`` / ``NeoHookean`` pinned on their own, before any kernel is held to them:
the stress against central differences of the energy and the tangent against central differences of the stress, the major
symmetry of the tangent, objectivity, the linear law against the oracle's mapped elasticity, the assembled residual and
tangent against differences of the assembled energy and residual, and the two Newton flows of the GPU tests."""
import numpy as np
import pytest

from oracle import tigar_oracle as O
import postproc_reference as R
import hyper_reference as H

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
LAM, MU = 1.3, 0.7


@pytest.fixture(scope="module")
def F():
    from tigar_amd import forms
    return forms


def _laws(F):
    return [F.LinearElastic(LAM, MU), F.StVenantKirchhoff(LAM, MU), F.NeoHookean(LAM, MU)]


@pytest.mark.parametrize("n", [2, 3])
def test_stress_and_tangent_are_derivatives_of_the_energy(F, n):
    """Central differences in longdouble with step h = 1e-6 along the unit directions e_jL: the truncation term is h^2 / 6
    times the next-but-one derivative (``derivative_bounds`` at |F| <= 1.44, |F^-1| <= 1 / 0.7, |ln J| <= 1.1), the rounding
    term eps / h times the size of the differenced function (|psi|, |P| <= 4 (lambda + mu) there)."""
    Fm = H.random_F(n, 40, 11 + n).astype(LD)
    J = np.array([np.linalg.det(f.astype(np.float64)) for f in Fm])
    assert J.min() >= 0.3 and J.max() <= 3.0
    h = LD(1e-6)
    c3, c4 = H.derivative_bounds(LAM, MU, 1.44, 1.0 / 0.7, 1.1)
    size = 4.0 * (LAM + MU)
    bP, bA = (c * float(h) ** 2 / 6.0 + size * EPS_LD / float(h) for c in (c3, c4))
    bound = max(bP, bA)
    for law in _laws(F):
        P, A, psi = law.host(Fm)
        assert P.dtype == LD and A.dtype == LD and psi.dtype == LD
        eP = eA = 0.0
        for j in range(n):
            for L in range(n):
                D = np.zeros((n, n), dtype=LD)
                D[j, L] = h
                Pp, _, sp = law.host(Fm + D)
                Pm, _, sm = law.host(Fm - D)
                eP = max(eP, float(np.max(np.abs((sp - sm) / (2 * h) - P[:, j, L]))))
                eA = max(eA, float(np.max(np.abs((Pp - Pm) / (2 * h) - A[:, :, :, j, L]))))
        print("%-18s nsd %d: |dpsi/dF - P| %.2e, |dP/dF - A| %.2e, bound %.2e" % (type(law).__name__, n, eP, eA, bound))
        assert eP <= bP and eA <= bA
        # major symmetry (sums of products of the same factors in another order: a few longdouble roundings)
        assert float(np.max(np.abs(A - A.transpose(0, 3, 4, 1, 2)))) <= 16 * EPS_LD * float(np.max(np.abs(A)))


@pytest.mark.parametrize("n", [2, 3])
def test_objectivity(F, n):
    """P(R F) = R P(F) and psi(R F) = psi(F) for a rotation R: the two finite-strain laws (the linear one is not objective)"""
    Fm = H.random_F(n, 10, 5).astype(LD)
    Rm = H.random_F(n, 1, 9)[0]
    U, _, Vt = np.linalg.svd(Rm)
    Rm = (U @ Vt).astype(LD)                       # the rotation of its polar decomposition (to float64 rounding)
    Rm = Rm @ (LD(1.5) * np.eye(n, dtype=LD) - LD(0.5) * Rm.T @ Rm)       # one Newton step: orthogonal to longdouble rounding
    for law in _laws(F)[1:]:
        P, _, psi = law.host(Fm)
        Pr, _, psir = law.host(np.einsum("ia,qaK->qiK", Rm, Fm))
        scale = float(np.max(np.abs(P)))
        assert float(np.max(np.abs(Pr - np.einsum("ia,qaK->qiK", Rm, P)))) <= 1e-14 * scale
        assert float(np.max(np.abs(psir - psi))) <= 1e-14 * float(np.max(np.abs(psi)))
    lin = _laws(F)[0]
    assert float(np.max(np.abs(lin.host(np.einsum("ia,qaK->qiK", Rm, Fm))[2] - lin.host(Fm)[2]))) > 1e-3


def test_neo_hookean_refuses_a_negative_jacobian(F):
    Fm = np.tile(np.eye(2), (3, 1, 1))
    Fm[1, 0, 0] = -1.0
    with pytest.raises(ValueError, match="1 points with J <= 0"):
        F.NeoHookean(LAM, MU).host(Fm)


def _small_patches():
    uks2, cp2 = R.annulus_patch(2)
    uks3, cp3 = R.volume_patch(2, (2, 1, 2))
    return [("annulus", uks2, 2, cp2), ("volume", uks3, 2, cp3)]


@pytest.mark.parametrize("rational", [False, True])
def test_linear_law_is_the_oracles_mapped_elasticity(F, rational):
    """the tangent of ``LinearElastic`` through the reference, block by block, against the oracle's element loop (which forms
    the strains of the component functions): both in float64, entries to 1e-12 of the largest.  The oracle has no rational
    variant: with ``rational`` the control weights are set to 1 (then phi / W_h = phi)."""
    for name, uks, p, cp in _small_patches():
        cp = [np.asarray(c, dtype=np.float64) for c in cp]
        if rational:
            cp = [c / cp[-1] for c in cp]
        ref = H.HyperReference(uks, p, cp, rational=rational, dtype=np.float64)
        A = F.LinearElastic(LAM, MU).host(np.tile(np.eye(ref.nsd), (ref.npts, 1, 1)))[1]
        D = ref.dense(A)
        Ao = np.asarray(O.mapped_elasticity_fe_system(uks, p, cp, LAM, MU).todense())
        assert D.shape == Ao.shape
        assert np.max(np.abs(D - Ao)) <= 1e-12 * np.max(np.abs(Ao)), name


@pytest.mark.parametrize("rational", [False, True])
def test_assembled_residual_and_tangent_are_derivatives(F, rational):
    """R = dE/du and K = dR/du of the ASSEMBLED quantities in longdouble, by central differences along a random direction w
    with h = 1e-6.  Truncation: h^2 / 6 times the third derivative along w, |d^3 E| <= C3 G^3 vol and |d^3 R_a| <= C4 G^3 S with
    G = max |grad w| at the points, S = max_a int |grad psi_a| dx (both computed from the reference's own tables) and C3, C4
    of ``derivative_bounds`` at the extremes of F over the points; rounding: eps / h times |E| and max |R|, with a factor 4."""
    h = LD(1e-6)
    for name, uks, p, cp in _small_patches():
        ref = H.HyperReference(uks, p, cp, rational=rational)
        rng = np.random.default_rng(3)
        u = (0.02 * rng.standard_normal(ref.nF * ref.n)).astype(LD)
        w = rng.uniform(-0.2, 0.2, ref.nF * ref.n).astype(LD)
        Fm = (ref.grad_u(u) + np.eye(ref.nsd)).astype(np.float64)
        sv = np.linalg.svd(Fm, compute_uv=False)
        G = float(np.max(np.sqrt(np.sum(ref.grad_u(w).astype(np.float64) ** 2, axis=(1, 2)))))
        # a step h w changes F by h G <= 1e-6: the extremes hold for the differenced states as well, to that accuracy
        c3, c4 = H.derivative_bounds(LAM, MU, 1.001 * sv.max(), 1.001 / sv.min(), 1.001 * np.max(np.abs(np.log(np.prod(sv, axis=1)))))
        vol = float(np.sum(ref.ref.wdet()))
        S = np.zeros(ref.n)
        for g, PSI, Gr, wd in ref.ref.elements:
            np.add.at(S, g, (wd[:, None] * np.sqrt(np.sum(Gr.astype(np.float64) ** 2, axis=2))).sum(axis=0).astype(np.float64))
        S = float(S.max())
        for law in _laws(F):
            Rv, K = ref.residual(u, law), ref.tangent(u, law)
            bE = c3 * G ** 3 * vol * float(h) ** 2 / 6.0 + 4.0 * float(abs(ref.energy(u, law))) * EPS_LD / float(h)
            bR = c4 * G ** 3 * S * float(h) ** 2 / 6.0 + 4.0 * float(np.max(np.abs(Rv))) * EPS_LD / float(h)
            dE = (ref.energy(u + h * w, law) - ref.energy(u - h * w, law)) / (2 * h)
            dR = (ref.residual(u + h * w, law) - ref.residual(u - h * w, law)) / (2 * h)
            e1, e2 = float(abs(dE - Rv @ w)), float(np.max(np.abs(dR - K @ w)))
            print("%-8s %-18s %s: |dE - R.w| %.2e (bound %.2e), |dR - K w| %.2e (bound %.2e)"
                  % (name, type(law).__name__, "rational" if rational else "plain", e1, bE, e2, bR))
            assert e1 <= bE and e2 <= bR
            assert float(np.max(np.abs(K - K.T))) <= 64 * EPS_LD * float(np.max(np.abs(K)))


def test_float64_run_is_close_to_the_longdouble_run(F):
    name, uks, p, cp = _small_patches()[1]
    r, r64 = H.HyperReference(uks, p, cp, rational=True), H.HyperReference(uks, p, cp, rational=True, dtype=np.float64)
    u = 0.05 * np.random.default_rng(1).standard_normal(r.nF * r.n)
    law = F.NeoHookean(LAM, MU)
    a, b = r.residual(u, law), r64.residual(u, law)
    assert b.dtype == np.float64 and 0 < float(np.max(np.abs(a - b))) <= 1e-13 * float(np.max(np.abs(a)))


@pytest.mark.parametrize("name", ["annulus", "block"])
def test_host_newton_flows_converge_quadratically_without_line_search(F, name):
    """the loads of the GPU Newton tests: at most 8 Newton steps to 1e-9, the data on the moved face kept, and the last two
    steps of order >= 1.5 (r_k+1 = r_k^q; quadratic convergence with a constant C gives q = 2 + log C / log r_k, and the
    rounding floor of about 1e-13 relative caps the last step from r_k = 1e-8 at q = 1.6)"""
    pb, U, hist = H.host_flow(name, F.NeoHookean(H.LAM, H.MU))
    print(name, ["%.2e" % v for v in hist])
    assert len(hist) - 1 <= 8 and hist[-1] < H.NEWTON_TOL
    fixed = np.setdiff1d(np.arange(U.size), pb["free"])
    assert np.array_equal(U[fixed], pb["U0"][fixed]) and np.max(np.abs(U[pb["free"]])) > 1e-2
    q = [np.log(hist[k + 1]) / np.log(hist[k]) for k in (-3, -2)]
    assert min(q) >= 1.5, q
