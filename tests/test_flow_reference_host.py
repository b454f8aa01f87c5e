"""CPU: the host reference of the system forms and of the stabilised flow (tests/flow_reference.py) and the numpy law
``forms.IncompressibleFlow.host`` against facts that do not depend on them -- the matrices of the references that came
before, the divergence theorem on a box, the metric of an affine box, central differences of the law's own source and flux
and of the assembled residual, and the steady Taylor-Green vortex: Newton counts, quadratic convergence, error rates.
"""
import numpy as np
import pytest

import postproc_reference as R
import coef_reference as CR
import hyper_reference as H
import flow_reference as FR

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
TOL = 1e-12


@pytest.fixture(scope="module")
def F():
    from tigar_amd import forms
    return forms


def _patches():
    uks2, cp2 = R.annulus_patch(2)
    uks3, cp3 = R.volume_patch(2, (2, 1, 2))
    return [("annulus", uks2, 2, [np.asarray(c, dtype=np.float64) for c in cp2]),
            ("volume", uks3, 2, [np.asarray(c, dtype=np.float64) for c in cp3])]


@pytest.mark.parametrize("rational", [False, True])
def test_one_field_is_the_scalar_reference(rational):
    """nF = 1: matrix and load of ``coef_reference`` (the same sums in another order), in both precisions"""
    for name, uks, p, cp in _patches():
        for dt, tol in ((LD, 64 * EPS_LD), (np.float64, 64 * CR.EPS)):
            sys_, one = FR.SystemReference(uks, p, cp, 1, rational=rational, dtype=dt), CR.CoefReference(uks, p, cp, rational=rational, dtype=dt)
            rng = np.random.default_rng(1)
            npts, nsd = one.npts, one.nsd
            A, b, c, m = rng.standard_normal((npts, nsd, nsd)), rng.standard_normal((npts, nsd)), rng.standard_normal((npts, nsd)), rng.standard_normal(npts)
            k1, v1 = sys_.coo(A[:, None, :, None, :], b[:, None, :, None], c[:, None, None, :], m[:, None, None])
            k0, v0 = one.matrix(A, b, c, m)
            assert np.array_equal(k0, k1) and float(np.max(np.abs(v1 - v0))) <= tol * float(np.max(np.abs(v0))), name
            s, Fx = rng.standard_normal(npts), rng.standard_normal((npts, nsd))
            l1, l0 = sys_.load(s[:, None], Fx[:, None, :]), one.load(s, Fx)
            assert float(np.max(np.abs(l1 - l0))) <= tol * float(np.max(np.abs(l0)))
            u = rng.standard_normal(one.nnodes)
            (U1, G1), (U0, G0) = sys_.eval(u), one.eval(u)
            assert float(np.max(np.abs(U1[:, 0] - U0))) <= tol * 10 and float(np.max(np.abs(G1[:, 0] - G0))) <= tol * 100


@pytest.mark.parametrize("rational", [False, True])
def test_without_b_and_c_it_is_the_vector_reference(rational):
    """nF = nsd, b = c = 0: the blocks of ``hyper_reference``"""
    for name, uks, p, cp in _patches():
        hy = H.HyperReference(uks, p, cp, rational=rational)
        sys_ = FR.SystemReference(uks, p, cp, hy.nF, rational=rational)
        rng = np.random.default_rng(2)
        A, M = rng.standard_normal((hy.npts, hy.nF, hy.nsd, hy.nF, hy.nsd)), rng.standard_normal((hy.npts, hy.nF, hy.nF))
        D0, D1 = hy.dense(A, M), sys_.dense(A, None, None, M)
        assert float(np.max(np.abs(D1 - D0))) <= 64 * EPS_LD * float(np.max(np.abs(D0))), name


@pytest.mark.parametrize("d", [1, 2, 3])
def test_advection_blocks_cancel_inside_a_box(d):
    """one constant b_iKj and c_ijL = b_iLj on an affine box: (B + C)_(i a)(j b) = b_iKj int d_K (phi_a phi_b), a boundary integral,
    which vanishes when a or b is an interior node -- in every block"""
    p, nels, nF = 2, (3, 2, 2)[:d], 2
    uks = [np.linspace(0.0, 1.0 + 0.5 * k, nels[k] + 1) ** 1.3 for k in range(d)]
    X = R.lagrange_nodes(uks, p)
    lin = np.array([[2.0, 0.3, -0.1], [0.2, 1.5, 0.4], [-0.3, 0.1, 0.8]])[:d, :d]
    cp = [sum(lin[i, k] * X[k] for k in range(d)) + 0.1 * i for i in range(d)] + [np.ones_like(X[0])]
    ref = FR.SystemReference(uks, p, cp, nF, dtype=np.float64)
    b = np.random.default_rng(3).standard_normal((nF, d, nF))
    S = ref.dense(None, b, b.transpose(0, 2, 1), None)
    n = [e * p + 1 for e in nels]
    idx = np.array(np.unravel_index(np.arange(ref.n), n, order="F")).T
    interior = np.tile(np.all((idx > 0) & (idx < np.array(n) - 1), axis=1), nF)
    scale = np.max(np.abs(ref.dense(None, b, None, None)))
    assert interior.any() and not interior.all()
    assert np.max(np.abs(S[interior, :])) <= TOL * scale and np.max(np.abs(S[:, interior])) <= TOL * scale
    assert np.max(np.abs(S)) > 1e-3 * scale


def test_metric_of_affine_maps_and_of_the_annulus():
    """an affine map x = L xi + c on non-uniform elements: G = (2 D^-1 L^-1)^T (2 D^-1 L^-1) with D = diag(h) at every point of
    the element; the quarter annulus: the radial direction is an eigenvector with the
    eigenvalue 4 / (dr/dxi h_0)^2 = 4 / h_0^2 (r = 1 + xi_0)"""
    p = 2
    uks = [np.array([0.0, 0.3, 1.0]), np.array([0.0, 0.5, 0.75, 1.0])]
    X = R.lagrange_nodes(uks, p)
    L = np.array([[2.0, 0.3], [0.2, 1.5]])
    cp = [L[i, 0] * X[0] + L[i, 1] * X[1] + 0.1 * i for i in range(2)] + [np.ones_like(X[0])]
    Li = np.linalg.inv(L)
    G = FR.metric(uks, p, cp).astype(np.float64).reshape(3, 2, 9, 2, 2)          # elements lexicographic, direction 0 fastest
    for e1 in range(3):
        for e0 in range(2):
            B = 2.0 * np.diag([1.0 / (uks[0][e0 + 1] - uks[0][e0]), 1.0 / (uks[1][e1 + 1] - uks[1][e1])]) @ Li
            assert np.max(np.abs(G[e1, e0] - B.T @ B)) <= 1e-13 * np.max(B.T @ B)
    uks, cp = R.annulus_patch(2)
    ref = CR.CoefReference(uks, 2, cp, dtype=np.float64)
    G = FR.metric(uks, 2, cp, dtype=np.float64)
    er = ref.x / np.linalg.norm(ref.x, axis=1)[:, None]
    Ger = np.einsum("qKL,qL->qK", G, er)
    assert np.max(np.abs(Ger - 4.0 / 0.5 ** 2 * er)) <= 1e-11 * 16.0


def _random_state(nsd, npts, seed):
    rng = np.random.default_rng(seed)
    U, gU = rng.standard_normal((npts, nsd + 1)), rng.standard_normal((npts, nsd + 1, nsd))
    B = rng.standard_normal((npts, nsd, nsd))
    return U, gU, 4.0 * (np.einsum("qab,qcb->qac", B, B) + np.eye(nsd)), rng.standard_normal((npts, nsd)), rng.standard_normal((npts, nsd))


@pytest.mark.parametrize("variant", ["steady", "transient"])
@pytest.mark.parametrize("nsd", [2, 3])
def test_law_tangent_is_the_derivative_of_source_and_flux(F, nsd, variant):
    """A, b, c, m of ``IncompressibleFlow.host`` against central differences of its own (s, F) in longdouble, h = 1e-6, at random
    states; bound: h^2 / 6 times C3 of ``flow_reference.derivative_bound`` (worked out there from the product rule) plus the
    rounding 4 eps max(|s|, |F|) / h"""
    law = F.IncompressibleFlow(1.3, 0.2)
    U, gU, G, a0, f = _random_state(nsd, 40, 7 + nsd)
    kw = dict(c_a=0.0, a0=None, f=None, dt4=0.0) if variant == "steady" else dict(c_a=1.7, a0=a0.astype(LD), f=f.astype(LD), dt4=256.0)
    h = LD(1e-6)
    U, gU, G = U.astype(LD), gU.astype(LD), G.astype(LD)
    s, Fx, A, b, c, m, tau = law.host(U, gU, G, **kw)
    assert all(v.dtype == LD for v in (s, Fx, A, b, c, m, tau))
    c3 = 1.001 * FR.derivative_bound(law, U, gU, G, **kw)
    bound = c3 * float(h) ** 2 / 6.0 + 4.0 * EPS_LD * max(float(np.max(np.abs(s))), float(np.max(np.abs(Fx)))) / float(h)
    nF, err = nsd + 1, 0.0
    for j in range(nF):
        D = np.zeros_like(U)
        D[:, j] = h
        (sp, Fp), (sm, Fm) = law.host(U + D, gU, G, **kw)[:2], law.host(U - D, gU, G, **kw)[:2]
        err = max(err, float(np.max(np.abs((sp - sm) / (2 * h) - m[:, :, j]))), float(np.max(np.abs((Fp - Fm) / (2 * h) - b[:, :, :, j]))))
        for L in range(nsd):
            D = np.zeros_like(gU)
            D[:, j, L] = h
            (sp, Fp), (sm, Fm) = law.host(U, gU + D, G, **kw)[:2], law.host(U, gU - D, G, **kw)[:2]
            err = max(err, float(np.max(np.abs((sp - sm) / (2 * h) - c[:, :, j, L]))), float(np.max(np.abs((Fp - Fm) / (2 * h) - A[:, :, :, j, L]))))
    print("flow law nsd %d %s: |difference - tangent| %.2e, bound %.2e (C3 = %.2e)" % (nsd, variant, err, bound, c3))
    assert err <= bound
    # tau as it is defined, and the float64 law next to the longdouble one
    tM = (LD(kw["dt4"]) + np.einsum("qK,qKL,qL->q", U[:, :nsd], G, U[:, :nsd]) + LD(36) * (LD(0.2) / LD(1.3)) ** 2 * np.einsum("qKL,qKL->q", G, G)) ** LD(-0.5)
    assert float(np.max(np.abs(tau[:, 0] - tM))) <= 8 * EPS_LD * float(np.max(tM))
    lo = law.host(U.astype(np.float64), gU.astype(np.float64), G.astype(np.float64),
                  **{k: (v.astype(np.float64) if hasattr(v, "astype") else v) for k, v in kw.items()})
    assert all(v.dtype == np.float64 for v in lo)
    assert float(np.max(np.abs(lo[2] - A))) <= 1e-13 * float(np.max(np.abs(A)))


@pytest.mark.parametrize("rational", [False, True])
def test_assembled_tangent_is_the_derivative_of_the_assembled_residual(F, rational):
    """K w against central differences of the ASSEMBLED residual along a random direction w in longdouble, h = 1e-6.
    Truncation: h^2 / 6 |d^3 R_a| <= h^2 / 6 sqrt(nsd) C3 W^3 S with W = max over the points of |(w, grad w)|, S = max_a int |psi_a| +
    |grad psi_a| dx (from the reference's own tables) and C3 of ``derivative_bound`` at the state; rounding: 4 eps max |R| / h"""
    h = LD(1e-6)
    law = F.IncompressibleFlow(1.3, 0.2)
    for name, uks, p, cp in _patches():
        ref = FR.FlowReference(uks, p, cp, rational=rational)
        rng = np.random.default_rng(3)
        u = (0.3 * rng.standard_normal(ref.nF * ref.n)).astype(LD)
        w = rng.uniform(-0.2, 0.2, ref.nF * ref.n).astype(LD)
        a0 = rng.standard_normal((ref.npts, ref.nsd))
        kw = dict(c_a=1.7, a0=a0, f=None, dt4=64.0)
        Wq, gWq = ref.eval(w)
        Wn = float(np.max(np.sqrt(np.sum(Wq.astype(np.float64) ** 2, axis=1) + np.sum(gWq.astype(np.float64) ** 2, axis=(1, 2)))))
        S = np.zeros(ref.n)
        np.add.at(S, ref.g.ravel(), (ref.wd[:, :, None] * (np.abs(ref.PSI) + np.sqrt(np.sum(ref.GR ** 2, axis=3)))).sum(axis=1).astype(np.float64).ravel())
        Uq, gUq = ref.eval(u)
        c3 = 1.001 * FR.derivative_bound(law, Uq, gUq, ref.G, **kw)
        Rv, K = ref.residual(u, law, **kw), ref.tangent(u, law, **kw)
        bound = np.sqrt(ref.nsd) * c3 * Wn ** 3 * float(S.max()) * float(h) ** 2 / 6.0 + 4.0 * float(np.max(np.abs(Rv))) * EPS_LD / float(h)
        dR = (ref.residual(u + h * w, law, **kw) - ref.residual(u - h * w, law, **kw)) / (2 * h)
        err = float(np.max(np.abs(dR - K @ w)))
        print("%-8s %s: |dR - K w| %.2e (bound %.2e)" % (name, "rational" if rational else "plain", err, bound))
        assert err <= bound
        assert float(np.max(np.abs(K - K.T))) > 1e-3 * float(np.max(np.abs(K)))          # (the flow tangent is not symmetric)


def test_float64_run_is_close_to_the_longdouble_run(F):
    name, uks, p, cp = _patches()[1]
    r, r64 = FR.FlowReference(uks, p, cp, rational=True), FR.FlowReference(uks, p, cp, rational=True, dtype=np.float64)
    u = 0.3 * np.random.default_rng(1).standard_normal(r.nF * r.n)
    law = F.IncompressibleFlow(1.0, 0.1)
    a, b = r.residual(u, law), r64.residual(u, law)
    assert b.dtype == np.float64 and 0 < float(np.max(np.abs(a - b))) <= 1e-13 * float(np.max(np.abs(a)))


def test_steady_taylor_green_host_flow():
    """p = 2 on 4^2, 8^2, 16^2 elements of the distorted square: Newton from zero reaches 1e-9 in at most 8 steps, the last two of
    order >= 1.5, the fixed dofs stay zero, and the velocity L2 errors fall by >= 3 from 8^2 to 16^2 (order >= 1.5 where 2 is
    expected).  Figures (this machine's numpy): the README section "Incompressible flow" records them."""
    errs = {}
    for nel in (4, 8, 16):
        pb, law, U, hist, e = FR.host_taylor_green(nel)
        errs[nel] = e
        print("taylor-green %2d^2: %d steps, history %s, L2 errors %.4e %.4e" % (nel, len(hist) - 1, " ".join("%.1e" % v for v in hist), e[0], e[1]))
        assert len(hist) - 1 <= 8 and hist[-1] < FR.NEWTON_TOL
        fixed = np.setdiff1d(np.arange(U.size), pb["free"])
        assert np.all(U[fixed] == 0.0) and np.max(np.abs(U[pb["free"]])) > 0.1
        q = [np.log(hist[k + 1]) / np.log(hist[k]) for k in (-3, -2)]
        assert min(q) >= 1.5, q
    ratios = [errs[8][i] / errs[16][i] for i in range(2)]
    print("error ratios 8^2 -> 16^2: %.2f %.2f" % tuple(ratios))
    assert min(ratios) >= 3.0


@pytest.mark.parametrize("scheme", ["generalized_alpha", "backward_euler"])
def test_transient_taylor_green_host_flow(F, scheme):
    """the vortex without a body force on 8^2 elements, dt = 1/8, four steps from the L2 projection of the exact fields: every step
    takes at most 4 Newton steps to 1e-9, and the amplitude int u_h . u_0 / int u_0 . u_0 follows exp(-2 nu t) to 1e-3 (measured:
    7e-4 generalized-alpha, 4e-4 backward Euler after four steps -- the error of this mesh and step, which the GPU test takes
    as its yardstick)"""
    pb, law, U0, V0, ref = FR.transient_taylor_green_data()
    S, V, hist = FR.time_stepping(ref, pb["Mc"], pb["free"], law, U0, V0, FR.TG_DT, 4, scheme=scheme)
    Mc = np.asarray(pb["Mc"].todense() if hasattr(pb["Mc"], "todense") else pb["Mc"])
    for k, s in enumerate(S):
        t = FR.TG_DT * (k + 1)
        amp = FR.amplitude(ref, Mc @ s)
        print("%s step %d: %d Newton steps, amplitude %.6f, exp(-2 nu t) %.6f" % (scheme, k + 1, len(hist[k]) - 1, amp, np.exp(-2 * FR.TG_MU / FR.TG_RHO * t)))
        assert len(hist[k]) - 1 <= 4 and abs(amp - np.exp(-2 * FR.TG_MU / FR.TG_RHO * t)) <= 1e-3


@pytest.mark.parametrize("nsd", [2, 3])
def test_source_and_flux_are_the_formulas_written_out(F, nsd):
    """(s, F, tau) of ``IncompressibleFlow.host`` against the formulas of the README evaluated here with plain loops over the points
    and the indices, term by term (Galerkin, SUPG, PSPG, LSIC each by itself), in longdouble: a few roundings apart"""
    rho, mu, CI, c_a, dt4 = LD(1.3), LD(0.2), LD(36), LD(1.7), LD(64)
    law = F.IncompressibleFlow(float(rho), float(mu), C_I=float(CI))
    U, gU, G, a0, f = [v.astype(LD) for v in _random_state(nsd, 12, 40 + nsd)]
    s, Fx, _, _, _, _, tau = law.host(U, gU, G, c_a=float(c_a), a0=a0, f=f, dt4=float(dt4))
    nu = mu / rho
    for q in range(U.shape[0]):
        u, p, du, dp = U[q, :nsd], U[q, nsd], gU[q, :nsd, :], gU[q, nsd, :]
        uGu = sum(u[K] * G[q, K, L] * u[L] for K in range(nsd) for L in range(nsd))
        GG = sum(G[q, K, L] * G[q, K, L] for K in range(nsd) for L in range(nsd))
        tM = 1 / np.sqrt(dt4 + uGu + CI * nu * nu * GG)
        tC = 1 / (tM * sum(G[q, K, K] for K in range(nsd)))
        div = sum(du[L, L] for L in range(nsd))
        want_s = np.zeros(nsd + 1, dtype=LD)
        want_F = np.zeros((nsd + 1, nsd), dtype=LD)
        r = np.zeros(nsd, dtype=LD)
        for i in range(nsd):
            acc = c_a * u[i] + a0[q, i] + sum(u[L] * du[i, L] for L in range(nsd)) - f[q, i]
            want_s[i] = rho * acc
            r[i] = rho * acc + dp[i]
        want_s[nsd] = div
        for i in range(nsd):
            for K in range(nsd):
                galerkin = mu * (du[i, K] + du[K, i]) - (p if i == K else 0)
                supg = tM * u[K] * r[i]
                lsic = rho * tC * div if i == K else 0
                want_F[i, K] = galerkin + supg + lsic
        for K in range(nsd):
            want_F[nsd, K] = tM / rho * r[K]                             # PSPG
        scale = max(float(np.max(np.abs(want_F))), float(np.max(np.abs(want_s))))
        assert float(np.max(np.abs(s[q] - want_s))) <= 32 * EPS_LD * scale and float(np.max(np.abs(Fx[q] - want_F))) <= 32 * EPS_LD * scale
        assert abs(float(tau[q, 0] - tM)) <= 8 * EPS_LD * float(tM) and abs(float(tau[q, 1] - tC)) <= 8 * EPS_LD * float(tC)
