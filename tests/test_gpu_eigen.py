"""GPU: the block kernels of csrc/tg_eig.hip against single-vector products and numpy, and SLEPcEigenSolver (block LOBPCG,
tigar_amd/eigen.py) against analytic cantilever frequencies, dense / sparse scipy eigensolvers on the downloaded pencils, on
Laplace, elasticity and a mapped NURBS patch, with every preconditioner and every refusal."""
import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

CANTILEVER = np.array([3.5160153, 22.034492, 61.697214, 120.90192, 199.85953])     # (beta_n L)^2


def _rand_csr(n, seed, long_rows=True, empty_frac=0.2):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=min(1.0, 12.0 / max(n, 1)), random_state=rng, format="lil")
    if long_rows and n > 300:
        for r in (0, n // 2):                  # rows longer than one 64-entry chunk
            cols = rng.choice(n, 200, replace=False)
            A[r, cols] = rng.standard_normal(200)
    A = A.tocsr()
    if n > 1:
        keep = rng.random(n) >= empty_frac     # empty rows
        A = sp.diags(keep.astype(float)) @ A
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


# ------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", [1, 1007])
@pytest.mark.parametrize("k", [1, 3, 8, 16, 33, 64])
def test_spmm_matches_spmv(n, k):
    from tigar_amd.device import DeviceCSR, DeviceBlock, DeviceVector
    A = _rand_csr(n, 10 * n + k)
    if n == 1:
        A = sp.csr_matrix(np.array([[2.5]]))
    rng = np.random.default_rng(k)
    X = rng.standard_normal((n, k))
    dA = DeviceCSR.from_scipy(A)
    Xb = DeviceBlock(n, k, data=X)
    Y = dA.mult_block(Xb).to_numpy()
    scale = abs(A) @ abs(X)
    for j in range(k):
        y = dA.mult(DeviceVector(data=X[:, j])).get_local()
        assert np.all(np.abs(Y[:, j] - y) <= 1e-14 * scale[:, j] + 1e-300), j
    assert np.all(np.abs(Y - A @ X) <= 1e-14 * scale + 1e-300)
    Y2 = dA.mult_block(Xb).to_numpy()
    assert np.array_equal(Y.view(np.int64), Y2.view(np.int64))


def test_spmm_empty_matrix_and_rectangular():
    from tigar_amd.device import DeviceCSR, DeviceBlock
    A = sp.csr_matrix((50, 50))
    Y = DeviceCSR.from_scipy(A).mult_block(DeviceBlock(50, 5, data=np.ones((50, 5)))).to_numpy()
    assert np.array_equal(Y, np.zeros((50, 5)))
    R = _rand_csr(1007, 3)[:300, :]
    X = np.random.default_rng(1).standard_normal((1007, 7))
    Y = DeviceCSR.from_scipy(R).mult_block(DeviceBlock(1007, 7, data=X)).to_numpy()
    assert np.allclose(Y, R @ X, rtol=0, atol=1e-13 * np.abs(R).max() * np.abs(X).max() * 300)


@pytest.mark.parametrize("n,kx,ky", [(1, 1, 1), (1007, 3, 8), (5000, 16, 16), (777, 64, 33), (4099, 64, 64)])
def test_gram_and_combine_match_numpy(n, kx, ky):
    from tigar_amd import device as dev
    rng = np.random.default_rng(n + kx + ky)
    X, Y = rng.standard_normal((n, kx)), rng.standard_normal((n, ky))
    Xb, Yb = dev.DeviceBlock(n, kx, data=X), dev.DeviceBlock(n, ky, data=Y)
    G = dev.block_gram(Xb, Yb)
    assert np.all(np.abs(G - X.T @ Y) <= 1e-13 * (np.abs(X).T @ np.abs(Y)))
    assert np.array_equal(G, dev.block_gram(Xb, Yb))
    Z = rng.standard_normal((n, 5))
    Zb = dev.DeviceBlock(n, 5, data=Z)
    C1, C2, C3 = rng.standard_normal((kx, ky)), rng.standard_normal((ky, ky)), rng.standard_normal((5, ky))
    out = dev.DeviceBlock(n, ky)
    dev.block_combine([(Xb, C1), (Yb, C2), (Zb, C3)], out)
    ref = X @ C1 + Y @ C2 + Z @ C3
    scale = np.abs(X) @ np.abs(C1) + np.abs(Y) @ np.abs(C2) + np.abs(Z) @ np.abs(C3)
    got = out.to_numpy()
    assert np.all(np.abs(got - ref) <= 1e-13 * scale)
    out2 = dev.DeviceBlock(n, ky)
    dev.block_combine([(Xb, C1), (Yb, C2), (Zb, C3)], out2)
    assert np.array_equal(got.view(np.int64), out2.to_numpy().view(np.int64))


def test_residual_columns_and_decoupled_rows():
    from tigar_amd import device as dev
    rng = np.random.default_rng(5)
    n, k = 1003, 6
    AX, BX = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    lam = rng.random(k) + 1.0
    mask = (rng.random(n) < 0.1).astype(float)
    d = rng.random(n) + 0.5
    R, W = dev.DeviceBlock(n, k), dev.DeviceBlock(n, k)
    rn, bn = dev.block_residual(dev.DeviceBlock(n, k, data=AX), dev.DeviceBlock(n, k, data=BX), lam, R, W,
                                dev.DeviceVector(data=mask), dev.DeviceVector(data=d))
    Rr = (AX - BX * lam) * (1.0 - mask)[:, None]
    assert np.allclose(R.to_numpy(), Rr, rtol=1e-15, atol=1e-15)
    assert np.allclose(W.to_numpy(), Rr * d[:, None], rtol=1e-15, atol=1e-15)
    assert np.allclose(rn, (Rr ** 2).sum(0), rtol=1e-13) and np.allclose(bn, (BX ** 2).sum(0), rtol=1e-13)
    v = R.get_column(2)
    assert np.array_equal(v.get_local(), R.to_numpy()[:, 2])
    R.set_column(4, v)
    assert np.array_equal(R.to_numpy()[:, 4], R.to_numpy()[:, 2])
    # decoupled rows: zeroed row / column with the diagonal kept, in both matrices
    A = (sp.random(n, n, density=0.01, random_state=1) + sp.identity(n)).tolil()
    A = (A + A.T).tolil()
    B = sp.identity(n, format="lil") * 2.0 + sp.diags(np.full(n - 1, 0.1), 1).tolil()
    B = (B + B.T).tolil()
    zd = [0, 7, 500, n - 1]
    for M, dg in ((A, 3.0), (B, 0.5)):
        for z in zd:
            M[z, :] = 0.0
            M[:, z] = 0.0
            M[z, z] = dg
    dA, dB = dev.DeviceCSR.from_scipy(A.tocsr()), dev.DeviceCSR.from_scipy(B.tocsr())
    mark, da, db, cnt, arow = dev.csr_decoupled_rows(dA, dB)
    assert cnt == len(zd) and np.array_equal(np.nonzero(mark.get_local())[0], zd)
    keep = np.setdiff1d(np.arange(n), zd)
    assert arow == np.abs(A.tocsr()[keep]).sum(1).max() or abs(arow / np.abs(A.tocsr()[keep]).sum(1).max() - 1) < 1e-14
    assert np.array_equal(da.get_local(), A.tocsr().diagonal()) and np.array_equal(db.get_local(), B.tocsr().diagonal())


def test_kernels_refuse_bad_widths_and_loose_csr():
    from tigar_amd import _lib, device as dev
    L = _lib.lib()
    A = dev.DeviceCSR.from_scipy(_rand_csr(100, 1))
    for k in (0, 65):
        X, Y = dev.DeviceVector(max(k, 1) * 100), dev.DeviceVector(max(k, 1) * 100)
        assert L.tg_spmm(A._h, X._h, k, Y._h) != 0
        assert L.tg_block_gram(X._h, k, Y._h, 1, 100, np.zeros(65 * 65).ctypes.data_as(_lib.c_f64p)) != 0
        assert L.tg_block_gram(X._h, 1, Y._h, k, 100, np.zeros(65 * 65).ctypes.data_as(_lib.c_f64p)) != 0
    with pytest.raises(ValueError):
        dev.DeviceBlock(10, 65)
    view = dev.csr_vstack_view([A, A])
    assert view.is_loose()
    with pytest.raises(_lib.TigarHipError, match="loose-row or view"):
        view.mult_block(dev.DeviceBlock(100, 4))


# ------------------------------------------------------------------------------------------------- the demo
def _cantilever(diag_a, diag_b=1.0, p=3, nel=100):
    import tigar_amd as t
    from tigar_amd import BSplines as Bs, forms as F
    mesh = Bs.ExplicitBSplineControlMesh([p], [Bs.uniformKnots(p, 0.0, 1.0, nel)])
    gen = t.EqualOrderSpline(1, mesh)
    gen.addZeroDofs(0, gen.getScalarSpline(0).getSideDofs(0, 0, nLayers=2))
    spline = t.ExtractedSpline(gen, 2 * p)
    g = spline.V.grids[0]
    Mfe, _, S2, _ = F.fe_matrices_1d_ext(g.vertices[0], g.degree)
    A = spline.extractMatrix(S2, diag=diag_a)
    B = spline.extractMatrix(Mfe, diag=diag_b)
    return spline, A, B


def test_modal_analysis_demo_as_written():
    import math
    import tigar_amd as t
    spline, A, B = _cantilever(1.0 / t.DOLFIN_EPS)
    solver = t.SLEPcEigenSolver(A, B)
    solver.parameters["spectrum"] = "smallest magnitude"
    solver.solve()
    assert solver.get_number_converged() >= 5
    om = []
    for n in range(5):
        omega2, _, uVectorIGA, _ = solver.get_eigenpair(n)
        om.append(math.sqrt(omega2))
        u = t.Function(spline.V)
        u.vector()[:] = spline.M * uVectorIGA                      # the demo's prolongation
        assert np.linalg.norm(u.vector().get_local()) > 0
    om = np.array(om)
    assert np.all(np.abs(om - CANTILEVER) <= 2e-6 * CANTILEVER), om
    # against the dense pencil on the host: to 1e-9, or to what the pencil determines in double precision where that is
    # less -- lambda_max / lambda_1 ~ 6e9 here, so a rounding of A of eps |A| moves lambda_1 by up to eps |A| |x|^2 (the
    # dense and the shift-invert solvers on the host differ by 5e-8 in lambda_1 themselves)
    Ah, Bh = A.to_scipy().toarray(), B.to_scipy().toarray()
    ref = sl.eigh(Ah, Bh, eigvals_only=True)[:5]
    lam = np.array([solver.get_eigenvalue(i)[0] for i in range(5)])
    X = np.array([solver.get_eigenpair(i)[2].get_local() for i in range(5)]).T
    keep = np.setdiff1d(np.arange(Ah.shape[0]), np.asarray(spline.zeroDofs))
    anorm = np.abs(Ah[keep]).sum(1).max()
    cond = 8 * np.finfo(np.float64).eps * anorm * (X ** 2).sum(0) / lam
    assert np.all(np.abs(lam - ref) <= np.maximum(1e-9, cond) * ref), (lam, ref, cond)
    assert np.all(np.abs(lam[1:] - ref[1:]) <= 1e-9 * ref[1:] + cond[1:] * ref[1:])
    print("cantilever omega rel. errors", om / CANTILEVER - 1, "vs dense", lam / ref - 1, "iterations",
          solver.last["iterations"])
    x = solver.get_eigenpair(0)[2].get_local()
    assert abs(x @ Bh @ x - 1.0) < 1e-10 and x[np.argmax(np.abs(x))] > 0


def test_diag_one_reports_unit_pairs_on_clamped_dofs():
    import tigar_amd as t
    spline, A, B = _cantilever(1.0, 1.0)
    solver = t.SLEPcEigenSolver(A, B)
    solver.solve(4)
    zd = sorted(np.asarray(spline.zeroDofs).tolist())
    ref = sl.eigh(A.to_scipy().toarray(), B.to_scipy().toarray(), eigvals_only=True)[:4]
    got = []
    for i in range(4):
        lam, _, x, cx = solver.get_eigenpair(i)
        got.append(lam)
        if i < 2:
            assert lam == 1.0
            xh = x.get_local()
            assert np.count_nonzero(xh) == 1 and int(np.nonzero(xh)[0][0]) in zd and xh.max() == 1.0
        assert np.all(cx.get_local() == 0.0)
    # (the free pairs to what the pencil determines in double precision, see the demo test)
    assert got[:2] == [1.0, 1.0] and np.allclose(got[2:], ref[2:], rtol=1e-6, atol=0)
    assert abs(got[3] - ref[3]) <= 1e-9 * ref[3]


# ------------------------------------------------------------------------------------------------- 2-D / 3-D / mapped
def _box(d, p, nel, nf=1, faces="all"):
    import tigar_amd as t
    from tigar_amd import BSplines as Bs
    gen = t.EqualOrderSpline(nf, Bs.ExplicitBSplineControlMesh([p] * d, [Bs.uniformKnots(p, 0.0, 1.0, nel)] * d))
    sc = gen.getScalarSpline(0)
    for f in range(nf):
        for direction in range(d):
            for side in (0, 1):
                if faces == "all" or (direction, side) in faces:
                    gen.addZeroDofs(f, sc.getSideDofs(direction, side))
    return gen, t.ExtractedSpline(gen, 2 * p)


def _eigsh_ref(A, B, nev):
    """shift-invert Lanczos on the host copies (a dense solve of the pencil loses the small eigenpairs next to the
    1 / DOLFIN_EPS rows)"""
    Ah, Bh = A.to_scipy(), B.to_scipy()
    lam, V = spla.eigsh(Ah, k=nev, M=Bh, sigma=0, which="LM", tol=1e-14)
    o = np.argsort(lam)
    return lam[o], V[:, o], Ah, Bh


def _check(solver, A, B, nev, tol=1e-8):
    ref, V, Ah, Bh = _eigsh_ref(A, B, nev)
    lam = np.array([solver.get_eigenvalue(i)[0] for i in range(nev)])
    assert np.all(np.abs(lam - ref) <= tol * np.abs(ref)), (lam, ref)
    X = np.array([solver.get_eigenpair(i)[2].get_local() for i in range(nev)]).T
    assert np.abs(X.T @ (Bh @ X) - np.eye(nev)).max() < 1e-10
    for i in range(nev):
        r = Ah @ X[:, i] - lam[i] * (Bh @ X[:, i])
        assert np.linalg.norm(r) <= 1.01 * solver.parameters["tolerance"] * abs(lam[i]) * np.linalg.norm(Bh @ X[:, i])
    return lam, X, V, Ah, Bh


@pytest.mark.parametrize("p", [2, 3])
def test_laplace_2d_square(p):
    import tigar_amd as t
    from tigar_amd import forms as F
    gen, spline = _box(2, p, 16)
    A, B = spline.assembleMatrix(F.LaplaceForm(), diag=1.0 / t.DOLFIN_EPS), spline.assembleMatrix(F.MassForm())
    solver = t.SLEPcEigenSolver(A, B)
    solver.solve(11)
    lam, X, V, Ah, Bh = _check(solver, A, B, 11)
    limit = np.array([2, 5, 5, 8, 10, 10, 13, 13, 17, 17, 18]) * np.pi ** 2
    assert np.all(np.abs(lam - limit) <= 3e-2 * limit)
    # the double eigenvalues: the cluster spans the space scipy finds
    for a, b in ((1, 3), (4, 6), (6, 8), (8, 10)):
        ang = sl.subspace_angles(X[:, a:b], V[:, a:b])
        assert ang.max() < 1e-6, (a, b, ang)


def test_elasticity_3d_one_face_clamped():
    import tigar_amd as t
    from tigar_amd import forms as F
    from tigar_amd.device import DeviceCSR
    gen, spline = _box(3, 2, 5, nf=3, faces=[(0, 0)])
    A = spline.assembleMatrix(F.ElasticityForm(lmbda=2.0, mu=1.0), diag=1.0 / t.DOLFIN_EPS)
    # mass of the vector space: one copy of the scalar mass (same clamped face) per field
    _, scalar = _box(3, 2, 5, nf=1, faces=[(0, 0)])
    Ms = scalar.assembleMatrix(F.MassForm()).to_scipy()
    assert A.shape[0] == 3 * Ms.shape[0]
    B = DeviceCSR.from_scipy(sp.block_diag([Ms] * 3, format="csr"))
    solver = t.SLEPcEigenSolver(A, B)
    solver.solve(6)
    _check(solver, A, B, 6)


def test_mapped_quarter_annulus():
    import tigar_amd as t
    from tigar_amd import forms as F
    from geom_util import quarter_annulus
    kv, Pf = quarter_annulus(8)
    gen = t.EqualOrderSpline(1, t.NURBSControlMesh([2, 2], [kv, kv], Pf))
    sc = gen.getScalarSpline(0)
    for direction in range(2):
        for side in (0, 1):
            gen.addZeroDofs(0, sc.getSideDofs(direction, side))
    spline = t.ExtractedSpline(gen, 4)
    A = spline.assembleMatrix(F.LaplaceForm(geometry=gen), diag=1.0 / t.DOLFIN_EPS)
    B = spline.assembleMatrix(F.MassForm(geometry=gen))
    solver = t.SLEPcEigenSolver(A, B)
    solver.solve(8)
    _check(solver, A, B, 8)


# ------------------------------------------------------------------------------------------------- preconditioners
def _laplace3d(nel, p=2):
    """the demo's pencil on a cube: zero dofs with 1 / DOLFIN_EPS in K (their pairs lie far above the requested ones)"""
    import tigar_amd as t
    from tigar_amd import forms as F
    gen, spline = _box(3, p, nel)
    return spline.assembleMatrix(F.LaplaceForm(), diag=1.0 / t.DOLFIN_EPS), spline.assembleMatrix(F.MassForm())


def test_fast_diagonalization_iterations_do_not_grow():
    import tigar_amd as t
    its = {}
    for nel in (12, 24):
        A, B = _laplace3d(nel)
        for pc in ("fast_diagonalization",) + (("jacobi",) if nel == 24 else ()):
            s = t.SLEPcEigenSolver(A, B)
            s.parameters["preconditioner"] = pc
            s.solve(8)
            its[(nel, pc)] = s.last["iterations"]
            if pc == "fast_diagonalization":
                _check(s, A, B, 8)
    print("LOBPCG iterations", its)
    f12, f24 = its[(12, "fast_diagonalization")], its[(24, "fast_diagonalization")]
    assert max(f12, f24) <= 1.5 * min(f12, f24), its
    assert f24 < its[(24, "jacobi")], its


def test_none_and_jacobi_agree():
    import tigar_amd as t
    A, B = _laplace3d(6)
    lam = {}
    for pc in ("none", "jacobi"):
        s = t.SLEPcEigenSolver(A, B)
        s.parameters["preconditioner"] = pc
        s.solve(5)
        lam[pc] = np.array([s.get_eigenvalue(i)[0] for i in range(5)])
    assert np.all(np.abs(lam["none"] - lam["jacobi"]) <= 1e-8 * lam["jacobi"])


def test_reproducible_and_seed_independent():
    import tigar_amd as t
    A, B = _laplace3d(6)
    runs = []
    for seed in (0, 0, 7):
        s = t.SLEPcEigenSolver(A, B)
        s.parameters["seed"] = seed
        s.solve(5)
        runs.append((np.array([s.get_eigenvalue(i)[0] for i in range(5)]),
                     np.array([s.get_eigenpair(i)[2].get_local() for i in range(5)])))
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64))
    assert np.array_equal(runs[0][1].view(np.int64), runs[1][1].view(np.int64))
    assert np.all(np.abs(runs[2][0] - runs[0][0]) <= 1e-9 * runs[0][0])


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import tigar_amd as t
    from tigar_amd.device import DeviceCSR
    A, B = _laplace3d(4)
    Ah, Bh = A.to_scipy(), B.to_scipy()
    with pytest.raises(ValueError, match="not square"):
        t.SLEPcEigenSolver(Ah[:, :-1], Bh)
    with pytest.raises(ValueError):
        t.SLEPcEigenSolver(A, Bh[:-1, :-1])
    N = Ah.tolil()
    N[20, 21] += 0.5
    with pytest.raises(ValueError, match="not symmetric"):
        t.SLEPcEigenSolver(N.tocsr(), Bh).solve(3)
    with pytest.raises(RuntimeError, match="positive definite"):
        t.SLEPcEigenSolver(Ah, -Bh).solve(3)
    with pytest.raises(ValueError, match="at most 48"):
        t.SLEPcEigenSolver(A, B).solve(49)
    with pytest.raises(ValueError, match="free rows"):
        t.SLEPcEigenSolver(A, B).solve(22)          # 4^3 elements, p = 2: 216 dofs, 64 free; block of 22
    s = t.SLEPcEigenSolver(A, B)
    s.parameters["spectrum"] = "largest magnitude"
    with pytest.raises(ValueError, match="spectrum"):
        s.solve(3)
    s = t.SLEPcEigenSolver(Ah, Bh)
    s.parameters["preconditioner"] = "fast_diagonalization"
    with pytest.raises(ValueError, match="fast_diagonalization: K carries no tensor-product structure"):
        s.solve(3)

    class Two:
        size = 2
    with pytest.raises(NotImplementedError):
        t.SLEPcEigenSolver(A, B, comm=Two())
    with pytest.raises(NotImplementedError):
        t.SLEPcEigenSolver(DeviceCSR.from_scipy(Ah[:100, :]), DeviceCSR.from_scipy(Bh[:100, :]))
    s = t.SLEPcEigenSolver(A, B)
    s.parameters["maximum_iterations"] = 1
    with pytest.raises(RuntimeError, match="converged"):
        s.solve(5)
