"""GPU: the fast diagonalization preconditioner (tigar_amd/fastdiag.py, csrc/tg_fd.hip) -- the device application against a
dense scipy inverse, FD-CG on unmapped and mapped Poisson, mass, elasticity, setup reuse and the refusals."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu


def _spline(d, p, nels, nf=1, faces="all", kv=None):
    import tigar_amd as t
    from tigar_amd import BSplines as B
    kv = kv or [B.uniformKnots(p, 0.0, 1.0, n) for n in nels]
    gen = t.EqualOrderSpline(nf, B.ExplicitBSplineControlMesh([p] * d, kv))
    sc = gen.getScalarSpline(0)
    for f in range(nf):
        for direction in range(d):
            for side in (0, 1):
                if faces == "all" or (direction, side) in faces:
                    gen.addZeroDofs(f, sc.getSideDofs(direction, side))
    return gen, t.ExtractedSpline(gen, 2 * p)


def _solver(rtol, pc="fast_diagonalization"):
    import tigar_amd as t
    s = t.PETScKrylovSolver("cg", pc)
    s.parameters["relative_tolerance"] = rtol
    return s


def _dense_p(kx, lo, hi, coef):
    """P on the free box from 1-D IGA matrices built here (M1^T K_fe M1)"""
    from tigar_amd.forms import fe_matrices_1d
    d = kx.d
    Ks, Ms = [], []
    for k in range(d):
        Mfe, Kfe = fe_matrices_1d(kx.grid.vertices[k], kx.grid.degree)
        M1 = kx.M1[k].toarray()
        Ks.append((M1.T @ Kfe.toarray() @ M1)[lo[k]:hi[k], lo[k]:hi[k]])
        Ms.append((M1.T @ Mfe.toarray() @ M1)[lo[k]:hi[k], lo[k]:hi[k]])

    def kron(mats):                      # direction 0 fastest
        out = np.ones((1, 1))
        for m in mats[::-1]:
            out = np.kron(out, m)
        return out
    P = coef[d] * kron(Ms)
    for k in range(d):
        P = P + coef[k] * kron([Ks[j] if j == k else Ms[j] for j in range(d)])
    return P


@pytest.mark.parametrize("d,p,nels,coef,scaling", [
    (2, 2, (10, 8), (1.0, 2.5, 0.0), "none"),
    (2, 3, (9, 7), (1.0, 0.5, 3.0), "diagonal"),
    (3, 2, (6, 5, 4), (1.0, 2.0, 0.5, 0.0), "diagonal"),
    (3, 3, (5, 4, 3), (0.7, 1.0, 1.3, 2.0), "none"),
])
def test_apply_matches_dense(d, p, nels, coef, scaling):
    import tigar_amd as t
    from tigar_amd.device import DeviceVector
    from tigar_amd.forms import LaplaceForm
    gen, spline = _spline(d, p, nels)
    K = spline.assembleMatrix(LaplaceForm())
    fd = t.FastDiagonalization(K, coefficients=coef, scaling=scaling)
    shape = K.tensor_structure.shape
    assert shape == [n + p for n in nels]
    n = K.shape[0]
    rng = np.random.default_rng(3)
    r = rng.standard_normal(n)
    z1, z2 = DeviceVector(n), DeviceVector(n)
    fd.apply(DeviceVector(data=r), z1)
    fd.apply(DeviceVector(data=r), z2)
    a, b = z1.get_local(), z2.get_local()
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), "two applications differ in bits"
    lo, hi = [1] * d, [s - 1 for s in shape]
    P = _dense_p(K.tensor_structure.kx, lo, hi, coef)
    grid = np.arange(n).reshape(shape[::-1])
    free = grid[tuple(slice(lo[d - 1 - a], hi[d - 1 - a]) for a in range(d))].ravel()
    Ks = K.to_scipy()
    dK = Ks.diagonal()
    S = np.sqrt(np.diag(P) / dK[free]) if scaling == "diagonal" else np.ones(free.size)
    want = dK ** -1 * r
    want[free] = S * np.linalg.solve(P, S * r[free])
    assert np.linalg.norm(a - want) <= 1e-12 * np.linalg.norm(want)


# relative 2-norm of B (K x) - x on the free dofs of _identity_case() with B evaluated by the float64 numpy reference of
# tests/fd_reference.py and K x by scipy from K.to_scipy(): 1.02e-14 (9.8e-15 with the reference in longdouble; the kernel gave 7.7e-15 on an MI355X) (measured; the error is the conditioning of P, 2.4e3 by its
# eigenvalue sums, times a few unit roundoffs, whatever evaluates B)
IDENTITY_HOST_ERROR = 1.02e-14


def _identity_case():
    """unmapped Laplace, p = 3, 62 x 30 x 14 elements: free box 63 x 31 x 15, padded to 64 x 32 x 16 (all different, and
    none the 16 x 16 x 16 of test_apply_matches_dense); P with coefficients (1, 1, 1, 0) is K on the free dofs"""
    import tigar_amd as t
    from tigar_amd.forms import LaplaceForm
    gen, spline = _spline(3, 3, (62, 30, 14))
    K = spline.assembleMatrix(LaplaceForm())
    fd = t.FastDiagonalization(K, coefficients=(1.0, 1.0, 1.0, 0.0), scaling="none")
    shape = K.tensor_structure.shape
    assert shape == [65, 33, 17]
    grid = np.arange(K.shape[0]).reshape(shape[::-1])
    free = grid[1:-1, 1:-1, 1:-1].ravel()
    x = np.zeros(K.shape[0])
    x[free] = np.random.default_rng(12).standard_normal(free.size)
    return K, fd, free, x


def test_apply_inverts_k_on_a_noncubic_box():
    from tigar_amd.device import DeviceVector
    K, fd, free, x = _identity_case()
    y = DeviceVector(K.shape[0])
    K.mult(DeviceVector(data=x), y)
    z = DeviceVector(data=np.full(K.shape[0], np.nan))
    fd.apply(y, z)
    z = z.get_local()
    assert np.all(np.isfinite(z))
    err = np.linalg.norm(z[free] - x[free]) / np.linalg.norm(x[free])
    print("FD identity: kernel %.3g, 4 x host %.3g" % (err, 4 * IDENTITY_HOST_ERROR))
    assert err <= 4 * IDENTITY_HOST_ERROR


def _poisson(d, p, nel, pc, rtol):
    import tigar_amd as t
    from tigar_amd import forms as F
    gen, spline = _spline(d, p, [nel] * d)
    solver = _solver(rtol, pc)
    spline.setSolverOptions(linearSolver=solver)
    f = lambda x: np.sin(np.pi * x)
    u = t.Function(spline.V)
    eq = F.Equation(F.LaplaceForm(), F.SeparableLoadForm([f] * d, scale=d * np.pi ** 2))
    U = spline.solveLinearVariationalProblem(eq, u)
    return spline, solver, U.get_local(), eq


@pytest.mark.parametrize("d,p,nel", [(3, 3, 24), (2, 4, 96)])
def test_unmapped_poisson(d, p, nel):
    spline, solver, U, eq = _poisson(d, p, nel, "fast_diagonalization", 1e-10)
    assert solver.last["preconditioner"] == "fast_diagonalization"
    assert solver.last["iterations"] <= 3
    c = solver.last["fd"]["coefficients"][0]
    assert np.allclose(c, [1.0] * d + [0.0], atol=1e-8)
    K, b = spline.assembleLinearSystem(eq.lhs, eq.rhs)
    if d == 2:
        Uref = spla.spsolve(K.to_scipy().tocsc(), b.get_local())
    else:
        # (a sparse LU of the 3-D system takes a minute on the host: the library's direct solver, no FD involved)
        import tigar_amd as t
        from tigar_amd.device import DeviceVector
        x = DeviceVector(K.shape[0])
        t.PETScLUSolver().solve(K, x, b)
        Uref = x.get_local()
    assert np.linalg.norm(U - Uref) <= 1e-8 * np.linalg.norm(Uref)


def test_mass_form():
    import tigar_amd as t
    from tigar_amd import forms as F
    gen, spline = _spline(3, 2, [8, 7, 6])
    solver = _solver(1e-10)
    spline.setSolverOptions(linearSolver=solver)
    u = t.Function(spline.V)
    spline.solveLinearVariationalProblem(F.Equation(F.MassForm(), F.SeparableLoadForm([lambda x: 1.0 + x] * 3)), u)
    assert solver.last["iterations"] <= 3
    assert np.allclose(solver.last["fd"]["coefficients"][0], [0.0, 0.0, 0.0, 1.0], atol=1e-10)


def _rational_volume(p, nel):
    from tigar_amd.BSplines import uniformKnots
    from tigar_amd.NURBS import NURBSControlMesh
    kv = np.asarray(uniformKnots(p, 0.0, 1.0, nel), dtype=np.float64)
    g = np.array([np.sum(kv[i + 1:i + p + 1]) / p for i in range(len(kv) - p - 1)])
    g0, g1, g2 = g[:, None, None], g[None, :, None], g[None, None, :]
    w = 1.0 + 0.25 * g0 * g1 + 0.1 * g2
    C = np.empty((len(g), len(g), len(g), 4))
    C[..., 0] = w * (g0 + 0.15 * g1 * g2)
    C[..., 1] = w * (g1 + 0.2 * g0 ** 2 - 0.1 * g2)
    C[..., 2] = w * (g2 * (1.0 + 0.3 * g0) + 0.05 * np.sin(2.0 * g1))
    C[..., 3] = w
    return NURBSControlMesh([p] * 3, [kv] * 3, C)


def _mapped_solve(nel, pc, rtol, p=3):
    import tigar_amd as t
    from tigar_amd import forms as F
    gen = t.EqualOrderSpline(1, _rational_volume(p, nel))
    sc = gen.getScalarSpline(0)
    for direction in range(3):
        for side in (0, 1):
            gen.addZeroDofs(0, sc.getSideDofs(direction, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    K = spline.assembleMatrix(F.LaplaceForm(geometry=gen))
    b = spline.assembleVector(F.NodalLoadForm(1.0, gen))
    solver = _solver(rtol, pc)
    spline.setSolverOptions(linearSolver=solver)
    U = spline.solveLinearSystem(K, b, t.Function(spline.V))
    return solver.last["iterations"], U.get_local()


def test_mapped_poisson():
    its = {}
    for nel in (8, 16, 24):
        its[nel], U = _mapped_solve(nel, "fast_diagonalization", 1e-10)
        assert its[nel] <= 20, its
    assert its[24] - its[8] <= 3, its
    itj, Uj = _mapped_solve(24, "jacobi", 1e-10)
    assert its[24] <= itj / 4.0, (its, itj)
    assert np.linalg.norm(U - Uj) <= 1e-7 * np.linalg.norm(Uj)


def test_elasticity_three_fields():
    import tigar_amd as t
    from tigar_amd import forms as F
    res = {}
    for pc in ("fast_diagonalization", "jacobi"):
        gen, spline = _spline(3, 2, [6, 5, 4], nf=3)
        solver = _solver(1e-10, pc)
        spline.setSolverOptions(linearSolver=solver)
        K = spline.assembleMatrix(F.ElasticityForm(lmbda=2.0, mu=1.0))
        bb = np.cos(np.arange(K.shape[0]) * 0.37)
        bb[np.asarray(spline.zeroDofs)] = 0.0
        from tigar_amd.device import DeviceVector
        U = spline.solveLinearSystem(K, DeviceVector(data=bb), t.Function(spline.V))
        res[pc] = (solver.last["iterations"], U.get_local())
    assert res["fast_diagonalization"][0] < res["jacobi"][0], res
    Uf, Uj = res["fast_diagonalization"][1], res["jacobi"][1]
    assert np.linalg.norm(Uf - Uj) <= 1e-7 * np.linalg.norm(Uj)


def test_setup_reused():
    spline, solver, U, eq = _poisson(3, 2, 10, "fast_diagonalization", 1e-10)
    assert solver.last["fd"]["setup_reused"] is False
    import tigar_amd as t
    spline.solveLinearVariationalProblem(eq, t.Function(spline.V))
    assert solver.last["fd"]["setup_reused"] is True


def test_refusals():
    import tigar_amd as t
    from tigar_amd import forms as F
    from tigar_amd.device import DeviceCSR, DeviceVector
    with pytest.raises(ValueError, match="cg only"):
        t.PETScKrylovSolver("gmres", "fast_diagonalization")
    gen, spline = _spline(2, 2, [6, 6])
    K = spline.assembleMatrix(F.LaplaceForm())
    b = DeviceVector(data=np.ones(K.shape[0]))
    raw = DeviceCSR.from_scipy(K.to_scipy())
    with pytest.raises(ValueError, match="no tensor-product structure"):
        _solver(1e-8).solve(raw, DeviceVector(K.shape[0]), b)
    # partial face: half of one side
    import tigar_amd as tt
    from tigar_amd import BSplines as B
    gen2 = tt.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], [B.uniformKnots(2, 0.0, 1.0, 6)] * 2))
    side = gen2.getScalarSpline(0).getSideDofs(0, 0)
    gen2.addZeroDofs(0, side[:len(side) // 2])
    sp2 = tt.ExtractedSpline(gen2, 4)
    K2 = sp2.assembleMatrix(F.LaplaceForm())
    with pytest.raises(ValueError, match="whole faces"):
        _solver(1e-8).solve(K2, DeviceVector(K2.shape[0]), DeviceVector(data=np.ones(K2.shape[0])))
    # permuted generator
    gen3 = tt.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([2, 2], [B.uniformKnots(2, 0.0, 1.0, 8)] * 2))
    gen3.applyPermutation(nparts=3, fe_owner=np.random.default_rng(1).integers(0, 3, size=gen3.V.dim()))
    assert not np.array_equal(gen3.permutation, np.arange(gen3.permutation.size))
    sp3 = tt.ExtractedSpline(gen3, 4, doPermutation=False)
    K3 = sp3.assembleMatrix(F.LaplaceForm())
    with pytest.raises(ValueError, match="permutation"):
        _solver(1e-8).solve(K3, DeviceVector(K3.shape[0]), DeviceVector(data=np.ones(K3.shape[0])))
