"""One rank of the multi-field multi-rank -m gpu tests: several fields on one tensor basis (EqualOrderSpline(nF > 1))
split into z-slabs -- rows of K, M^T b, the Krylov solution and the prolongation of this rank, with the reference
(field-after-field) index of every local dof, written to ``outdir/rank<r>.npz``."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hashed(n, seed):
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 9007199254740992.0) - 1.0


def coupling_blocks(kind, S, pf, nz, c_planes=None):
    """Blocks (0, 1) and (1, 0) of an FE matrix whose fields 0 and 1 are coupled on a FEW nodes -- a constraint, penalty or
    contact term added by hand (tests/test_gpu_field_couplings.py).  ``S``: the element-coupling pattern of one field
    (n x n, node plane k = rows [k pf, (k + 1) pf), ``nz`` planes); entries of magnitude in [1, 2].

      a  one entry in (0, 1) on node plane 1, row and column the same node
      b  one entry in (0, 1), its row strictly between the middle and the last plane, its column on plane 3: a coupling
         between nodes of no common element
      c  the element-pattern entries of all rows of two adjacent interior planes in (0, 1), mirrored in (1, 0)
      d  as c, (1, 0) left empty
      e  the element-pattern entries of the rows of the first, the middle and the last plane: what three probes see
      f  both blocks empty"""
    import scipy.sparse as sp
    n = S.shape[0]
    rng = np.random.default_rng([5, ord(kind), n])
    rp = (nz // 2 + nz - 1) // 2 + 1                       # (17 planes: 13; 28 planes: 21)

    def values(k):
        return rng.uniform(1.0, 2.0, k) * rng.choice([-1.0, 1.0], k)

    def rows_of(planes):
        mask = np.zeros(n)
        for k in planes:
            mask[k * pf:(k + 1) * pf] = 1.0
        Bk = (sp.diags(mask) @ S).tocsr()
        Bk.eliminate_zeros()
        Bk.sort_indices()
        Bk.data = values(Bk.nnz)
        return Bk
    empty = sp.csr_matrix((n, n))
    if kind == "a":
        i = 1 * pf + pf // 2
        return sp.csr_matrix((values(1), ([i], [i])), shape=(n, n)), empty
    if kind == "b":
        return sp.csr_matrix((values(1), ([rp * pf + pf // 2], [3 * pf + pf // 3])), shape=(n, n)), empty
    if kind in ("c", "d"):
        Bk = rows_of(c_planes if c_planes is not None else (rp - 1, rp))
        return Bk, (Bk.T.tocsr() if kind == "c" else empty)
    if kind == "e":
        Bk = rows_of((0, nz // 2, nz - 1))
        return Bk, Bk.T.tocsr()
    assert kind == "f"
    return empty, empty


def coupled_fe_matrix(diag_blocks, kind, pf, nz, c_planes=None):
    """(A, A without its off-diagonal blocks): the diagonal blocks given, blocks (0, 1) / (1, 0) from ``coupling_blocks``"""
    import scipy.sparse as sp
    nF = len(diag_blocks)
    S = diag_blocks[0].tocsr().copy()
    S.data[:] = 1.0
    B01, B10 = coupling_blocks(kind, S, pf, nz, c_planes)
    blocks = [[diag_blocks[a] if a == b else None for b in range(nF)] for a in range(nF)]
    A0 = sp.bmat(blocks, format="csr")
    blocks[0][1], blocks[1][0] = B01, B10
    A = sp.bmat(blocks, format="csr")
    A.sort_indices()
    A0.sort_indices()
    return A, A0


def coupled_space(space, kind, comm):
    """(generator, spline, A, A without the couplings) of a field-coupling case: ``space`` "eq3d" (two fields, p = 2, 3 x 3 x 8
    elements: 833 FE rows per field on 17 node planes), "eq2d" (two fields, p = 3, 4 x 9 elements: 13 x 28 nodes), "rt3d"
    (BSplineCompat "RT" of degrees 1, 1, 1 on 3 x 4 x 8 elements: three fields on different bases, 7 x 9 x 17 nodes)"""
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    if space == "rt3d":
        from tigar_amd.compatibleSplines import BSplineCompat
        degs, nels = [1, 1, 1], [3, 4, 8]
        kv = [B.uniformKnots(degs[k], 0., 1. + 0.25 * k, nels[k]) for k in range(3)]
        gen = BSplineCompat(comm, B.ExplicitBSplineControlMesh(degs, kv), "RT", degs)
        for f in range(3):
            gen.addZeroDofs(f, gen.getFieldSpline(f).getSideDofs(2, 0))
        spline = t.ExtractedSpline(gen, 4)
        nfe = spline.V.dim() // 3
        Ae = F.ElasticityForm(2.0, 1.0).assemble_matrix(spline.V).to_scipy().tocsr()
        diag_blocks = [Ae[f * nfe:(f + 1) * nfe, f * nfe:(f + 1) * nfe].tocsr() for f in range(3)]
        # (rank 1 of 2 owns the dof planes 5 .. 9; its FE rows of the fields of degree 1 in z are the node planes 8 .. 16, of
        #  the field of degree 2 the planes 6 .. 16 -- localFERange(): first / middle / last 8 / 12 / 16 and 6 / 11 / 16)
        pf, nz, c_planes = 7 * 9, 17, (13, 14)
    else:
        d, p, nels = (3, 2, [3, 3, 8]) if space == "eq3d" else (2, 3, [4, 9])
        kv = [B.uniformKnots(p, 0., 1., nels[k]) for k in range(d)]
        gen = t.EqualOrderSpline(comm, 2, B.ExplicitBSplineControlMesh([p] * d, kv))
        for f in range(2):
            gen.addZeroDofs(f, gen.getScalarSpline(f).getSideDofs(d - 1, 0))
        spline = t.ExtractedSpline(gen, 2 * p)
        V1 = t.TensorFunctionSpace([gen.getScalarSpline(0).generateMesh(degree=p)], "Lagrange")
        A1 = (F.LaplaceForm().assemble_matrix(V1).to_scipy() + 0.7 * F.MassForm().assemble_matrix(V1).to_scipy()).tocsr()
        A1.sort_indices()
        diag_blocks = [A1, A1]
        # (eq3d: 10 dof planes; rank 1 of 2 owns the planes 5 .. 9, whose supports are the node planes 6 .. 16 --
        #  localFERange() is (6 * 49, 17 * 49) per field: first / middle / last plane 6 / 11 / 16; rank 1 of 3 owns the dof
        #  planes 4 .. 6, node planes 4 .. 14: 4 / 9 / 14.  Case b sits on plane 13, case c on the planes 12 and 13.)
        pf, nz, c_planes = int(np.prod([p * n + 1 for n in nels[:-1]])), p * nels[-1] + 1, None
    A, A0 = coupled_fe_matrix(diag_blocks, kind, pf, nz, c_planes)
    assert A.shape[0] == spline.V.dim()
    return gen, spline, A, A0


def solver_parameters(case):
    """Krylov parameters of a case beyond the method, for the ranks and for the single-rank run they are compared with.
    Couplings of magnitude 1 .. 2 beside diagonal blocks of the size of h make K indefinite (eq3d, case c: eigenvalues
    -9.7 .. 10.3, condition 850): GMRES(30) stagnates, one cycle of 200 converges in about 190 steps; the tolerance is
    tightened by that condition number so that two converged solutions agree to the 1e-8 the tests ask for."""
    return {"gmres_restart": 200, "relative_tolerance": 1e-12} if case.startswith("couple_") else {}


def couples_beyond_the_halo(case):
    """case b couples a node of plane 13 with one of plane 3: on several ranks that column of K lies outside the dofs and halo
    planes a rank's Krylov vectors hold, and ``solveLinearSystem`` says so instead of multiplying"""
    return case.startswith("couple_") and case.endswith("_b")


def problem(case, comm):
    """(generator, spline, K, rhs, solver method) of a test case, through the public API on communicator ``comm``"""
    import scipy.sparse as sp
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    if case.startswith("couple_"):
        # couple_<space>_<kind>: fields coupled on a few nodes, inside rank 1's rows and off the first, the middle and the last
        # node plane of them (``coupled_space``)
        _, space, kind = case.split("_")
        gen, spline, A, _ = coupled_space(space, kind, comm)
        K = spline.extractMatrix(A, diag=1.5)
        rhs = spline.extractVector(hashed(A.shape[0], 81))
        return gen, spline, K, rhs, "gmres"
    if case == "rt3d":
        # the space of demos/taylor-green/taylor-green-3d.py:42-50: BSplineCompat("RT") -- three fields on DIFFERENT bases (one
        # degree higher along their own direction) over one Q_(k+1) node grid, normal-direction boundary conditions
        from tigar_amd.compatibleSplines import BSplineCompat
        degs = [int(v) for v in os.environ.get("TIGAR_TEST_FDEGS", "1,1,1").split(",")]
        nels = [int(v) for v in os.environ.get("TIGAR_TEST_FNELS", "5,4,9").split(",")]
        kv = [B.uniformKnots(degs[k], 0., 1. + 0.25 * k, nels[k]) for k in range(3)]
        gen = BSplineCompat(comm, B.ExplicitBSplineControlMesh(degs, kv), "RT", degs)
        for f in range(3):
            s0 = gen.getFieldSpline(f)
            for side in (0, 1):
                gen.addZeroDofs(f, s0.getSideDofs(f, side))
        spline = t.ExtractedSpline(gen, 2 * (max(degs) + 1))
        K = spline.assembleMatrix(F.ElasticityForm(2.0, 1.0), diag=1.5)
        rhs = spline.extractVector(hashed(spline.V.dim(), 79))
        return gen, spline, K, rhs, "gmres"
    if case == "mapped_elasticity3d":
        # three displacement fields on a rational volume (a NURBS control mesh): ElasticityForm(geometry=...) hands out row
        # blocks of its nine field blocks from the element kernels, on the control-function window of the rank's slab
        from tigar_amd import NURBS
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from geom_util import rational_volume
        p = int(os.environ.get("TIGAR_TEST_FP", 2))
        nels = [int(v) for v in os.environ["TIGAR_TEST_FNELS"].split(",")] if os.environ.get("TIGAR_TEST_FNELS") else [4, 3, 7]
        kvs, C = rational_volume(p, nels)
        gen = t.EqualOrderSpline(comm, 3, NURBS.NURBSControlMesh([p] * 3, kvs, C))
        for f in range(3):
            gen.addZeroDofs(f, gen.getScalarSpline(f).getSideDofs(2, 0))
        spline = t.ExtractedSpline(gen, 2 * p)
        K = spline.assembleMatrix(F.ElasticityForm(2.0, 1.0, geometry=gen), diag=1.5)
        rhs = spline.extractVector(hashed(spline.V.dim(), 80))
        return gen, spline, K, rhs, "cg"
    if case == "shell2d":            # cfg5-like: 2-D p=3, three fields, hashed non-symmetric A on the 3-field pattern
        d, p, nel, nF, method = 2, 3, 14, 3, "gmres"
    else:                            # 3-D elasticity, p=2, three fields (ElasticityForm: blocks as Kronecker sums)
        d, p, nel, nF, method = 3, 2, 7, 3, "cg"
    # (optional overrides, set by the tests for both the single-rank reference and the ranks: degree, element counts per
    #  direction, periodic directions other than the last)
    p = int(os.environ.get("TIGAR_TEST_FP", p))
    nels = [int(v) for v in os.environ["TIGAR_TEST_FNELS"].split(",")] if os.environ.get("TIGAR_TEST_FNELS") else [nel] * d
    per = set(int(c) for c in os.environ.get("TIGAR_TEST_FPER", ""))
    kv = [B.uniformKnots(p, 0., 1., nels[k], k in per) for k in range(d)]
    gen = t.EqualOrderSpline(comm, nF, B.ExplicitBSplineControlMesh([p] * d, kv))
    for f in range(nF):
        s0 = gen.getScalarSpline(f)
        if case == "shell2d":
            gen.addZeroDofs(f, s0.getSideDofs(0, 0, nLayers=2))
        else:
            gen.addZeroDofs(f, s0.getSideDofs(d - 1, 0))
    spline = t.ExtractedSpline(gen, 2 * p)
    nfe = spline.V.dim() // nF
    if case == "shell2d":
        pat = F.LaplaceForm().assemble_matrix(t.TensorFunctionSpace([gen.getScalarSpline(0).generateMesh(degree=p)],
                                                                    "Lagrange")).to_scipy().tocsr()
        pat.sort_indices()
        blocks = [[None] * nF for _ in range(nF)]
        for a in range(nF):
            for b in range(nF):
                Bk = pat.copy()
                Bk.data = 0.05 * hashed(Bk.nnz, 3 * a + b)
                blocks[a][b] = Bk if a != b else (Bk + 4.0 * sp.identity(nfe, format="csr")).tocsr()
        A = sp.bmat(blocks, format="csr")
        K = spline.extractMatrix(A, diag=1.5)
        rhs = spline.extractVector(hashed(A.shape[0], 77))
    else:
        K = spline.assembleMatrix(F.ElasticityForm(2.0, 1.0), diag=1.5)
        rhs = spline.extractVector(hashed(spline.V.dim(), 78))
    return gen, spline, K, rhs, method


def main():
    outdir, case = sys.argv[1], sys.argv[2]
    import tigar_amd as t
    from tigar_amd import common as tc, device as dev
    comm = tc.worldcomm
    dcomm = comm.device()
    gen, spline, K, rhs, method = problem(case, comm)
    assert getattr(gen.M, "is_implicit", False) and gen.M.nfields >= 2
    solver = t.PETScKrylovSolver(method, "jacobi")
    solver.parameters["relative_tolerance"] = 1e-10
    solver.parameters.update(solver_parameters(case))
    spline.setSolverOptions(linearSolver=solver)
    u = t.Function(spline.V, spline.localFERange())
    dev.prof_reset()
    refused = ""
    try:
        U = spline.solveLinearSystem(K, rhs, u)
    except NotImplementedError as e:
        # a K that couples dofs beyond the halo of the Krylov vectors (``couples_beyond_the_halo``): refused on every rank,
        # before anything is multiplied; the rows of K and M^T b are still compared
        if not couples_beyond_the_halo(case):
            raise
        refused, U, solver.last = str(e), t.Function(spline.V, spline.localFERange()).vector(), {"iterations": -1}
    Ks = K.to_scipy()
    np.savez(os.path.join(outdir, "rank%d.npz" % comm.rank), dofs=spline.localDofIndices(),
             new_of_old=spline._slab_path().new_of_old(), g=np.array(spline.localDofRange()),
             fe=np.array(spline.localFERange()), K_indptr=Ks.indptr, K_indices=Ks.indices, K_data=Ks.data,
             rhs=rhs.get_local(), U=U.get_local(), u=u.vector().get_local(), its=np.array([solver.last["iterations"]]),
             refused=np.array([refused]), host_waits=np.array([dev.prof_get(4)[1]]), kind=np.array([dev.Comm.KINDS.index(dcomm.info()[2])]))
    comm.barrier()


if __name__ == "__main__":
    main()
