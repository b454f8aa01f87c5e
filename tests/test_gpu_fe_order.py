"""GPU: FE operands in the caller's dof order (tigar_amd/feorder.py, csrc/tg_feorder.hip).  Every comparison is exact
(integer arrays equal, fp64 compared as int64 views) unless a tolerance is named.  The numpy / scipy reference is
tests/fe_order_reference.py."""
import gc
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import tigar_oracle as O
import fe_order_reference as R
from test_fe_order_host import golden_patches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import tigar_amd
    from tigar_amd import BSplines, forms, device, feorder
    device.device_info()

    class NS:
        pass
    ns = NS()
    ns.t, ns.B, ns.F, ns.dev, ns.fo = tigar_amd, BSplines, forms, device, feorder
    return ns


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_csr(X, Y):
    return (X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(bits(X.data), bits(Y.data)))


def live_blocks(dev):
    gc.collect()
    dev.sync()
    return dev.pool_stats()[2]


# ---- 1: tg_nodes_locate ----------------------------------------------------------------------------------------------
def test_locate_matches_the_reference_on_the_golden_patches(T):
    rng = np.random.default_rng(5)
    seen = set()
    n = 0
    for name, degs, kvs in golden_patches():
        X, axes = O.fe_node_grid(O.BSpline(degs, kvs))
        seen.add(len(axes))
        perm = rng.permutation(X.shape[0])
        Xp = X[perm]
        g_ref, inv_ref, _ = R.locate([axes], Xp)
        order = T.fo.FEOrder.locate([axes], Xp)
        assert np.array_equal(order.grid_of_fe, g_ref) and np.array_equal(order.fe_of_grid, inv_ref), name
        assert np.array_equal(order.grid_of_fe, perm) and order.max_snap == 0.0 and order.n == X.shape[0], name
        assert order.is_identity == bool(np.array_equal(perm, np.arange(len(perm)))), name
        # three fields on the one grid, rows interleaved node by node
        f = np.tile(np.arange(3), X.shape[0])
        X3 = np.repeat(Xp, 3, axis=0)
        g3_ref, inv3_ref, _ = R.locate([axes] * 3, X3, f)
        order3 = T.fo.FEOrder.locate([axes] * 3, X3, f)
        assert np.array_equal(order3.grid_of_fe, g3_ref) and np.array_equal(order3.fe_of_grid, inv3_ref), name
        # coordinates moved by +-1..4 ulp: the same permutation, and the distance is reported
        Xm = Xp.copy()
        for _ in range(4):
            step = rng.integers(-1, 2, size=Xm.shape)
            Xm = np.where(step > 0, np.nextafter(Xm, np.inf), np.where(step < 0, np.nextafter(Xm, -np.inf), Xm))
        Xm[0] = np.nextafter(Xp[0], np.inf)
        _, _, snap_ref = R.locate([axes], Xm)
        moved = T.fo.FEOrder.locate([axes], Xm)
        assert np.array_equal(moved.grid_of_fe, perm), name
        assert moved.max_snap > 0.0 and moved.max_snap == snap_ref, name
        n += 1
    assert n == 56 and seen == {1, 2, 3}


def test_locate_declines_with_the_reason_and_keeps_nothing(T):
    rng = np.random.default_rng(6)
    cases = 0
    for name, degs, kvs in list(golden_patches())[::4]:
        X, axes = O.fe_node_grid(O.BSpline(degs, kvs))
        if X.shape[0] < 6:
            continue
        perm = rng.permutation(X.shape[0])
        Xp = X[perm]
        row, k = int(rng.integers(0, X.shape[0])), int(rng.integers(0, len(axes)))
        off = Xp.copy()
        off[row, k] += 0.3 * np.min(np.diff(axes[k]))
        dup = Xp.copy()
        a, b = sorted(rng.choice(X.shape[0], 2, replace=False).tolist())
        dup[b] = dup[a]
        f = np.tile(np.arange(3), X.shape[0])
        fw = f.copy()
        fw[4] = 0                                       # row 4 is node perm[1] of field 1, labelled field 0
        inputs = [("off the grid", "row %d " % row, [axes], off, None),
                  ("two rows on one node", "rows %d and %d " % (a, b), [axes], dup, None),
                  ("wrong row count", "%d rows" % (X.shape[0] - 1), [axes], Xp[:-1], None),
                  ("node of another field", "row 4 ", [axes] * 3, np.repeat(Xp, 3, axis=0), fw)]
        for reason, where, fa, x, fields in inputs:
            with pytest.raises(R.Declined) as ref:
                R.locate(fa, x, fields)
            assert ref.value.reason == reason
            before = live_blocks(T.dev)
            with pytest.raises(ValueError) as e:
                T.fo.FEOrder.locate(fa, x, fields)
            assert reason in str(e.value) and where in str(e.value), (name, reason, str(e.value))
            assert live_blocks(T.dev) == before, (name, reason)
            cases += 1
    assert cases >= 32
    # fields on different grids: a row of field 0 that sits on a node field 1 alone has
    fine = np.linspace(0.0, 1.0, 9)
    coarse = np.linspace(0.0, 1.0, 5)
    x = np.concatenate([coarse, fine]).reshape(-1, 1)
    f = np.array([0] * 5 + [1] * 9)
    assert np.array_equal(T.fo.FEOrder.locate([[coarse], [fine]], x, f).grid_of_fe, np.arange(14))
    x[2] = fine[3]
    with pytest.raises(ValueError) as e:
        T.fo.FEOrder.locate([[coarse], [fine]], x, f)
    assert "row 2 is a node of another field" in str(e.value)
    with pytest.raises(ValueError):
        T.fo.FEOrder.from_permutation([0, 2, 2, 1])


# ---- 2: tg_csr_permute_sym -------------------------------------------------------------------------------------------
def _matrix_with_rows_of(rng, n, lengths):
    """random sparse matrix whose first rows hold exactly ``lengths`` entries (0 = an empty row), the rest a few"""
    rows, cols = [], []
    for r in range(n):
        ln = lengths[r] if r < len(lengths) else int(rng.integers(0, 9))
        c = rng.choice(n, ln, replace=False)
        rows += [r] * ln
        cols += c.tolist()
    vals = rng.standard_normal(len(rows))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def test_permute_sym_matches_scipy(T):
    rng = np.random.default_rng(8)
    n = 4000
    lengths = [0, 1, 0, 64, 65, 343, 729, 1029, 3001, 128, 129, 2048, 2049, 512, 513, 0]
    A = _matrix_with_rows_of(rng, n, lengths)
    assert sorted(set(np.diff(A.indptr)[:len(lengths)])) == sorted(set(lengths))
    Ad = T.dev.DeviceCSR.from_scipy(A)
    for kind in ("random", "reversal", "identity"):
        g = {"random": rng.permutation(n), "reversal": np.arange(n)[::-1].copy(), "identity": np.arange(n)}[kind]
        order = T.fo.FEOrder.from_permutation(g)
        assert order.is_identity == (kind == "identity")
        Bd = order.permute_matrix(Ad)
        if kind == "identity":
            assert Bd is Ad
            continue
        B, Bref = Bd.to_scipy(), R.permute_sym(A, g)
        assert not Bd.is_loose()
        assert same_csr(B, Bref), kind
        # the parent commit's two calls give the same matrix
        inv = np.empty(n, dtype=np.int64)
        inv[g] = np.arange(n)
        old = Ad.gather_rows(inv).permute_columns(g).to_scipy()
        assert same_csr(B, old), kind
        # and the inverse brings A back
        assert same_csr(order.permute_matrix(Bd, inverse=True).to_scipy(), A), kind
        inv_order = T.fo.FEOrder.from_permutation(inv)
        assert same_csr(inv_order.permute_matrix(Bd).to_scipy(), A), kind
    order = T.fo.FEOrder.from_permutation(rng.permutation(n))
    with pytest.raises(ValueError):
        order.permute_matrix(T.dev.DeviceCSR.from_scipy(sp.identity(n + 1, format="csr")))
    with pytest.raises(ValueError):
        order.permute_matrix(T.dev.DeviceCSR.from_scipy(sp.csr_matrix((n, n + 1))))


# ---- 3: tg_vec_permute -----------------------------------------------------------------------------------------------
def test_vec_permute_both_directions(T):
    rng = np.random.default_rng(9)
    n = 100003
    g = rng.permutation(n)
    order = T.fo.FEOrder.from_permutation(g)
    x = rng.standard_normal(n)
    xg = order.to_grid(x)
    assert np.array_equal(bits(xg.get_local()), bits(R.vec_to_grid(x, g)))
    out = T.dev.DeviceVector(n)
    assert order.to_caller(xg, out=out) is out
    assert np.array_equal(bits(out.get_local()), bits(x))
    assert np.array_equal(bits(order.to_caller(T.dev.DeviceVector(data=x)).get_local()), bits(R.vec_to_caller(x, g)))
    ident = T.fo.FEOrder.from_permutation(np.arange(n))
    v = T.dev.DeviceVector(data=x)
    assert ident.to_grid(v) is v and ident.to_caller(v) is v


# ---- 4-5, 8: the API on a caller-ordered scalar space ----------------------------------------------------------------
class FakePETScMat(object):
    """what petsc4py's Mat offers of the operand"""

    def __init__(self, A):
        self._A = sp.csr_matrix(A)

    def getValuesCSR(self):
        return self._A.indptr.astype(np.int32), self._A.indices.astype(np.int32), self._A.data.copy()

    def getSize(self):
        return self._A.shape


class FakeDolfinMatrix(object):
    """what dolfin's PETScMatrix offers: .mat()"""

    def __init__(self, A):
        self._m = FakePETScMat(A)

    def mat(self):
        return self._m


class FakePETScVec(object):
    def __init__(self, b):
        self._b = np.array(b, dtype=np.float64)

    def getArray(self):
        return self._b


class FakeDolfinVector(object):
    def __init__(self, b):
        self._v = FakePETScVec(b)

    def vec(self):
        return self._v


class FakeGenericVector(object):
    def __init__(self, b):
        self._b = np.array(b, dtype=np.float64)

    def get_local(self):
        return self._b.copy()


def _poisson_pair(T, d, p, nel, seed, fe_nodes="random"):
    """(grid-ordered spline, caller-ordered spline, perm, X): zero dofs on all faces"""
    t, B = T.t, T.B
    kv = [B.uniformKnots(p, 0.0, 1.0, nel) for _ in range(d)]
    out = []
    X = perm = None
    for caller in (False, True):
        cm = B.ExplicitBSplineControlMesh([p] * d, kv)
        if caller:
            X = gen.V.tabulate_dof_coordinates()
            n = X.shape[0]
            perm = np.random.default_rng(seed).permutation(n) if fe_nodes == "random" else np.arange(n)
            gen = t.EqualOrderSpline(1, cm, fe_nodes=X[perm])
        else:
            gen = t.EqualOrderSpline(1, cm)
        s0 = gen.getScalarSpline(0)
        for direction in range(d):
            for side in (0, 1):
                gen.addZeroDofs(0, s0.getSideDofs(direction, side))
        out.append(t.ExtractedSpline(gen, 2 * p))
    return out[0], out[1], perm, X


@pytest.mark.parametrize("d,p,nel", [(2, 2, 16), (2, 3, 10), (3, 2, 6), (3, 3, 5)])
def test_poisson_in_the_callers_order(T, d, p, nel):
    t, F = T.t, T.F
    plain, caller, perm, X = _poisson_pair(T, d, p, nel, 100 + d * 10 + p)
    assert plain.feOrder is None and not caller.feOrder.is_identity
    assert np.array_equal(caller.feOrder.grid_of_fe, perm)
    assert np.array_equal(caller.V.tabulate_dof_coordinates(), X[perm])
    assert np.array_equal(caller._generator.feOrder.grid_of_fe, perm)
    f = lambda x: np.sin(np.pi * x)
    A = F.LaplaceForm().assemble_matrix(plain.V)
    b = F.SeparableLoadForm([f] * d, scale=d * np.pi ** 2).assemble_vector(plain.V)
    Ah, bh = A.to_scipy(), b.get_local()
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    Ap = Ah[perm][:, perm].tocsr()                    # permuted on the host: caller row i is grid node perm[i]
    bp = bh[perm]
    K0, y0 = plain.extractMatrix(A), plain.extractVector(b)
    for Aw, bw in ((FakeDolfinMatrix(Ap), FakeDolfinVector(bp)), (FakePETScMat(Ap), FakePETScVec(bp)),
                   (Ap, FakeGenericVector(bp))):
        K1, y1 = caller.extractMatrix(Aw), caller.extractVector(bw)
        assert same_csr(K1.to_scipy(), K0.to_scipy())
        assert K1.ptap_route == K0.ptap_route
        assert np.array_equal(bits(y1.get_local()), bits(y0.get_local()))
        assert getattr(K1, "tensor_structure", None) is not None and getattr(K0, "tensor_structure", None) is not None
    # assembleMatrix / assembleVector: an assembled object is the caller's, a form object numbers the grid itself
    assert same_csr(caller.assembleMatrix(FakeDolfinMatrix(Ap)).to_scipy(), K0.to_scipy())
    assert same_csr(caller.assembleMatrix(F.LaplaceForm()).to_scipy(), plain.assembleMatrix(F.LaplaceForm()).to_scipy())
    assert np.array_equal(bits(caller.assembleVector(FakeDolfinVector(bp)).get_local()), bits(y0.get_local()))
    assert np.array_equal(bits(caller.assembleVector(F.SeparableLoadForm([f] * d, scale=d * np.pi ** 2)).get_local()),
                          bits(y0.get_local()))
    # the solve: U identical, u in the caller's order
    its = []
    sols = []
    for spline, K, y in ((plain, K0, y0), (caller, K1, y1)):
        solver = t.PETScKrylovSolver("cg", "fast_diagonalization")
        solver.parameters["relative_tolerance"] = 1e-10
        spline.setSolverOptions(linearSolver=solver)
        u = t.Function(spline.V)
        U = spline.solveLinearSystem(K, y, u)
        its.append(solver.last["iterations"])
        sols.append((U.get_local(), u.vector().get_local()))
    assert its[0] == its[1] and its[0] > 0
    assert np.array_equal(bits(sols[0][0]), bits(sols[1][0]))
    assert np.array_equal(bits(sols[1][1]), bits(sols[0][1][perm]))
    # against the oracle on the permuted operands
    s = O.BSpline([p] * d, [O.uniform_knots(p, 0., 1., nel)] * d)
    Mo = O.generate_M([s], [X[perm]])
    zd = list(caller.zeroDofs)
    Ko = O.extract_matrix(Mo, Ap, zd)
    assert abs(K1.to_scipy() - Ko).max() <= 1e-12 * abs(Ko).max()
    assert np.max(np.abs(y1.get_local() - O.extract_vector(Mo, bp, zd))) <= 1e-12 * np.max(np.abs(bp))
    # 5: M with the caller's rows
    Mfe = caller.extractionMatrixFE().to_scipy()
    Mpts = T.dev.extract_csr_points(s_splines(T, p, d, nel), X[perm], 0, caller.M.shape[1], 1e-15).to_scipy()
    assert same_csr(Mfe, Mpts)
    assert same_csr(caller.M.to_scipy(), plain.M.to_scipy())            # (M itself stays in grid order)
    # 8: FEtoIGA reads the caller's order; so does a non-zero initial guess
    ug, uc = sols[0][1], sols[1][1]
    solver = t.PETScKrylovSolver("cg", "jacobi")
    solver.parameters["relative_tolerance"] = 1e-12
    back = []
    for spline, uvec in ((plain, ug), (caller, uc)):
        spline.setSolverOptions(linearSolver=solver)
        back.append(spline.FEtoIGA(T.dev.DeviceVector(data=uvec)).get_local())
    assert np.array_equal(bits(back[0]), bits(back[1]))
    guess_its = []
    for spline, K, y, uvec in ((plain, K0, y0, ug), (caller, K1, y1, uc)):
        ks = t.PETScKrylovSolver("cg", "jacobi")
        ks.parameters["relative_tolerance"] = 1e-8
        ks.parameters["nonzero_initial_guess"] = True
        spline.setSolverOptions(linearSolver=ks)
        u = t.Function(spline.V)
        u.vector().set_local(uvec)
        U = spline.solveLinearSystem(K, y, u)
        guess_its.append((ks.last["iterations"], U.get_local()))
    assert guess_its[0][0] == guess_its[1][0]           # (the seed M^T u is the same vector: u was read in the caller's order)
    assert np.array_equal(bits(guess_its[0][1]), bits(guess_its[1][1]))


def s_splines(T, p, d, nel):
    return T.B.BSpline([p] * d, [T.B.uniformKnots(p, 0.0, 1.0, nel) for _ in range(d)]).splines


def test_extraction_matrix_rows_on_golden_patches(T):
    """five reference patches: the rows of extractionMatrixFE() are the reference's rows of M in the permuted order"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_random.npz"))
    rng = np.random.default_rng(12)
    names = [str(n) for n in g["names"]]
    for name in names[3::11][:5]:
        degs = [int(v) for v in g[name + "/degrees"]]
        kvs = [[float(v) for v in g[name + "/kvec%d" % k]] for k in range(len(degs))]
        gen = T.t.EqualOrderSpline(1, T.B.ExplicitBSplineControlMesh(degs, kvs))
        X = gen.V.tabulate_dof_coordinates()
        perm = rng.permutation(X.shape[0])
        gen.setFENodes(X[perm])
        spline = T.t.ExtractedSpline(gen, 2)
        Mref = sp.csr_matrix((g[name + "/M_val"], g[name + "/M_col"], g[name + "/M_rowptr"]),
                             shape=(X.shape[0], gen.M.shape[1]))[perm].tocsr()
        Mref.sort_indices()
        assert same_csr(spline.extractionMatrixFE().to_scipy(), Mref), name


# ---- 6: several fields -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,p,nel", [(2, 2, 7), (3, 2, 4)])
def test_elasticity_rows_interleaved_node_by_node(T, d, p, nel):
    t, B, F = T.t, T.B, T.F
    kv = [B.uniformKnots(p, 0.0, 1.0, nel) for _ in range(d)]
    plain = t.EqualOrderSpline(d, B.ExplicitBSplineControlMesh([p] * d, kv))
    Xf = plain.V.tabulate_dof_coordinates()
    nn = Xf.shape[0] // d
    # an FE library numbers a vector space node by node: caller row d*j + f is node j of field f
    grid_of_fe = (np.tile(np.arange(d), nn) * nn + np.repeat(np.arange(nn), d)).astype(np.int64)
    with pytest.raises(ValueError) as e:
        t.EqualOrderSpline(d, B.ExplicitBSplineControlMesh([p] * d, kv), fe_nodes=Xf[grid_of_fe])
    assert "fe_fields" in str(e.value)
    caller = t.EqualOrderSpline(d, B.ExplicitBSplineControlMesh([p] * d, kv), fe_nodes=Xf[grid_of_fe],
                                fe_fields=np.tile(np.arange(d), nn))
    assert np.array_equal(caller.feOrder.grid_of_fe, grid_of_fe)
    for gen in (plain, caller):
        gen.addZeroDofs(0, gen.getScalarSpline(0).getSideDofs(0, 0))
    sp0, sp1 = t.ExtractedSpline(plain, 2 * p), t.ExtractedSpline(caller, 2 * p)
    A = F.ElasticityForm(lmbda=2.0, mu=1.0).assemble_matrix(sp0.V)
    Ap = A.to_scipy()[grid_of_fe][:, grid_of_fe].tocsr()
    K0 = sp0.extractMatrix(A, diag=1.5)
    K1 = sp1.extractMatrix(FakeDolfinMatrix(Ap), diag=1.5)
    assert same_csr(K1.to_scipy(), K0.to_scipy())
    assert K1.ptap_route == K0.ptap_route
    # (the 2-D product takes both fields in one pair of walks; in 3-D every field block names its own)
    assert getattr(K1, "ptap_block_routes", None) == getattr(K0, "ptap_block_routes", None)
    assert d == 2 or K0.ptap_block_routes is not None


# ---- 7: a coupling outside the element pattern -----------------------------------------------------------------------
def test_hand_added_coupling_3d_p3(T):
    plain, caller, perm, X = _poisson_pair(T, 3, 3, 4, 77)
    A2 = T.F.LaplaceForm().assemble_matrix(plain.V).to_scipy().tolil()
    A2[3, A2.shape[1] - 5] = 0.25
    A2 = A2.tocsr()
    K0 = plain.extractMatrix(A2, diag=1.5)
    K1 = caller.extractMatrix(FakePETScMat(A2[perm][:, perm].tocsr()), diag=1.5)
    assert same_csr(K1.to_scipy(), K0.to_scipy())
    assert K1.ptap_route == K0.ptap_route


# ---- 9: the identity, and no growth ----------------------------------------------------------------------------------
def test_identity_order_copies_nothing_and_repeats_leave_memory_alone(T):
    t, F, dev = T.t, T.F, T.dev
    plain, ident, perm, X = _poisson_pair(T, 3, 2, 6, 1, fe_nodes="identity")
    assert ident.feOrder is not None and ident.feOrder.is_identity and ident.feOrder.max_snap == 0.0
    A = F.LaplaceForm().assemble_matrix(plain.V)
    assert ident.feOrder.permute_matrix(A) is A
    grown = []
    for spline in (plain, ident):
        K = spline.extractMatrix(A)                       # (plans are made here)
        del K
        before = live_blocks(dev)
        K = spline.extractMatrix(A)
        grown.append(live_blocks(dev) - before)
        del K
    assert grown[0] == grown[1], grown                    # K and nothing else: no copy of A
    # ten repeats of the caller-ordered flow
    plain, caller, perm, X = _poisson_pair(T, 2, 2, 16, 3)
    Ap = FakeDolfinMatrix(F.LaplaceForm().assemble_matrix(plain.V).to_scipy()[perm][:, perm].tocsr())
    bp = FakeDolfinVector(F.SeparableLoadForm([np.sin] * 2).assemble_vector(plain.V).get_local()[perm])
    solver = t.PETScKrylovSolver("cg", "jacobi")
    caller.setSolverOptions(linearSolver=solver)

    def used():
        gc.collect()
        dev.sync()
        free, total = dev.mem_info()[:2]
        return total - free, dev.pool_stats()
    marks = []
    for it in range(12):
        K, y = caller.extractMatrix(Ap), caller.extractVector(bp)
        u = t.Function(caller.V)
        caller.solveLinearSystem(K, y, u)
        del K, y, u
        if it in (1, 11):
            marks.append(used())
    assert marks[0] == marks[1], marks


# ---- 10: refusals ----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(T):
    t, B, F = T.t, T.B, T.F
    from tigar_amd.implicit import LazyFEMatrix, LazyFEVector
    p, nel = 2, 6
    kv = [B.uniformKnots(p, 0.0, 1.0, nel)] * 2
    mesh = lambda: B.ExplicitBSplineControlMesh([p, p], kv)
    gen = t.EqualOrderSpline(1, mesh())
    X = gen.V.tabulate_dof_coordinates()
    n = X.shape[0]
    perm = np.random.default_rng(4).permutation(n)
    for x, reason in ((X[perm][:-1], "wrong row count"), (X[perm][:, :1], "wrong shape"),
                      (np.vstack([X[perm][:-1], X[perm][:1]]), "two rows on one node"),
                      (X[perm] + 0.4 / (nel * p), "off the grid")):
        with pytest.raises(ValueError) as e:
            t.EqualOrderSpline(1, mesh(), fe_nodes=x)
        assert reason in str(e.value), (reason, str(e.value))
    # a node set of another mesh (as many nodes, other knots) is off by a fraction of a spacing
    knots = [0.0, 0.0, 0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0, 1.0]
    other = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p, p], [knots, knots]))
    assert other.V.dim() == n
    with pytest.raises(ValueError) as e:
        gen.setFENodes(other.V.tabulate_dof_coordinates())
    assert "off the grid" in str(e.value)
    assert gen.feOrder is None
    with pytest.raises(ValueError) as e:
        t.EqualOrderSpline(2, mesh(), fe_nodes=np.vstack([X, X]))
    assert "fe_fields" in str(e.value)
    # DG and multi-patch node sets are no permutation of one grid
    dg = t.EqualOrderSpline(1, mesh())
    dg.V.grids[0].dg = True
    with pytest.raises(ValueError) as e:
        dg.setFENodes(X)
    assert "DG" in str(e.value)
    dg.V.grids[0] = object()                               # (what a multi-patch or T-spline space holds is no TensorNodeGrid)
    with pytest.raises(ValueError) as e:
        dg.setFENodes(X)
    assert "TensorNodeGrid" in str(e.value)
    # several ranks
    many = t.EqualOrderSpline(1, mesh())
    many.comm = t.common._Comm(2, 0)
    with pytest.raises(NotImplementedError) as e:
        many.setFENodes(X[perm])
    assert "several ranks" in str(e.value)
    # lazy operands and the nonlinear drivers on a caller-ordered spline
    spline = t.ExtractedSpline(t.EqualOrderSpline(1, mesh(), fe_nodes=X[perm]), 2 * p)
    with pytest.raises(NotImplementedError) as e:
        spline.extractMatrix(LazyFEMatrix(lambda r0, r1: None, (n, n)))
    assert "LazyFEMatrix" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        spline.extractVector(LazyFEVector(lambda r0, r1: None, n))
    assert "LazyFEVector" in str(e.value)
    u = t.Function(spline.V)
    with pytest.raises(NotImplementedError) as e:
        spline.solveNonlinearVariationalProblem(F.LaplaceForm(), F.LaplaceForm(), u)
    assert "caller-ordered" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        t.ExtractedNonlinearProblem(spline, None, None, u)
    assert "caller-ordered" in str(e.value)
    # what is no matrix raises the TypeError of before
    for s_ in (spline, t.ExtractedSpline(gen, 2 * p)):
        with pytest.raises(TypeError):
            s_.extractMatrix(object())
