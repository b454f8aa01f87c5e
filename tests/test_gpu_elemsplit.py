"""-m gpu: the cell-block product for CONNECTED meshes (tigar_amd/elemptap.py, csrc tg_elemsplit_*): A assembled on a mesh whose
cells share nodes is split into one dense block per cell (every entry to the lowest cell holding both nodes) and
K = M^T A M = sum_c (R_c M)^T A_c (R_c M) runs as dense cell products -- MatPtAP of tIGAr/common.py:1194-1195 for ANY values of
A and an M that is used as a general CSR matrix.  Checked against scipy's triple product and the general
kernels: pattern and values, non-symmetric A, MatZeroRowsColumns fused, a matrix with an entry outside every cell declined."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


def _operands(d, p, nels, seed=0):
    from tigar_amd import device as dev
    from tigar_amd.common import TensorFunctionSpace, _cell_dofs_arrays
    from tigar_amd.BSplines import ExplicitBSplineControlMesh, uniformKnots
    from tigar_amd.forms import LaplaceForm
    cm = ExplicitBSplineControlMesh([p] * d, [uniformKnots(p, 0., 1., n) for n in nels])
    basis = cm.getScalarSpline()
    grid = basis.generateMesh(degree=p)
    V = TensorFunctionSpace([grid], "Lagrange")
    A = LaplaceForm().assemble_matrix(V)
    M = dev.extract_csr_tensor(basis.splines, grid.axes, 0, basis.getNcp(), 1e-15)
    return A, M, _cell_dofs_arrays(grid)


@pytest.mark.parametrize("d,p,nels", [(3, 3, (5, 4, 6)), (3, 2, (7, 5, 6)), (2, 3, (17, 12)), (3, 1, (9, 8, 7)), (2, 2, (20, 15)),
                                      (3, 4, (3, 2, 4)), (2, 5, (7, 6)), (2, 7, (5, 4)),       # (125-node cells: the panel kernel)
                                      (3, 4, (5, 5, 3))])      # (a function in 75 cells of 125 functions: the two-list merge)
def test_element_split_product_matches_scipy(d, p, nels):
    from tigar_amd import device as dev
    from tigar_amd.elemptap import ElementSplitPtAP
    A, M, cells = _operands(d, p, nels)
    rng = np.random.default_rng(d * 10 + p)
    As = A.to_scipy().tocsr()
    As.sort_indices()
    As.data = As.data * (1.0 + 0.3 * rng.standard_normal(As.nnz)) + 0.01 * rng.standard_normal(As.nnz)     # not symmetric
    A2 = dev.DeviceCSR.from_scipy(As)
    Ms = M.to_scipy().tocsr()
    plan = ElementSplitPtAP(M, cells)
    assert plan.b == (p + 1) ** d
    K = plan.ptap(A2)
    assert K is not None
    Ks = K.to_scipy().tocsr()
    assert all(np.all(np.diff(Ks.indices[a:b]) > 0) for a, b in zip(Ks.indptr[:-1], Ks.indptr[1:]))        # canonical rows
    Ks.sort_indices()
    ref = (Ms.T @ As @ Ms).tocsr()
    ref.sort_indices()
    pat = (abs(Ms).T @ sp.csr_matrix((np.ones(As.nnz), As.indices, As.indptr), shape=As.shape) @ abs(Ms)).tocsr()
    pat.sort_indices()
    assert np.array_equal(Ks.indptr, pat.indptr) and np.array_equal(Ks.indices, pat.indices)       # the structural pattern
    assert abs(Ks - ref).max() <= 1e-12 * abs(ref).max()
    # the general kernels give the same matrix
    MT = M.transpose()
    Kg = dev.ptap_numeric(dev.ptap_symbolic(A2, M, MT), A2, M, MT).to_scipy().tocsr()
    assert abs(Ks - Kg).max() <= 1e-12 * abs(ref).max()
    # a second product on the plan (places known): bit for bit the same; other values, same pattern: the splitting is reused
    K2 = plan.ptap(A2).to_scipy().tocsr()
    K2.sort_indices()
    assert np.array_equal(K2.data.view(np.int64), Ks.data.view(np.int64))
    As3 = As.copy()
    As3.data = rng.standard_normal(As.nnz)
    K3 = plan.ptap(dev.DeviceCSR.from_scipy(As3)).to_scipy()
    ref3 = (Ms.T @ As3 @ Ms)
    assert abs(K3 - ref3).max() <= 1e-12 * abs(ref3).max()
    # MatZeroRowsColumns fused (tIGAr/common.py:1196-1200)
    zd = np.unique(rng.integers(0, Ms.shape[1], 25)).astype(np.int32)
    Kz = plan.ptap(A2, zero_dofs=zd, diag=1.0).to_scipy().tolil()
    refz = ref.tolil()
    refz[zd, :] = 0.0
    refz[:, zd] = 0.0
    for i in zd:
        refz[i, i] = 1.0
    assert abs(Kz.tocsr() - refz.tocsr()).max() <= 1e-12 * abs(ref).max()


def test_another_pattern_of_the_same_size_is_split_again():
    """the splitting maps block positions to entries of the matrix it was made for; a matrix with as many rows and entries but
    another pattern (here: one coupling moved within a cell) must not be read through it -- the reference redoes the symbolic
    product at every call (tIGAr/common.py:1194-1195)"""
    from tigar_amd import device as dev
    from tigar_amd.elemptap import ElementSplitPtAP
    A, M, cells = _operands(2, 2, (9, 7))
    Ms = M.to_scipy().tocsr()
    full = A.to_scipy().tocsr()
    c = cells[5]
    e1, e2 = (int(c[0]), int(c[3])), (int(c[4]), int(c[7]))
    assert full[e1] != 0.0 and full[e2] != 0.0

    def without(entry):
        L = full.tolil()
        L[entry] = 0.0
        L = L.tocsr()
        L.eliminate_zeros()
        return L

    B1, B2 = without(e1), without(e2)                 # as many rows and entries, another pattern
    assert B1.nnz == B2.nnz == full.nnz - 1
    plan = ElementSplitPtAP(M, cells)
    for B in (B1, B2, B1):
        K = plan.ptap(dev.DeviceCSR.from_scipy(B)).to_scipy()
        ref = Ms.T @ B @ Ms
        assert abs(K - ref).max() <= 1e-12 * abs(ref).max()


def test_an_entry_outside_every_cell_is_declined():
    from tigar_amd import device as dev
    from tigar_amd.elemptap import ElementSplitPtAP
    A, M, cells = _operands(2, 2, (8, 8))
    As = A.to_scipy().tolil()
    n = As.shape[0]
    As[0, n - 1] = 1.0                               # opposite corners of the mesh: no common cell
    plan = ElementSplitPtAP(M, cells)
    assert plan.ptap(dev.DeviceCSR.from_scipy(As.tocsr())) is None
    assert plan.ptap(A) is not None


def _star(n, seed=0):
    """a star mesh: n cells of two nodes [0, i], node 0 in every cell; M a random CSR of 2 to 3 entries per row with sorted
    columns, A random on the couplings of the cells ((0, 0), (0, i), (i, 0), (i, i))"""
    rng = np.random.default_rng(1000 * n + seed)
    ncp = 24
    cells = np.stack([np.zeros(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)], axis=1)
    rows, cols = [], []
    for r in range(n + 1):
        c = np.sort(rng.choice(ncp, size=int(rng.integers(2, 4)), replace=False))
        rows += [r] * c.size
        cols += list(c)
    Ms = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(n + 1, ncp))
    Ms.sort_indices()
    i = np.arange(1, n + 1)
    ar = np.concatenate([[0], np.zeros(n, dtype=np.int64), i, i])
    ac = np.concatenate([[0], i, np.zeros(n, dtype=np.int64), i])
    As = sp.csr_matrix((rng.standard_normal(ar.size), (ar, ac)), shape=(n + 1, n + 1))
    As.sort_indices()
    return cells, Ms, As


def test_a_node_in_forty_cells_takes_the_list_tables(monkeypatch, capfd):
    """node 0 lies in 40 cells (more than the 8 of the node table): the node -> cells lists stay lists and ``k_el_scatter``
    splits A, chosen by the data alone (the trace line of the product names it); K against scipy, a second product bit for
    bit the same"""
    from tigar_amd import device as dev
    from tigar_amd.elemptap import CellNodes, ElementSplitPtAP
    cells, Ms, As = _star(40)
    plan = ElementSplitPtAP(dev.DeviceCSR.from_scipy(Ms), CellNodes.from_host(cells))
    assert plan.b == 2 and plan._chunk.ninc_max >= 40
    A = dev.DeviceCSR.from_scipy(As)
    monkeypatch.setenv("TIGAR_TRACE", "1")
    capfd.readouterr()
    K = plan.ptap(A)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[tigar] element split:")]
    monkeypatch.delenv("TIGAR_TRACE")
    assert len(lines) == 1 and "split k_el_scatter," in lines[0]
    assert K is not None
    Ks = K.to_scipy().tocsr()
    Ks.sort_indices()
    ref = (Ms.T @ As @ Ms).tocsr()
    assert Ks.shape == ref.shape
    assert abs(Ks - ref).max() <= 1e-12 * abs(ref).max()
    K2 = plan.ptap(A).to_scipy().tocsr()
    K2.sort_indices()
    assert np.array_equal(K2.indptr, Ks.indptr) and np.array_equal(K2.indices, Ks.indices)
    assert np.array_equal(K2.data.view(np.int64), Ks.data.view(np.int64))


def test_a_node_in_seventy_cells_is_declined():
    """a node in more than 64 cells: the splitting pass declines (``ptap`` returns None), the general kernels give scipy's K"""
    from tigar_amd import device as dev
    from tigar_amd.elemptap import CellNodes, ElementSplitPtAP
    cells, Ms, As = _star(70)
    M, A = dev.DeviceCSR.from_scipy(Ms), dev.DeviceCSR.from_scipy(As)
    plan = ElementSplitPtAP(M, CellNodes.from_host(cells))
    assert plan.ptap(A) is None
    MT = M.transpose()
    Kg = dev.ptap_numeric(dev.ptap_symbolic(A, M, MT), A, M, MT).to_scipy().tocsr()
    ref = (Ms.T @ As @ Ms).tocsr()
    assert abs(Kg - ref).max() <= 1e-12 * abs(ref).max()


def test_a_function_in_more_than_128_cells_does_not_qualify():
    from tigar_amd import device as dev
    from tigar_amd.elemptap import CellNodes, ElementChunk
    cells, Ms, _ = _star(130)
    with pytest.raises(ValueError):
        ElementChunk(CellNodes.from_host(cells), dev.DeviceCSR.from_scipy(Ms))


@pytest.mark.parametrize("d,p,nel", [(3, 2, 6), (2, 3, 14), (3, 3, 4)])
def test_extract_matrix_takes_the_element_split_product(monkeypatch, d, p, nel):
    """through the API (tIGAr/common.py:1194-1200): with the Kronecker paths switched off ``extractMatrix`` on an assembled
    matrix runs the element-split product; a matrix with couplings beyond the cells (a band) falls through to the general
    kernels; both equal scipy's triple product, Dirichlet rows and columns fused"""
    import tigar_amd as t
    from tigar_amd import BSplines as B, forms as F
    monkeypatch.setenv("TIGAR_PTAP_TENSOR", "0")
    monkeypatch.setenv("TIGAR_PTAP_FACTORED", "0")
    monkeypatch.setenv("TIGAR_PTAP_ELEMENTS", "2")
    gen = t.EqualOrderSpline(1, B.ExplicitBSplineControlMesh([p] * d, [B.uniformKnots(p, 0., 1., nel)] * d))
    s0 = gen.getScalarSpline(0)
    for side in (0, 1):
        gen.addZeroDofs(0, s0.getSideDofs(0, side))
    spline = t.ExtractedSpline(gen, 2 * p)
    A = F.LaplaceForm().assemble_matrix(spline.V).to_scipy().tocsr()
    rng = np.random.default_rng(p)
    A.data = A.data + 0.1 * rng.standard_normal(A.nnz)
    Kd = spline.extractMatrix(A)
    K = Kd.to_scipy().tocsr()
    assert Kd.ptap_route == "elements"                                                      # the element path ran
    M = gen.M.to_scipy()
    ref = (M.T @ A @ M).tolil()
    zd = np.asarray(gen.zeroDofsArray(), dtype=np.int64)
    ref[zd, :] = 0.0
    ref[:, zd] = 0.0
    for i in zd:
        ref[i, i] = 1.0
    ref = ref.tocsr()
    assert abs(K - ref).max() <= 1e-12 * abs(ref).max()
    # a band that reaches beyond the cells: declined by the splitting, the general kernels take it
    i = np.arange(p * nel + 1)
    C1 = sp.csr_matrix(np.abs(i[:, None] - i[None, :]) <= p)
    P = C1
    for _ in range(d - 1):
        P = sp.kron(C1, P, format="csr")
    Bm = P.astype(np.float64).tocsr()
    Bm.data = rng.standard_normal(Bm.nnz)
    K2d = spline.extractMatrix(Bm)
    K2 = K2d.to_scipy().tocsr()
    assert K2d.ptap_route == "general"
    ref2 = (M.T @ Bm @ M).tolil()
    ref2[zd, :] = 0.0
    ref2[:, zd] = 0.0
    for i2 in zd:
        ref2[i2, i2] = 1.0
    assert abs(K2 - ref2.tocsr()).max() <= 1e-12 * abs(ref2).max()


def test_element_split_at_a_size_the_oracle_does_not_reach():
    """32^3 elements, p = 3 (0.9 M FE rows, 1.1e8 entries of A, 32 768 cells of 64 nodes: the one-cell-per-workgroup kernel and
    the 16-bit places): K x = M^T (A (M x)) for random x, the entry count of the general kernels' K, symmetry carried over from
    A, and the same bits in a second product"""
    from tigar_amd import device as dev
    from tigar_amd.elemptap import ElementSplitPtAP
    A, M, cells = _operands(3, 3, (32, 32, 32))
    plan = ElementSplitPtAP(M, cells)
    assert plan.b == 64 and plan.nfmax == 64
    K = plan.ptap(A)
    rng = np.random.default_rng(1)
    for _ in range(2):
        x = dev.DeviceVector(data=rng.standard_normal(K.shape[0]))
        y1 = K.mult(x).get_local()
        y2 = M.mult_transpose(A.mult(M.mult(x))).get_local()
        assert np.max(np.abs(y1 - y2)) <= 1e-13 * np.max(np.abs(y2))
    MT = M.transpose()
    Kg = dev.ptap_numeric(dev.ptap_symbolic(A, M, MT), A, M, MT)
    assert Kg.nnz == K.nnz
    xs, ys = rng.standard_normal(K.shape[0]), rng.standard_normal(K.shape[0])
    a1 = float(ys @ K.mult(dev.DeviceVector(data=xs)).get_local())
    a2 = float(xs @ K.mult(dev.DeviceVector(data=ys)).get_local())
    assert abs(a1 - a2) <= 1e-11 * (abs(a1) + abs(a2))
    K2 = plan.ptap(A)
    r = K.shape[0] // 2
    assert np.array_equal(K.rows_to_scipy(r, r + 2000).data.view(np.int64), K2.rows_to_scipy(r, r + 2000).data.view(np.int64))


@pytest.mark.parametrize("d,p,nels", [(3, 2, (4, 3, 5)), (2, 3, (6, 5)), (3, 1, (3, 4, 2)), (1, 4, (9,))])
def test_cell_node_lists_generated_on_the_device(d, p, nels):
    """``CellNodes.from_grid`` (the dofmap of the Q_p stand-in, generated by a kernel) against the host arrays of
    ``common._cell_dofs_arrays``: all cells, and a box of elements"""
    from tigar_amd.common import _cell_dofs_arrays
    from tigar_amd.BSplines import ExplicitBSplineControlMesh, uniformKnots
    from tigar_amd.elemptap import CellNodes
    cm = ExplicitBSplineControlMesh([p] * d, [uniformKnots(p, 0., 1., n) for n in nels])
    grid = cm.getScalarSpline().generateMesh(degree=p)
    ref = _cell_dofs_arrays(grid)
    got = CellNodes.from_grid(grid).to_host()
    assert got.shape == ref.shape and np.array_equal(got, ref)
    lo = [n // 3 for n in nels]
    hi = [max(l + 1, n - 1) for l, n in zip(lo, nels)]
    box = CellNodes.from_grid(grid, lo, hi).to_host()
    e = np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij")
    idx = sum(c.ravel(order="F") * int(np.prod(nels[:k])) for k, c in enumerate(e))
    assert np.array_equal(box, ref[idx])


@pytest.mark.parametrize("d,p,nels,cuts", [(3, 2, (5, 4, 9), (0, 3, 4, 9)), (2, 3, (7, 12), (0, 5, 12)), (3, 3, (3, 3, 7), (0, 2, 5, 7)),
                                           (3, 1, (4, 4, 6), (0, 1, 2, 6))])
def test_chunks_of_cells_add_up_to_the_whole_product(d, p, nels, cuts):
    """The mesh worked off in chunks of element layers of the last direction (``ElementChunk``): a chunk lists the layer below
    it as well (ownership of the entries on the shared node plane), sees only the rows of A and M of its own cells' nodes, and
    checks the rows whose cells are all listed; the chunks' K -- rows of their own functions, global columns -- add up to
    M^T A M.  An entry without a common cell is declined by the chunk that checks its row."""
    from tigar_amd import device as dev
    from tigar_amd.elemptap import CellNodes, ElementChunk
    A, M, _ = _operands(d, p, nels)
    rng = np.random.default_rng(p + d)
    As = A.to_scipy().tocsr()
    As.sort_indices()
    As.data = As.data * (1.0 + 0.3 * rng.standard_normal(As.nnz)) + 0.01 * rng.standard_normal(As.nnz)
    Ms = M.to_scipy().tocsr()
    ref = (Ms.T @ As @ Ms).tocsr()
    from tigar_amd.BSplines import ExplicitBSplineControlMesh, uniformKnots
    grid = ExplicitBSplineControlMesh([p] * d, [uniformKnots(p, 0., 1., n) for n in nels]).getScalarSpline().generateMesh(degree=p)
    plane = int(np.prod(grid.shape()[:-1]))
    per_layer = int(np.prod(nels[:-1]))
    total = sp.csr_matrix(ref.shape)
    bad = As.tolil()
    r_bad = (cuts[1] * p) * plane + 1                     # a row on the node plane two chunks share
    bad[r_bad, As.shape[0] - 1] = 1.0
    bad = bad.tocsr()
    declined = 0
    for e0, e1 in zip(cuts[:-1], cuts[1:]):
        f0 = max(e0 - 1, 0)
        lo, hi = [0] * (d - 1) + [f0], list(nels[:-1]) + [e1]
        cells = CellNodes.from_grid(grid, lo, hi)
        r0, r1 = e0 * p * plane, (e1 * p + 1) * plane
        Mc = dev.DeviceCSR.from_scipy(Ms[r0:r1])
        chunk = ElementChunk(cells, Mc, r0, own=((e0 - f0) * per_layer, (e1 - f0) * per_layer))
        chk = (r0, r1 if e1 == nels[-1] else e1 * p * plane)
        K = chunk.ptap(dev.DeviceCSR.from_scipy(As[r0:r1]), r0, chk)
        assert K is not None and K.shape == (chunk.dofs[1] - chunk.dofs[0], ref.shape[1])
        Kc = K.to_scipy().tocsr()
        total = total + sp.vstack([sp.csr_matrix((chunk.dofs[0], ref.shape[1])), Kc,
                                   sp.csr_matrix((ref.shape[0] - chunk.dofs[1], ref.shape[1]))]).tocsr()
        declined += chunk.ptap(dev.DeviceCSR.from_scipy(bad[r0:r1]), r0, chk) is None
    assert abs(total - ref).max() <= 1e-12 * abs(ref).max()
    assert declined == 1


@pytest.mark.parametrize("d,p,nels,layers,world", [(3, 2, (5, 4, 11), 3, 1), (3, 3, (3, 4, 9), 2, 3), (2, 3, (9, 14), 4, 2),
                                                    (3, 1, (4, 3, 8), 1, 2), (3, 2, (4, 4, 6), 100, 1), (3, 4, (2, 2, 7), 2, 2)])
def test_streamed_element_chunks_in_the_slab_engine(monkeypatch, d, p, nels, layers, world):
    """``dist.SlabHotPath`` with nothing assumed about M (``factored=False``): the element split over chunks of ``layers`` element
    layers -- M materialised chunk by chunk, A handed out in row blocks, the planes at a chunk's top carried and added, the rows
    of every rank of a ``world`` of ranks computed without any exchange.  Against scipy's triple product with MatZeroRowsColumns;
    non-symmetric values; M^T b as well.  An A with a coupling beyond the cells falls through to the row-wise stages."""
    from tigar_amd import device as dev
    from tigar_amd.dist import SlabHotPath
    from tigar_amd.BSplines import ExplicitBSplineControlMesh, uniformKnots
    monkeypatch.setenv("TIGAR_ELEM_LAYERS", str(layers))
    monkeypatch.setenv("TIGAR_PTAP_ELEMENTS", "2")
    A, M, _ = _operands(d, p, nels)
    rng = np.random.default_rng(7 * p + d)
    As = A.to_scipy().tocsr()
    As.sort_indices()
    As.data = As.data * (1.0 + 0.3 * rng.standard_normal(As.nnz)) + 0.01 * rng.standard_normal(As.nnz)
    Ms = M.to_scipy().tocsr()
    b = rng.standard_normal(As.shape[0])
    zd = np.unique(rng.integers(0, Ms.shape[1], 17)).astype(np.int32)
    ref = (Ms.T @ As @ Ms).tolil()
    ref[zd, :] = 0.0
    ref[:, zd] = 0.0
    for i in zd:
        ref[i, i] = 2.5
    ref = ref.tocsr()
    yref = Ms.T @ b
    yref[zd] = 0.0
    basis = ExplicitBSplineControlMesh([p] * d, [uniformKnots(p, 0., 1., n) for n in nels]).getScalarSpline()
    grid = basis.generateMesh(degree=p)
    calls = []

    def a_rows(r0, r1, mat=As):
        calls.append((r0, r1))
        return dev.DeviceCSR.from_scipy(mat[int(r0):int(r1)])

    def b_rows(r0, r1):
        return dev.DeviceVector(data=b[int(r0):int(r1)])

    Krows, yparts = [], []
    for rank in range(world):
        eng = SlabHotPath(basis, grid, rank, world, None, sub_planes=2, factored=False)
        timers = {}
        K, y = eng.assemble(a_rows, b_rows, zd, 2.5, timers)
        assert K.shape == (eng.mine["dofs"][1] - eng.mine["dofs"][0], Ms.shape[1])
        Krows.append(K.to_scipy().tocsr())
        yparts.append(y.get_local())
    Kall = sp.vstack(Krows).tocsr()
    Kall.sort_indices()
    pat = (abs(Ms).T @ sp.csr_matrix((np.ones(As.nnz), As.indices, As.indptr), shape=As.shape) @ abs(Ms)).tocsr()
    pat.sort_indices()
    assert np.array_equal(Kall.indptr, pat.indptr) and np.array_equal(Kall.indices, pat.indices)     # the structural pattern
    assert abs(Kall - ref).max() <= 1e-12 * abs(ref).max()
    assert np.max(np.abs(np.concatenate(yparts) - yref)) <= 1e-12 * np.max(np.abs(yref))
    # the blocks asked for were element layers (+ the node plane on top), several of them unless one chunk covers the rank
    plane = int(np.prod(grid.shape()[:-1]))
    assert all((r1 - r0) % plane == 0 and ((r1 - r0) // plane - 1) % p == 0 for r0, r1 in calls)
    if layers < nels[-1] // world:
        assert len(calls) > world
    # a coupling between nodes of no common cell: declined by the chunk that checks its row, same result from the row-wise stages
    bad = As.tolil()
    bad[1, As.shape[0] - 2] = 0.75
    bad = bad.tocsr()
    eng = SlabHotPath(basis, grid, 0, 1, None, sub_planes=3, factored=False)
    K2 = eng.assemble(lambda r0, r1: a_rows(r0, r1, bad), None, None, 1.0, {})[0].to_scipy()
    ref2 = Ms.T @ bad @ Ms
    assert abs(K2 - ref2).max() <= 1e-12 * abs(ref2).max()


def test_several_fields_on_element_chunks(monkeypatch):
    """Three fields on one basis (elasticity, tIGAr/common.py:1891-1914) with the operator kept implicit and NOTHING assumed about
    M or A in the product (``TIGAR_PTAP_FACTORED=0``): every field block (f, g) = M_s^T A_fg M_s runs through the element chunks
    of the scalar engine, all nine on ONE pass (``dist.FieldSlabPath`` -> ``SlabHotPath.assemble_blocks_by_elements``: a chunk's
    plan depends on M only), the blocks are interleaved plane by plane.  Against the resident path's K; an explicit scipy A
    takes the same way."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import gpu_rank_worker_fields as W
    from tigar_amd import common as tc, dist
    gen, spline, K, rhs, method = W.problem("elasticity3d", tc.selfcomm)
    Kref = K.to_scipy().tocsr()
    monkeypatch.setenv("TIGAR_IMPLICIT_M", "1")
    monkeypatch.setenv("TIGAR_PTAP_FACTORED", "0")
    monkeypatch.setenv("TIGAR_PTAP_TENSOR", "0")
    monkeypatch.setenv("TIGAR_PTAP_ELEMENTS", "2")
    monkeypatch.setenv("TIGAR_ELEM_LAYERS", "2")
    calls = []
    orig = dist.SlabHotPath.assemble_blocks_by_elements

    def spy(self, producers, *a, **k):
        out = orig(self, producers, *a, **k)
        calls.append((len(producers), out is not None))
        return out
    monkeypatch.setattr(dist.SlabHotPath, "assemble_blocks_by_elements", spy)
    gen2, spline2, K2, rhs2, _ = W.problem("elasticity3d", tc.selfcomm)
    assert getattr(gen2.M, "is_implicit", False)
    assert calls == [(9, True)]                              # nine field blocks on ONE pass over the element chunks
    dofs = spline2.localDofIndices()
    n2o = spline2._slab_path().new_of_old()
    n = Kref.shape[0]
    old_of_new = np.empty(n, dtype=np.int64)
    old_of_new[n2o] = np.arange(n)
    Kr = Kref[dofs][:, old_of_new].tocsr()
    K2s = K2.to_scipy().tocsr()
    assert abs(K2s - Kr).max() <= 1e-12 * abs(Kref).max()
    from tigar_amd import forms as F
    A3 = F.ElasticityForm(2.0, 1.0).assemble_matrix(spline.V).to_scipy()
    K3 = spline2.extractMatrix(A3, diag=1.5).to_scipy().tocsr()
    assert abs(K3 - Kr).max() <= 1e-12 * abs(Kref).max()
    assert calls[-1] == (9, True)


@pytest.mark.parametrize("p,drops,nels,world", [(2, (0, 0, 1), (4, 3, 7), 2), (3, (1, 0, 2), (3, 3, 6), 1), (2, (1, 1, 1), (4, 4, 5), 3)])
def test_repeated_interior_knots_on_the_streamed_path(monkeypatch, p, drops, nels, world):
    """Knot vectors with REPEATED interior knots (``uniformKnots(..., continuityDrop > 0)``, tIGAr/BSplines.py:14-38): the tensor
    walks do not take them, the element chunks do not care -- M comes from the general extraction kernels, the cells' function
    lists from its rows.  Streamed in chunks of two element layers on 1-3 ranks against scipy (VERDICT r5 missing #5: such
    patches took the row-wise stages at scale)."""
    from tigar_amd import device as dev
    from tigar_amd.dist import SlabHotPath
    from tigar_amd.common import TensorFunctionSpace
    from tigar_amd.BSplines import ExplicitBSplineControlMesh, uniformKnots
    from tigar_amd.forms import LaplaceForm
    monkeypatch.setenv("TIGAR_ELEM_LAYERS", "2")
    monkeypatch.setenv("TIGAR_PTAP_ELEMENTS", "2")
    kvs = [uniformKnots(p, 0., 1., n, False, dr) for n, dr in zip(nels, drops)]
    basis = ExplicitBSplineControlMesh([p] * 3, kvs).getScalarSpline()
    grid = basis.generateMesh(degree=p)
    A = LaplaceForm().assemble_matrix(TensorFunctionSpace([grid], "Lagrange")).to_scipy().tocsr()
    rng = np.random.default_rng(p)
    A.data = A.data * (1.0 + 0.3 * rng.standard_normal(A.nnz))
    Ms = dev.extract_csr_tensor(basis.splines, grid.axes, 0, basis.getNcp(), 1e-15).to_scipy().tocsr()
    assert Ms.shape[1] == int(np.prod([n + p + dr * (n - 1) for n, dr in zip(nels, drops)]))     # (more functions: lower continuity)
    ref = (Ms.T @ A @ Ms).tocsr()
    rows = []
    for rank in range(world):
        eng = SlabHotPath(basis, grid, rank, world, None, sub_planes=2, factored=False)
        K = eng.assemble(lambda r0, r1: dev.DeviceCSR.from_scipy(A[int(r0):int(r1)]), None, None, 1.0, {})[0]
        rows.append(K.to_scipy().tocsr())
    Kall = sp.vstack(rows).tocsr()
    assert Kall.shape == ref.shape and abs(Kall - ref).max() <= 1e-12 * abs(ref).max()
